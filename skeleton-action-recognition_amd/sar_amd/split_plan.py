"""What a split-arithmetic ST-GCN engine (mfma="f32_split*", sar_amd/stgcn.py) decides once, when it is constructed: per block, which
launch runs on the split kernels with which ready keyword arguments, and which operand-bound cells exist.  The step only reads it.

The kinds of SAR_SPLIT_KINDS name the nine launches of a block: {g, t, r} x {fwd, dgrad, wgrad} = graph convolution, temporal
convolution, 1x1 residual convolution x forward, data gradient, weight gradient.  A launch is ON when its kind is switched on and the
split kernels are built for its shape (its term images exist in the PackedSplitWeights; for a graph or temporal weight gradient, the
images of both orientations).

Cells.  The fp16 arithmetic (f16x3a) scales each operand by a bound of its magnitude: the bits of a float in a one-element int32
tensor, zeroed at the start of a training step and only ever RAISED by the pass that produces the operand.  A weight's bound comes
with its term images; the five activation operands of a block have a cell each, named by what it bounds:

  cell  bounds                          raised by                                          read by (its consumers)
  X     the block input                 the tail of the block below (block 0: ops.amax)    gfwd, gwgrad, rfwd, rwgrad
  g     relu(bn1(graph conv output))    ops.bn_bound (Samuelson, from gamma / beta)        tfwd, twgrad
  du    gradient of the temporal conv   the backward tail pass (bn_add_relu_bwd_apply)     tdgrad, twgrad
  dg    gradient of the graph conv      the BN1-backward apply pass (affine2)              gdgrad, gwgrad
  dr    gradient of the residual conv   the backward tail pass                             rdgrad, rwgrad

A cell exists -- and is raised -- exactly when at least one of its consumers is ON (_CONSUMERS below is the one place that says so);
otherwise the record holds None and the producer's `amax_cell=None` raises nothing.  The bf16x6 arithmetic scales nothing: no cells."""
import torch

from . import ops

_CONSUMERS = {"X": ("gfwd", "gwgrad", "rfwd", "rwgrad"), "g": ("tfwd", "twgrad"), "du": ("tdgrad", "twgrad"),
              "dg": ("gdgrad", "gwgrad"), "dr": ("rdgrad", "rwgrad")}
# the launches: kind -> (the weight images it needs, source cell); a weight gradient -> (.., source cell, output-gradient cell)
_GEMMS = {"gfwd": ("gcn.f", "X"), "tfwd": ("tcn.f", "g"), "rfwd": ("res.f", "X"),
          "gdgrad": ("gcn.b", "dg"), "tdgrad": ("tcn.b", "du"), "rdgrad": ("res.b", "dr")}
_WGRADS = {"gwgrad": (("gcn.f", "gcn.b"), "X", "dg"), "twgrad": (("tcn.f", "tcn.b"), "g", "du"), "rwgrad": (("res.f",), "X", "dr")}


class BlockPlan:
    """One block's record; plain attributes, fixed at construction.  The default is a block with nothing on the split kernels (every
    block of an engine without a plan, and every block at inference).
      gfwd tfwd rfwd gdgrad tdgrad rdgrad   None = the fp32 / bf16-operand kernel, else dict(split=, packed=, bounds=(src cell, w_bound))
      gwgrad twgrad rwgrad                  None, else dict(split=, bounds=(src cell, dout cell) or None); rwgrad also needs T == s * To
      X g du dg dr                          the cell (one-element view) or None
      y                                     the cell of the NEXT block's X, raised by this block's tail; amax_X: this block raises its
                                            own X in front of its graph convolution (block 0)
      bn1                                   (gamma, beta) of bn1: what g's bound is computed from
      compact_skip                          the skip gradient of this (stride-2, conv-residual) block as its even frames only
      join_aux                              the third-stream fork is joined in front of this block's graph convolution: the launch reads
                                            a term image, or raises a cell the fork zeroes"""
    __slots__ = tuple(_GEMMS) + tuple(_WGRADS) + tuple(_CONSUMERS) + ("y", "amax_X", "bn1", "compact_skip", "join_aux")

    def __init__(self, compact_skip=False):
        for a in self.__slots__:
            setattr(self, a, None)
        self.amax_X = self.join_aux = False
        self.compact_skip = compact_skip


OFF = BlockPlan()


class SplitPlan:
    """packed: the PackedSplitWeights of the engine; cells: the int32 cell tensor (None: bf16x6); blocks: one BlockPlan per block"""

    def __init__(self, eng, packed, kinds):
        self.packed, self.V, self.strides = packed, eng.V, [s for _, s, _ in eng.blocks]
        arith, f16 = eng.split, eng.split.startswith("f16")
        has = (lambda key: key in packed.index) if packed is not None else (lambda key: False)
        # which launches are ON, block by block
        ons, compact = [], []
        for i, (f, s, res) in enumerate(eng.blocks):
            pre = "l%d." % i
            on = {k: k in kinds and has(pre + key) for k, (key, _) in _GEMMS.items()}
            on.update({k: k in kinds and all(has(pre + key) for key in keys) for k, (keys, _, _) in _WGRADS.items()})
            on["rwgrad"] = on["rwgrad"] and ops.TAP1_SPLIT
            # the dense 1x1 data gradient exists only inside the compact skip gradient
            compact.append(eng._compact_skip(s, on["rdgrad"]))
            on["rdgrad"] = on["rdgrad"] and compact[i]
            ons.append(on)
        # the cells that exist: one per operand with a consumer that is ON
        live = [[c for c, consumers in _CONSUMERS.items() if f16 and any(on[k] for k in consumers)] for on in ons]
        self.cells = torch.zeros(sum(len(names) for names in live), dtype=torch.int32, device=eng.device) if f16 else None
        self.blocks, n = [], 0
        for i, (on, names) in enumerate(zip(ons, live)):
            pre, rec = "l%d." % i, BlockPlan(compact[i])
            rec.bn1 = (eng.p[pre + "bn1.gamma"], eng.p[pre + "bn1.beta"])
            for c in names:
                setattr(rec, c, self.cells[n:n + 1])
                n += 1
            for k, (key, src) in _GEMMS.items():
                if on[k]:
                    setattr(rec, k, dict(split=arith, packed=packed.image(pre + key), bounds=(getattr(rec, src), packed.bound(pre + key))))
            for k, (_, src, dout) in _WGRADS.items():
                if on[k]:
                    setattr(rec, k, dict(split=arith, bounds=(getattr(rec, src), getattr(rec, dout)) if f16 else None))
            rec.amax_X = i == 0 and rec.X is not None
            rec.join_aux = rec.gfwd is not None or rec.amax_X
            if i > 0:
                self.blocks[-1].y = rec.X
            self.blocks.append(rec)

    def begin_step(self, flat):
        """the term images of this step's parameters; every cell back to zero"""
        if self.packed is not None:
            self.packed.refresh(flat)
        if self.cells is not None:
            self.cells.zero_()

    def raise_bn_bound(self, i, count):
        """g's cell of block i (which exists) from bn1's gamma / beta and the sample count"""
        rec = self.blocks[i]
        ops.bn_bound(rec.bn1[0], rec.bn1[1], count, rec.g)

    def raise_bn_bounds(self, B, T):
        """every Samuelson cell of a step on a clip of B bodies x T frames"""
        for i, s in enumerate(self.strides):
            if self.blocks[i].g is not None:
                self.raise_bn_bound(i, B * T * self.V)
            T = -(-T // s)
