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
otherwise the record holds None and the producer's `amax_cell=None` raises nothing.  The bf16x6 arithmetic scales nothing: no cells.

ResNetPlan, below, is the same for Path B's classifier (sar_amd/resnet.py): one record per convolution; its docstring has that engine's
table, and the one rule it does NOT share with the plan above."""
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


# ---------------------------------------------------------------------------------------------------- Path B's classifier
_FP32 = dict(split=None)


def _views(cv):
    """the term images a convolution gets -- the one place that says so: "f" = the forward view (tap, c, m), "b" = the data-gradient
    view (c and m exchanged).  3x3 / stride 1: both; 3x3 / stride 2: the data gradient's (four parity classes, csrc/conv2d_split.hip)"""
    if cv.k == 3 and cv.stride == 1 and 8 <= cv.cin <= 512 and cv.cout % 8 == 0 and cv.cout <= 512:
        return ("f", "b")
    if cv.k == 3 and cv.stride == 2 and 8 <= cv.cin and cv.cin % 8 == 0 and 16 <= cv.cout <= 512:
        return ("b",)
    return ()


class ConvPlan:
    """One convolution's record; plain attributes, fixed at construction.  The default is a convolution on the fp32 kernels.
      fwd dgrad   keyword arguments of ops.conv2d_gemm: dict(split=None), or dict(split=, packed=, bounds=(f / b, w_bound))
      wgrad       keyword arguments of ops.conv2d_wgrad: dict(split=None), or dict(split=, bounds=(f, b))
      f b         the cell (one-element view) of the forward's / the data gradient's source operand, or None
      y           on a block's conv2: the f cell of the NEXT block's conv1, raised by this block's tail
      bound       index into ResNetPlan.bounds of the Samuelson bound that raises f, or None"""
    __slots__ = ("fwd", "dgrad", "wgrad", "f", "b", "y", "bound")

    def __init__(self):
        self.fwd = self.dgrad = self.wgrad = _FP32
        self.f = self.b = self.y = self.bound = None


CONV_OFF = ConvPlan()


class ResNetPlan:
    """What a ResNet18 engine (sar_amd/resnet.py) decides once, when it is constructed.  packed: the PackedSplitWeights (None:
    mfma="fp32"); cells: the int32 cell tensor; recs: one ConvPlan per convolution name; bounds: the Samuelson bounds of a step as
    (gamma, beta, cell, the convolution whose output the BatchNorm normalises -- its sample count), in the order they are raised.

    The kinds of SAR_SPLIT_KINDS_PATHB are fwd, dgrad, wgrad.  A launch ASKS for the split kernels when its kind is switched on and
    its term image exists (_views; a weight gradient: the "f" image); the wrapper still demotes it at a feature map the kernels are
    not built for (ops.conv2d_split_applicable: at a (2, 1, 64, 64) clip every launch of layers 3 and 4).

      cell      bounds                          raised by                                                read by
      conv1.f   the block input                 block 0: ops.bn_bound of the stem's bn1 (the stem tail   conv1 fwd, conv1 wgrad
                                                is max-pool(relu(bn1))); else the tail of the block
                                                below (bn_add_relu_fwd, that block's conv2 record: y)
      conv2.f   relu(bn1(conv1 output))         ops.bn_bound of the block's bn1, folded into conv2's     conv2 fwd, conv2 wgrad
                                                operand load (Samuelson: no pass over the data)
      conv2.b   gradient of conv2's output      the backward tail pass (bn_add_relu_bwd_apply)           conv2 dgrad, conv2 wgrad
      conv1.b   gradient of conv1's output      the BN1-backward apply pass (affine2)                    conv1 dgrad, conv1 wgrad

    (a stride-2 conv1 has no "f" image, hence no f cell: the tail below it raises nothing and its weight gradient stays fp32.)

    UNLIKE the ST-GCN plan above, a cell here exists whenever its image exists, whatever SAR_SPLIT_KINDS_PATHB and the arithmetic say,
    and its producer raises it even when no launch reads it -- under a kinds subset, under bf16x6, and where the wrapper demotes
    every reader.  That is what the engine has always launched, and it is why the f cell is raised whenever it exists: the forward
    launch AND the weight gradient read it (with SAR_SPLIT_KINDS_PATHB=dgrad,wgrad the weight gradient once read a bound that only a
    split forward launch used to raise).  The "no unread cell" rule would change the arguments of the producer launches."""

    def __init__(self, eng, kinds):
        self.convs, self.blocks = eng.convs, eng.blocks
        self.packed, self.cells, self.bounds = None, None, []
        self.recs = {name: ConvPlan() for name in eng.convs}
        if not eng.split:
            return
        self.packed = sp = ops.PackedSplitWeights(eng.split)
        for name, cv in eng.convs.items():
            src, cc = eng.offsets[name + ".weight"], cv.cin * cv.cout
            for v in _views(cv):
                if v == "f":
                    sp.add((name, v), src, cc, cv.cout, 1, 9, cv.cin, cv.cout)
                elif cv.stride == 1:      # mirrored taps (include/sar_hip.h sar_conv2d_gemm_split)
                    sp.add((name, v), src + 8 * cc, -cc, 1, cv.cout, 9, cv.cout, cv.cin)
                else:                     # the stride-2 data gradient addresses the forward taps of the (tap, m, c) view
                    sp.add((name, v), src, cc, 1, cv.cout, 9, cv.cout, cv.cin)
        sp.finalize(eng.device)
        self.cells = torch.zeros(max(1, len(sp.items)), dtype=torch.int32, device=eng.device)      # one per image, in its order
        for name, cv in eng.convs.items():
            rec = self.recs[name]
            for v in _views(cv):
                setattr(rec, v, self.cells[sp.item_of[(name, v)]:][:1])
            gemm = lambda v: dict(split=eng.split, packed=sp.image((name, v)), bounds=(getattr(rec, v), sp.bound((name, v))))
            if rec.f is not None and "fwd" in kinds:
                rec.fwd = gemm("f")
            if rec.b is not None and "dgrad" in kinds:
                rec.dgrad = gemm("b")
            if rec.f is not None and "wgrad" in kinds:
                rec.wgrad = dict(split=eng.split, bounds=(rec.f, rec.b))
        # the producers that are not a convolution's own backward passes: Samuelson bounds and block tails
        self._samuelson(eng, "bn1", eng.blocks[0][0] + "conv1", "conv1")
        for i, blk in enumerate(eng.blocks):
            self._samuelson(eng, blk[0] + "bn1", blk[0] + "conv2", blk[0] + "conv1")
            if i + 1 < len(eng.blocks):
                self.recs[blk[0] + "conv2"].y = self.recs[eng.blocks[i + 1][0] + "conv1"].f

    def _samuelson(self, eng, bn, consumer, producer):
        rec = self.recs[consumer]
        if rec.f is not None:
            rec.bound = len(self.bounds)
            self.bounds.append((eng.p[bn + ".weight"], eng.p[bn + ".bias"], rec.f, producer))

    def rec(self, name, training=True):
        """the record of convolution `name` in a training step; inference keeps the fp32 kernels and raises nothing"""
        return self.recs[name] if training else CONV_OFF

    begin_step = SplitPlan.begin_step      # (reads .packed and .cells only)

    def raise_bn_bound(self, i, count):
        """entry i of bounds (None: nothing) from its gamma / beta and the sample count"""
        if i is not None:
            gamma, beta, cell, _ = self.bounds[i]
            ops.bn_bound(gamma, beta, count, cell)

    def raise_bn_bounds(self, B, H, W):
        """every Samuelson cell of a step on B images of H x W, from the geometry alone: what forward() raises layer by layer when
        the bounds are not forked"""
        def osz(n, cv):
            return (n + 2 * cv.pad - cv.k) // cv.stride + 1
        cv = self.convs["conv1"]
        H, W = osz(H, cv), osz(W, cv)
        count = {"conv1": B * H * W}
        H, W = (H + 2 - 3) // 2 + 1, (W + 2 - 3) // 2 + 1      # the stem's max-pool
        for blk in self.blocks:
            cv = self.convs[blk[0] + "conv1"]
            H, W = osz(H, cv), osz(W, cv)
            count[cv.name] = B * H * W
        for i, (_, _, _, producer) in enumerate(self.bounds):
            self.raise_bn_bound(i, count[producer])
