"""ST-GCN training engine on the HIP kernels (one process = one MI355X).

Mirrors the reference model (models/stgcn.py:101-160, blocks :11-64, GraphConvTD models/gcn.py:187-209)
and its train step (main_gnn.py:219-239): forward, hand-scheduled backward, gradients into ONE flat
fp32 buffer (so data parallelism is a single RCCL all-reduce, main_gnn.py:257 MirroredStrategy), fused
Nesterov SGD (main_gnn.py:312-314).  Parameters keep the reference's Keras layouts and names.

HBM layout: activations are [C][B*T*V] matrices (CN layout, include/sar_hip.h); per block the tensors
that cross a BatchNorm barrier (g = graph conv out, u = temporal conv out, r = residual conv out,
y = block out) are materialised once in forward and kept for backward; BN+ReLU is folded into the
consumer's operand load, BN statistics into the producer's epilogue.
"""
import math
import os

import numpy as np
import torch

from . import _lib as L
from . import ops
from .engine import FlatEngine
from .split_plan import OFF, BlockPlan, SplitPlan

BN_EPS = 1e-3        # Keras BatchNormalization defaults (models/stgcn.py:27,37,56,111)
BN_MOMENTUM = 0.99
KS, KT = 3, 9        # kernel_size=[3, 9], models/stgcn.py:14
# A block's weight gradients are ISSUED behind its data gradients in the fp32 engines (side stream as before): they then run
# beside the NEXT block's element-wise BatchNorm passes instead of beside this block's data-gradient GEMMs.  Three interleaved
# rounds: fp32 59.22 -> 58.99 ms per step; bf16 13.26 -> 13.55 (slower: there the order stays as it was).  SAR_WGRAD_DEFER=0/1 forces it.
_WGRAD_DEFER_ENV = os.environ.get("SAR_WGRAD_DEFER")
# SAR_EPI_ADD_GATE in the fp32 graph data gradient
_FUSE_TAIL_F32 = os.environ.get("SAR_F32_FUSE_TAIL", "1") == "1"
# the arithmetic an STGCN built without an explicit `mfma` uses (the parity suites run once per value: tests/conftest.py)
DEFAULT_MFMA = os.environ.get("SAR_MFMA", "fp32")
# engine mode -> arithmetic of csrc/conv_gemm_split.hip
SPLIT_ARITH = {"f32_split": "f16x3a", "f32_split_bf16x6": "bf16x6"}
# SAR_STGCN_AUX_STREAM=0: the split engine's term images, the zeroing of its bound cells and its Samuelson cells on the main stream again
# instead of on a third stream beside the data_bn stage and the first layer (round 6, as sar_amd/resnet.py; bit-identical).  One bench.py
# process per entry (profiles/r06_stgcn_aux_stream_ab.txt): f32_split 1 929 -> 1 936 clips/s (+0.3 %); the bf16 engine's single pack launch
# forked the same way: 5 497 -> 5 466 (-0.5 %), not forked
AUX_STREAM = os.environ.get("SAR_STGCN_AUX_STREAM", "1") == "1"
# the skip gradient of a conv-residual block as its even frames only: "fp32" (default) = the fp32-arithmetic engine, where it measured
# +0.4 % (58.70 -> 58.47 ms, interleaved); "1" = the split engines too (single stream -0.29 ms, two streams 34.34 -> 34.44 ms: not taken);
# "0" = never (gpurun_out/compact_skip_ab*.txt)
_COMPACT_SKIP = os.environ.get("SAR_COMPACT_SKIP", "fp32")
# A/B switch: which kernel families of a split engine take the split kernels (default all that are built)
_SPLIT_KINDS = set(os.environ.get("SAR_SPLIT_KINDS", "tfwd,tdgrad,twgrad,gfwd,gdgrad,gwgrad,rfwd,rdgrad,rwgrad").split(","))
_NO_SPLIT = dict(split=None)      # the arithmetic keyword arguments of a weight gradient that stays on the fp32 / bf16-operand kernel
# (filters, stride, residual) -- models/stgcn.py:113-123
BLOCKS = [(64, 1, False), (64, 1, True), (64, 1, True), (64, 1, True), (128, 2, True), (128, 1, True), (128, 1, True),
          (256, 2, True), (256, 1, True), (256, 1, True)]


def same_pad(T, k, s):
    """TF 'SAME': (out, pad_begin, pad_end); the extra pad goes at the end."""
    out = -(-T // s)
    total = max((out - 1) * s + k - T, 0)
    return out, total // 2, total - total // 2


def ntu_adjacency():
    """graph/ntu_rgb_d.py:6-40 + graph/tools.py:4-30 ('spatial' labelling) -> (3,25,25) float64."""
    from graph.ntu_rgb_d import Graph  # the package's drop-in mirror of the reference module
    return Graph().A


class _BN:
    """Per-BatchNorm device state: parameters are views of the flat buffer, statistics are buffers."""

    def __init__(self, C, device, pivoted=False):
        z = lambda: torch.zeros(C, dtype=torch.float32, device=device)
        self.pivot = z() if pivoted else None       # data_bn: the value its two-pass statistics subtract (ops.data_bn_stats)
        self.moving_mean, self.moving_var = z(), torch.ones(C, dtype=torch.float32, device=device)
        self.mean, self.rstd, self.scale, self.shift = z(), z(), z(), z()
        self.k1, self.k2, self.k3 = z(), z(), z()


class STGCN(FlatEngine):
    # What a sibling engine (sar_amd/stgin.py, stpgcn.py, stgcn_ta.py) declares about itself; __init__ and the gates below read these:
    env_arithmetic = True      # built without `mfma`: DEFAULT_MFMA (the siblings are fp32)
    batched_slabs = True       # one slab reduction per gradient bucket (ops.SlabBatch) instead of one per weight gradient
    third_stream = True        # the aux stream of forward() (AUX_STREAM)
    batched_wT = True          # one re-layout launch for every data-gradient operand (_wT) instead of one transpose per layer
    stock_backward = True      # blocks run STGCN._block_backward: the fused fp32 tail and the compact skip gradient apply

    def __init__(self, num_classes=60, in_channels=3, num_node=25, A=None, device="cuda", seed=0, bone_pairs=None,
                 blocks=None, motion=False, mfma=None, trainable_adjacency=False):
        L.load()  # fail loudly if the HIP library is missing
        # mfma="fp32" (default) is the reference's arithmetic.
        # mfma="bf16" is SURVEY.md 8d config 3: activations and activation gradients are stored in HBM as bfloat16 (CN8
        # layout, csrc/cn8.h), every convolution / data gradient / weight gradient multiplies bf16 operands with fp32
        # accumulation (sar_conv_gemm_cn8, sar_conv_wgrad_cn8); BatchNorm statistics, master weights, gradients and the
        # optimizer stay fp32 (sar_amd/stgcn8.py holds the step).
        # mfma="bf16_operands" is the round-1 intermediate kept for A/B runs: bf16 MFMA operands, fp32 activations in HBM.
        # mfma="f32_split": fp32 RESULTS on the fp16 matrix pipe -- storage, BatchNorm statistics, epilogues and parameters are the
        # fp32 engine's, the contraction of the GEMM-shaped kernels multiplies two fp16 terms per operand (three products, fp32
        # accumulation: csrc/conv_gemm_split.hip; same parity tolerances as "fp32").  "f32_split_bf16x6": three bfloat16 terms,
        # six products (no operand scaling).  Kernels without a split form, and inference, stay on the fp32 kernels.
        if mfma is None:
            mfma = DEFAULT_MFMA if (self.env_arithmetic and not trainable_adjacency) else "fp32"
        assert mfma in ("fp32", "bf16", "bf16_operands", "f32_split", "f32_split_bf16x6")
        self.mfma = mfma
        self.cn8 = mfma == "bf16"
        self.bf16 = mfma == "bf16_operands"
        self.split = SPLIT_ARITH.get(mfma)
        # trainable_adjacency: the stacked adjacency becomes the trainable variable `adjacency_matrix`
        # (models/gcn.py:212-238 AdjGraphConv) shared by all blocks; the graph convolution then keeps the reference's
        # order -- 1x1 convolution to 3F channels, dense contraction with A (csrc/graph_dense.hip) -- and the backward pass
        # produces dA.  `train_adjacency` gates its gradient per step (main_gnn.py:228-232: trained only while
        # epoch > --freeze-graph-until).  fp32 only.
        self.dense_A = bool(trainable_adjacency)
        self.train_adjacency = True
        assert not (self.dense_A and mfma != "fp32"), "trainable adjacency is built for the fp32 engine"
        self.num_classes, self.C_in, self.V = num_classes, in_channels, num_node
        self.blocks = list(blocks if blocks is not None else BLOCKS)
        # every engine of the family runs these steps, in this order; a sibling overrides the step that differs
        self._init_device(device, bone_pairs, motion)
        self._init_adjacency(A)
        self._declare_params()
        total = self._allocate()
        self._init_bn()
        self._init_operand_images()
        self._init_params(seed)
        self._saved = None
        self._deferred, self._flushing = [], False
        self._buckets = self._make_buckets(total)

    # ------------------------------------------------------------------ the constructor's steps
    def _init_device(self, device, bone_pairs, motion):
        self.device = dev = torch.device(device)
        # the weight-gradient stream (SAR_WGRAD_STREAM=0: none); SAR_WGRAD_PRIO: its priority (default 0 = same as the main chain)
        prio = int(os.environ.get("SAR_WGRAD_PRIO", "0")) if os.environ.get("SAR_WGRAD_STREAM", "1") == "1" else None
        self._init_streams(prio, ops.SLAB_BATCH and self.batched_slabs, AUX_STREAM and self.third_stream)
        self._aux_pending = False
        self.motion = bool(motion)   # motion stream (data_gen/gen_motion_data.py:24-27) of the joint / bone data, on the fly
        self.bone_parent = None
        if bone_pairs is not None:
            bp = np.full(self.V, -1, dtype=np.int32)
            for v1, v2 in bone_pairs:          # data_gen/gen_bone_data.py:36-41 (1-based pairs)
                assert 1 <= v1 <= self.V and 1 <= v2 <= self.V, "bone pair (%d, %d) outside 1..%d" % (v1, v2, self.V)
                bp[v1 - 1] = v2 - 1
            self.bone_parent = torch.from_numpy(bp).to(dev)

    def _init_adjacency(self, A):
        A = np.asarray(ntu_adjacency() if A is None else A, dtype=np.float64)
        assert A.shape == (KS, self.V, self.V)
        self.A_host = A.astype(np.float32)
        self.A = torch.from_numpy(self.A_host).to(self.device)     # 'adjacency_matrix', non-trainable (stgcn.py:105-109)
        self.tab_fwd = ops.GraphTables(self.A_host, self.device, transpose=False)
        self.tab_bwd = ops.GraphTables(self.A_host, self.device, transpose=True)

    def _declare_params(self):
        """the parameter table (Keras layouts and names), in the order of the flat buffer"""
        self.shapes, self.kinds = {}, []
        nch = self.V * self.C_in
        self._add("data_bn.gamma", (nch,)), self._add("data_bn.beta", (nch,))
        cin = self.C_in
        for i, (f, s, res) in enumerate(self.blocks):
            kind = "none" if not res else ("identity" if (cin == f and s == 1) else "conv")   # stgcn.py:41-56
            self.kinds.append(kind)
            self._declare_block("l%d." % i, cin, f, kind)
            self._params_after_block(i)
            cin = f
        self.C_last = cin
        self._add("logits.kernel", (1, 1, cin, self.num_classes)), self._add("logits.bias", (self.num_classes,))
        if self.dense_A and self._shared_adjacency():
            self._add("adjacency_matrix", (KS, self.V, self.V))

    def _declare_block(self, pre, cin, f, kind):
        self._add(pre + "gcn.kernel", (1, 1, cin, KS * f)), self._add(pre + "gcn.bias", (KS * f,))
        self._declare_temporal(pre, f, cin, f, kind)

    def _declare_temporal(self, pre, c, cin, f, kind):
        """what follows a block's spatial operator (c channels): bn1, the temporal convolution c -> f, bn2, the residual branch"""
        self._add(pre + "bn1.gamma", (c,)), self._add(pre + "bn1.beta", (c,))
        self._add(pre + "tcn.kernel", (KT, 1, c, f)), self._add(pre + "tcn.bias", (f,))
        self._add(pre + "bn2.gamma", (f,)), self._add(pre + "bn2.beta", (f,))
        if kind == "conv":
            self._add(pre + "res.kernel", (1, 1, cin, f)), self._add(pre + "res.bias", (f,))
            self._add(pre + "res_bn.gamma", (f,)), self._add(pre + "res_bn.beta", (f,))

    def _allocate(self):
        total = self._allocate_flat(("velocity",))
        if "adjacency_matrix" in self.p:
            self.A = self.p["adjacency_matrix"]          # the trainable copy (initialised from the graph in _init_params)
        return total

    def _init_bn(self):
        self.bn = {"data_bn": _BN(self.V * self.C_in, self.device, pivoted=True)}
        for i, (f, s, res) in enumerate(self.blocks):
            self._init_block_bn("l%d." % i, f, self.kinds[i])

    def _init_block_bn(self, pre, f, kind, c=None):
        """c: channels of the spatial operator's output where they are not f"""
        self.bn[pre + "bn1"], self.bn[pre + "bn2"] = _BN(c or f, self.device), _BN(f, self.device)
        if kind == "conv":
            self.bn[pre + "res_bn"] = _BN(f, self.device)

    def _weight_images(self):
        """Every convolution weight as a GEMM operand in both orientations -- .f the forward launch, .b the data gradient (the same
        tensor with the roles of c and m exchanged) -- block by block: (key, block index, (src_off, st, sc, sm, taps, Kc, M)) with
        element (tap, c, m) at flat[src_off + tap * st + c * sc + m * sm]"""
        cin = self.C_in
        for i, (f, s, res) in enumerate(self.blocks):
            pre = "l%d." % i
            ot, og = self.offsets[pre + "tcn.kernel"], self.offsets[pre + "gcn.kernel"]
            yield pre + "tcn.f", i, (ot, f * f, f, 1, KT, f, f)              # (tap, c, m) = kernel[tap][c][m]
            yield pre + "tcn.b", i, (ot, f * f, 1, f, KT, f, f)              # (tap, c', m') = kernel[tap][m'][c']
            yield pre + "gcn.f", i, (og, f, KS * f, 1, KS, cin, f)           # (k, c, m) = kernel[c][k*F + m]
            yield pre + "gcn.b", i, (og, f, 1, KS * f, KS, f, cin)           # (k, c', m') = kernel[m'][k*F + c']
            if self.kinds[i] == "conv":
                orr = self.offsets[pre + "res.kernel"]
                yield pre + "res.f", i, (orr, 0, f, 1, 1, cin, f)            # (0, c, m) = kernel[c][m]
                yield pre + "res.b", i, (orr, 0, 1, f, 1, f, cin)            # (0, c', m') = kernel[m'][c']
            cin = f

    def _pack(self, pk, admit):
        """the images of _weight_images() that admit(key, stride of the block, taps, Kc, M) takes, refreshed by one launch per step"""
        for key, i, w in self._weight_images():
            if admit(key, self.blocks[i][1], *w[4:]):
                pk.add(key, *w)
        if not pk.items:
            return None
        pk.finalize(self.device)
        return pk

    def _split_admits(self, key, s, taps, Kc, M):
        """the shapes csrc/conv_gemm_split.hip is built for; the 1x1 residual convolution (conv_tap1_split_kernel, round 6): its strided
        forward form and the dense product of the compact skip gradient of a stride-2 block"""
        layer, way = key.split(".")[1:]
        if layer == "gcn":
            return ops.split_applicable(L.SAR_CONV_GRAPH, self.V, Kc, M, taps, 1, self.tab_fwd if way == "f" else self.tab_bwd)
        if layer == "tcn":
            return ops.split_applicable(L.SAR_CONV_TEMPORAL, self.V, Kc, M, taps, s)
        return (self.split in ("f16x3a", "bf16x6") and (way == "f" or s == 2)
                and ops.split_applicable(L.SAR_CONV_TEMPORAL, self.V, Kc, M, 1, s if way == "f" else 1))

    def _init_operand_images(self):
        """what the arithmetic needs beside the fp32 parameters: bf16 operand images (cn8: of EVERY conv weight), the split engines'
        term images and operand-bound cells, the fp32 engines' transposed data-gradient operands"""
        dev = self.device
        self.packed = self.plan = self.spacked = self._cells = None
        if self.cn8:
            self.packed = self._pack(ops.PackedWeights(), lambda key, s, taps, Kc, M: True)
        if self.bf16:
            self.packed = self._pack(ops.PackedWeights(), lambda key, s, taps, Kc, M: M % 8 == 0 and Kc >= 16)
        if self.split:
            # every per-launch decision of the split arithmetic, made here once (SAR_SPLIT_KINDS is read now, not per launch)
            self.plan = SplitPlan(self, self._pack(ops.PackedSplitWeights(self.split), self._split_admits), _SPLIT_KINDS)
            self.spacked, self._cells = self.plan.packed, self.plan.cells
        # what block i's launches read (no plan: nothing on the split kernels)
        self._recs = self.plan.blocks if self.plan else [BlockPlan(self._compact_skip(s)) for _, s, _ in self.blocks]
        # fp32 operands of the data-gradient GEMMs ((tap, f, c) / (k, f, c) / (f, c) transposes of the kernels): ONE
        # re-layout launch at the start of backward() instead of one small dependent launch in front of every data gradient
        # (22 per step, each on the critical chain)
        self._wT_off, self._wT_perm, self._wT = {}, None, None
        if self.batched_wT and not self.cn8:
            pb, off = ops.PermuteBatch(), 0
            for key, i, (src, st, sc, sm, taps, Kc, M) in self._weight_images():
                if key.endswith(".b"):
                    pb.add(src, off, taps, Kc, M, st, sc, sm)          # [tap][Kc][M], contiguous
                    self._wT_off[key[:-2]], off = off, off + taps * Kc * M
            pb.finalize(dev)
            self._wT_perm, self._wT = pb, torch.zeros(off, dtype=torch.float32, device=dev)

    # ------------------------------------------------------------------ gradient buckets (data-parallel exchange)
    def _make_buckets(self, total):
        """Contiguous slices of the flat gradient buffer in the order backward() completes them (main_gnn.py:234,239: the
        all-reduce inside apply_gradients).  Parameters are laid out data_bn, l0 .. l9, logits(, adjacency_matrix); backward
        produces logits, l9 .. l0, data_bn(, adjacency): bucket 0 = [first block of the last stage .. logits], one bucket per
        earlier stage boundary (a stride-2 block), the last bucket = [data_bn .. end of the first stage]; a trainable
        adjacency is summed over the blocks at the very end and forms its own slice.  Each entry: (block index after whose
        backward the slice is complete, or -1 = at the end of backward; lo; hi)."""
        nb = len(self.blocks)
        starts = [i for i, (f, s, res) in enumerate(self.blocks) if s != 1 and i > 0]     # a new stage begins here
        hi = self.offsets.get("adjacency_matrix", total)
        out = []
        for i in reversed(starts):
            lo = min(o for k, o in self.offsets.items() if k.startswith("l%d." % i))
            if lo < hi:
                out.append((i, lo, hi))
                hi = lo
        out.append((-1, 0, hi))
        if "adjacency_matrix" in self.offsets:
            out.append((-1, self.offsets["adjacency_matrix"], total))
        assert sum(h - l for _, l, h in out) == total and nb > 0
        return out

    def _finish_backward(self, cb):
        """nothing deferred is left behind"""
        if self._deferred:
            self._flush_deferred()
        super()._finish_backward(cb)

    # ------------------------------------------------------------------ a layer between two blocks (sar_amd/stpgcn.py)
    # Hook points of a sibling model that inserts a layer after block i: its parameters follow block i's in the flat buffer, its
    # forward runs on block i's output, its backward on the gradient that block i + 1 hands down.  No-ops here.
    def _params_after_block(self, i):
        pass

    def _layer_after(self, i):
        """does a layer sit between block i and block i + 1?"""
        return False

    def _after_block_forward(self, i, h, B, T, training, saved, keep):
        return h

    def _after_block_backward(self, i, dY, B):
        return dY

    # ------------------------------------------------------------------ the dense contraction of a block (sar_amd/stgcn_ta.py)
    # Hook points of a sibling model whose blocks contract with tables of their own: which table block i uses and which three ops
    # (csrc/graph_dense.hip here: ONE (K, V, V) adjacency shared by the blocks, its gradient summed over them at the end of backward).
    def _shared_adjacency(self):
        """is the trainable adjacency the single parameter `adjacency_matrix` shared by all blocks?"""
        return True

    def _dense_fwd(self, i, y3, g, f, B, T, training):
        return ops.graph_dense_fwd(y3, self.A, g, KS, f, self.V, B * T, stats=training)

    def _dense_bwd_data(self, i, dg, dy3, f, B, T):
        ops.graph_dense_bwd_data(dg, self.A, dy3, KS, f, self.V, B * T)

    def _dense_dA(self, i, y3, dg, f, B, T):
        """one V x V x K block per layer; summed over the layers by _dense_backward_end"""
        ops.graph_dense_dA(y3, dg, self._dA_layers[i], KS, f, self.V, B * T)

    def _dense_backward_begin(self, dev):
        self._dA_layers = torch.zeros((len(self.blocks), KS * self.V * self.V), dtype=torch.float32, device=dev)

    def _dense_backward_end(self):
        """the adjacency is shared by all blocks: dA = sum over the layers (fixed order); zero while frozen"""
        n = KS * self.V * self.V
        ops.check(L.load().sar_slab_reduce_f32(ops.ptr(self._dA_layers), len(self.blocks), n, n,
                                               ops.ptr(self.g["adjacency_matrix"]), ops.stream_ptr()), "sar_slab_reduce_f32")
        self._dA_layers = None

    # ------------------------------------------------------------------ parameters
    def _add(self, name, shape):
        self.shapes[name] = tuple(shape)

    def _init_params(self, seed):
        """models/stgcn.py:7-8 VarianceScaling(2, fan_out, truncated_normal); biases 0; BN gamma 1, beta 0."""
        gen = torch.Generator().manual_seed(seed)
        for k, shp in self.shapes.items():
            if k == "adjacency_matrix":
                self.p[k].copy_(torch.from_numpy(self.A_host))
            elif k.endswith(".kernel"):
                fan_out = int(np.prod(shp[:-2])) * shp[-1]      # (kh, kw, in, out) and Conv1D (k, in, out)
                std = math.sqrt(2.0 / fan_out) / .87962566103423978
                w = torch.empty(shp, dtype=torch.float64)
                torch.nn.init.trunc_normal_(w, 0.0, std, -2 * std, 2 * std, generator=gen)
                self.p[k].copy_(w.to(torch.float32))
            elif k.endswith(".gamma"):
                self.p[k].fill_(1.0)
            else:
                self.p[k].zero_()

    def load_params(self, params):
        """params: dict name -> tensor in the oracle / Keras layouts (incl. optional moving stats, 'A' ignored)."""
        self._lr_host = None      # (a restored engine re-writes the device-side learning rate at its next step)
        super().load_params(params)

    def state_dict(self):
        out = super().state_dict()
        out["A"] = self.A.cpu().clone()
        return out

    def grads(self):
        return {k: v for k, v in self.g.items()}

    # ------------------------------------------------------------------ forward
    def _bn_forward(self, name, result, count, training, unbiased=True):
        """BatchNorm `name` ready for its consumer's operand load (scale, shift): training, from the statistics its producer's epilogue
        left in result = (partials, nparts, ..) over `count` samples, the moving statistics updated; inference, from the moving
        statistics.  Returns the _BN."""
        b = self.bn[name]
        if training:
            ops.bn_finalize(result[0], result[1], b.mean.numel(), count, BN_EPS, BN_MOMENTUM, unbiased, self.p[name + ".gamma"],
                            self.p[name + ".beta"], b.moving_mean, b.moving_var, b.mean, b.rstd, b.scale, b.shift, pivot=b.pivot)
        else:
            self._bn_eval(name)
        return b

    def _bn_eval(self, name):
        b = self.bn[name]
        ops.bn_eval_affine(self.p[name + ".gamma"], self.p[name + ".beta"], b.moving_mean, b.moving_var, BN_EPS, b.scale,
                           b.shift)

    def forward(self, x, training=True, keep=None):
        """x: (N, C, T, V, M) float32 cuda -> logits (N, classes).  keep: optional dict receiving
        intermediate activations (tests)."""
        if self.cn8:
            from . import stgcn8
            return stgcn8.forward(self, x, training, keep)
        assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 5
        x = x.contiguous()
        N, Cin, T, V, M = x.shape
        assert Cin == self.C_in and V == self.V
        dev, B = x.device, N * M
        saved = {"x": x, "N": N, "M": M, "T": T, "blocks": [], "training": training}
        if self.packed is not None:
            self.packed.refresh(self.flat)       # the parameters may have changed since the last step
        self._bounds_forked = False
        if self.spacked is not None and training:
            if self._aux is not None:
                # term images, bound cells and the Samuelson cells (functions of gamma / beta and the sample counts) beside the data_bn
                # stage and the 3-channel layer: joined in front of the first launch that reads an image or a cell (_join_aux)
                def images():
                    self.plan.begin_step(self.flat)
                    self.plan.raise_bn_bounds(B, T)
                self._fork(images)      # behind the optimizer step that produced self.flat
                self._aux_pending = self._bounds_forked = True
            else:
                self.plan.begin_step(self.flat)
        # ---- data_bn (models/stgcn.py:142-147)
        part = None
        if training:
            part = torch.empty((V * Cin, N, 2), dtype=torch.float32, device=dev)
            ops.data_bn_stats(x, self.bone_parent, part, self.motion, pivot=self.bn["data_bn"].pivot)
        dbn = self._bn_forward("data_bn", (part, N), N * M * T, training, unbiased=False)
        h = torch.empty((Cin, B * T * V), dtype=torch.float32, device=dev)
        ops.data_bn_apply(x, self.bone_parent, dbn.scale, dbn.shift, h, self.motion)
        if keep is not None:
            keep["x0"] = h
        Tc, cin = T, Cin
        for i, (f, s, res) in enumerate(self.blocks):
            h, Tc = self._block_forward(i, h, cin, f, s, B, Tc, training, saved, keep)
            h = self._after_block_forward(i, h, B, Tc, training, saved, keep)
            cin = f
        # ---- head (models/stgcn.py:153-158)
        feat = torch.empty((N, cin), dtype=torch.float32, device=dev)
        ops.pool_fwd(h, B, Tc * V, M, feat)
        logits = torch.empty((N, self.num_classes), dtype=torch.float32, device=dev)
        ops.fc_fwd(feat, self.p["logits.kernel"].view(cin, self.num_classes), self.p["logits.bias"], logits)
        saved.update(feat=feat, T_last=Tc, y_last_shape=(cin, B * Tc * V))
        self._saved = saved if training else None
        if keep is not None:
            keep["feat"] = feat
        return logits

    def _block_forward(self, i, X, cin, f, s, B, T, training, saved, keep):
        V, dev = self.V, X.device
        pre = "l%d." % i
        kind = self.kinds[i]
        To, pad, _ = same_pad(T, KT, s)
        n_in, n_out = B * T * V, B * To * V
        epi = L.SAR_EPI_STATS if training else L.SAR_EPI_NONE
        rec = self._recs[i] if training else OFF      # inference keeps the fp32 kernels (no batch statistics to bound with)
        # sgcn: GraphConvTD (models/gcn.py:199-209)
        g = torch.empty((f, n_in), dtype=torch.float32, device=dev)
        y3 = None
        if self.dense_A:   # models/gcn.py:229-237: Conv2D(3F, 1x1) then einsum 'nkctv,kvw->nctw' with the trainable A
            y3 = torch.empty((KS * f, n_in), dtype=torch.float32, device=dev)
            ops.conv_gemm(L.SAR_CONV_TEMPORAL, X, y3, self.p[pre + "gcn.kernel"], 0, KS * f, B=B, V=V, T_src=T, T_out=T, Kc=cin,
                          M=KS * f, taps=1, stride=1, pad=0, bias=self.p[pre + "gcn.bias"])
            r1 = self._dense_fwd(i, y3, g, f, B, T, training)
        else:
            if rec.join_aux:
                self._join_aux()                    # first reader of a term image / first writer of a cell on the main chain
            if rec.amax_X:
                ops.amax(X, rec.X)                  # the bound of the block input (blocks > 0: written by the previous block's tail)
            r1 = ops.conv_gemm(L.SAR_CONV_GRAPH, X, g, self.p[pre + "gcn.kernel"], f, KS * f, B=B, V=V, T_src=T, T_out=T,
                               Kc=cin, M=f, taps=KS, bias=self.p[pre + "gcn.bias"], tables=self.tab_fwd, epi=epi,
                               **self._arith(rec.gfwd, self._img(pre + "gcn.f")))
        bn1 = self._bn_forward(pre + "bn1", r1, n_in, training)
        # tgcn: BN -> ReLU folded into the operand load, Conv2D [9,1] stride s SAME (models/stgcn.py:26-36)
        u = torch.empty((f, n_out), dtype=torch.float32, device=dev)
        self._join_aux()           # (the 3-channel layer's graph convolution above reads neither images nor cells: the fork ends here)
        if rec.g is not None and not self._bounds_forked:
            self.plan.raise_bn_bound(i, n_in)
        r2 = ops.conv_gemm(L.SAR_CONV_TEMPORAL, g, u, self.p[pre + "tcn.kernel"], f * f, f, B=B, V=V, T_src=T, T_out=To,
                           Kc=f, M=f, taps=KT, stride=s, pad=pad, bias=self.p[pre + "tcn.bias"],
                           pro=(bn1.scale, bn1.shift), pro_relu=True, epi=epi, **self._arith(rec.tfwd, self._img(pre + "tcn.f")))
        bn2 = self._bn_forward(pre + "bn2", r2, n_out, training)
        r = None
        rbn = None
        if kind == "conv":  # models/stgcn.py:47-56
            r = torch.empty((f, n_out), dtype=torch.float32, device=dev)
            r3 = ops.conv_gemm(L.SAR_CONV_TEMPORAL, X, r, self.p[pre + "res.kernel"], 0, f, B=B, V=V, T_src=T, T_out=To,
                               Kc=cin, M=f, taps=1, stride=s, pad=0, bias=self.p[pre + "res.bias"], epi=epi,
                               **self._arith(rec.rfwd, self._img(pre + "res.f")))
            rbn = self._bn_forward(pre + "res_bn", r3, n_out, training)
        y = torch.empty((f, n_out), dtype=torch.float32, device=dev)
        res_kind = {"none": 0, "identity": 1, "conv": 2}[kind]
        ymask = ops.relu_mask(y) if training else None     # 1 bit per element: what the BatchNorm-backward passes read instead of y
        # (split arithmetic: y is the next block's operand; its bound, rec.y, is a by-product of this pass)
        ops.bn_add_relu_fwd(u, bn2.scale, bn2.shift, res_kind, X if kind == "identity" else r,
                            rbn.scale if rbn else None, rbn.shift if rbn else None, y, mask=ymask, amax_cell=rec.y)
        if training:
            saved["blocks"].append(dict(X=X, g=g, u=u, r=r, y=y, ymask=ymask, T=T, To=To, pad=pad, cin=cin, f=f, s=s, kind=kind, y3=y3))
        if keep is not None:
            keep[pre + "g"], keep[pre + "u"], keep[pre + "y"] = g, u, y
        return y, To

    # ------------------------------------------------------------------ one block on its own (models/stgcn.py SpatioTemporalGraphConv)
    # The layer-level class runs block i of a (one-block) engine on a CN tensor of its own: the block's forward and backward ARE
    # _block_forward / _block_backward, with what forward() / backward() do around them for that block.
    def block_forward(self, i, X, B, T, training):
        """X [cin][B T V] -> (y [f][B To V], To, what block_backward needs or None)"""
        f, s, _ = self.blocks[i]
        saved = {"blocks": []}
        y, To = self._block_forward(i, X, X.shape[0], f, s, B, T, training, saved, None)
        return y, To, (saved["blocks"][0] if training else None)

    def block_backward(self, i, sb, dY, B):
        """dY [f][B To V] (overwritten) -> dX [cin][B T V]; the block's gradients (and a trainable adjacency's) are in self.g"""
        if self._wT_perm is not None:
            self._wT_perm.run(self.flat, self._wT)
        if self.dense_A:
            self._dense_backward_begin(dY.device)
        dX, _ = self._block_backward(i, sb, dY, B, None, None)
        if self.dense_A:
            if self.train_adjacency:
                self._dense_backward_end()
            else:
                self._dA_layers = None
        self._finish_backward(None)
        return dX

    def _join_aux(self):
        """the main chain waits for what forward() forked onto the third stream (once per step)"""
        if self._aux_pending:
            self._join()
            self._aux_pending = False

    def _img(self, key):
        """packed bf16 operand image of a conv weight (bf16 mode), else None"""
        return self.packed.image(key) if self.packed is not None and key in self.packed.index else None

    def _arith(self, split_args, packed=None):
        """the arithmetic keyword arguments of ops.conv_gemm: those of the block's record (sar_amd/split_plan.py) for a launch on the
        split kernels, else the fp32 / bf16-operand kernel with its `packed` image"""
        return split_args or dict(split=None, bf16=self.bf16, packed=packed)

    # ------------------------------------------------------------------ backward
    def _off_critical_path(self, fn, *tensors):
        """fn() on the weight-gradient stream (_on_side), at once or -- see _WGRAD_DEFER_ENV above -- when the block's data
        gradients have been issued (_flush_deferred)"""
        if self._side is not None and self._wgrad_defer() and not self._flushing:
            self._deferred.append((fn, tensors))
        else:
            self._on_side(fn, *tensors)

    def _wgrad_defer(self):
        return (not self.cn8) if _WGRAD_DEFER_ENV is None else _WGRAD_DEFER_ENV == "1"

    def _flush_deferred(self):
        q, self._deferred = self._deferred, []
        self._flushing = True
        try:
            for fn, tensors in q:
                self._off_critical_path(fn, *tensors)
        finally:
            self._flushing = False

    def backward(self, dlogits, bucket_cb=None, need_dx=False):
        """dlogits (N, classes) -> fills self.grad (every trainable parameter).  main_gnn.py:233.  bucket_cb: see
        _bucket_done (the data-parallel exchange starts per bucket while backward is still running).  need_dx additionally returns
        d loss / d x, float32 (N, C, T, V, M): the backward apply pass of data_bn, one more launch behind the last bucket (a
        per-rank quantity, never exchanged); without it the launches are those of a step that asks for no input gradient."""
        if self.cn8:
            from . import stgcn8
            return stgcn8.backward(self, dlogits, bucket_cb, need_dx)
        sv = self._saved
        assert sv is not None, "backward() needs a preceding forward(training=True)"
        dev, V = dlogits.device, self.V
        if self._wT_perm is not None:
            self._wT_perm.run(self.flat, self._wT)      # every data-gradient operand of this step
        N, M = sv["N"], sv["M"]
        B = N * M
        c_last = self.C_last
        feat = sv["feat"]
        dfeat = torch.empty_like(feat)
        ops.fc_bwd(feat, self.p["logits.kernel"].view(c_last, self.num_classes), dlogits.contiguous(),
                   self.g["logits.kernel"].view(c_last, self.num_classes), self.g["logits.bias"], dfeat)
        dY = torch.empty(sv["y_last_shape"], dtype=torch.float32, device=dev)
        ops.pool_bwd(dfeat, B, sv["T_last"] * V, M, dY)
        if self.dense_A:
            self._dense_backward_begin(dev)
        # fp32 engine, gather tables: the graph data gradient of block i gates the output gradient of block i - 1 with that block's
        # ReLU mask and reduces its BatchNorm-backward sums in the same epilogue (SAR_EPI_ADD_GATE; sar_amd/stgcn8.py does the same
        # for the bf16 engine) -- the bn_add_relu_bwd_reduce pass and the masked-gradient write of the apply pass are gone for
        # every block whose successor's skip path is not a convolution
        fuse = self._fuse_tail_f32()
        gated = None
        for i in reversed(range(len(self.blocks))):
            dY = self._after_block_backward(i, dY, B)
            sb, sbb = sv["blocks"][i], sv["blocks"][i - 1] if i >= 1 else None
            # (a layer between the blocks adds its own gradient first: no gating of block i - 1 inside block i's data gradient)
            below = sbb if (fuse and sbb is not None and self.kinds[i - 1] != "conv" and sbb.get("ymask") is not None
                            and sb["kind"] != "none" and sb["cin"] % 8 == 0 and not self._layer_after(i - 1)) else None
            dY, gated = self._block_backward(i, sb, dY, B, gated, below)
            if self._deferred:
                self._flush_deferred()
            self._buckets_after_block(i, bucket_cb)
        if self.dense_A:
            self._dense_backward_end()
        # data_bn gamma/beta; the input's gradient only on request (need_dx)
        x = sv["x"]
        nch = V * self.C_in
        part = torch.empty((nch, N, 2), dtype=torch.float32, device=dev)
        ops.data_bn_bwd_reduce(x, self.bone_parent, dY, self.bn["data_bn"].mean, part, self.motion)
        self._bn_backward("data_bn", (part, N), 2, 1, N * M * sv["T"], coefficients=need_dx)
        self._finish_backward(bucket_cb)
        if need_dx:     # behind the last bucket's hand-over: the exchange does not wait for it
            b = self.bn["data_bn"]
            return ops.data_bn_bwd_apply(x, self.bone_parent, dY, (b.k1, b.k2, b.k3), motion=self.motion)
        return None

    def _fuse_tail_f32(self):
        """SAR_EPI_ADD_GATE in the fp32 graph data gradient (SAR_F32_FUSE_TAIL=0 turns it off): plain ST-GCN engine, fp32 MFMA
        operands, gather tables, ReLU masks written by the forward tails"""
        return (_FUSE_TAIL_F32 and self.stock_backward and not self.bf16 and not self.dense_A and not self.cn8
                and ops.RELU_MASK and not ops.BN_TAIL)

    def _bn_backward(self, name, sums, per, which, count, coefficients=True):
        """gamma / beta gradients of BatchNorm `name` and the coefficients k1..k3 of its backward apply pass, from sums = (partials,
        nparts, ..) of `per` sums per channel and partial over `count` samples; `which`: the second sum's position"""
        b = self.bn[name]
        ops.bn_bwd_finalize(sums[0], sums[1], sums[1] * per, per, 0, which, b.mean.numel(), count, self.p[name + ".gamma"], b.mean,
                            b.rstd, self.g[name + ".gamma"], self.g[name + ".beta"], *((b.k1, b.k2, b.k3) if coefficients else ()))

    def _tail_backward_sums(self, pre, sb, dY, n_out, gated, reduce):
        """Backward of the block tail y = relu(bn2(u) + res) (models/stgcn.py:37,62-63) up to its apply pass: the BatchNorm-backward
        sums of bn2 (and res_bn) finalised.  gated: the sums came with dY; else `reduce` (the engine's bn_add_relu_bwd_reduce)
        produces them, with ops.BN_TAIL its last workgroup per channel finalises as well (no launch between)."""
        y, u, kind = sb["y"], sb["u"], sb["kind"]
        bn2, rbn = self.bn[pre + "bn2"], self.bn.get(pre + "res_bn")
        r, rmean = (sb["r"], rbn.mean) if kind == "conv" else (None, None)
        if gated is not None:    # (sum dz, sum dz (u - mean)) per channel and partial
            assert kind != "conv"
            self._bn_backward(pre + "bn2", gated, 2, 1, n_out)
        elif ops.BN_TAIL:
            tail = ops.make_bn_tail(dY.device, n_out, self.p[pre + "bn2.gamma"], bn2, self.g[pre + "bn2.gamma"], self.g[pre + "bn2.beta"],
                                    *((self.p[pre + "res_bn.gamma"], rbn, self.g[pre + "res_bn.gamma"], self.g[pre + "res_bn.beta"])
                                      if kind == "conv" else ()))
            reduce(dY, y, u, r, bn2.mean, rmean, tail=tail)
        else:
            sums = reduce(dY, y, u, r, bn2.mean, rmean, mask=sb.get("ymask"))
            self._bn_backward(pre + "bn2", sums, 4, 1, n_out)
            if kind == "conv":
                self._bn_backward(pre + "res_bn", sums, 4, 2, n_out)

    def _block_backward(self, i, sb, dY, B, gated=None, below=None):
        """gated: this block's BatchNorm-backward partial sums when dY already carries the ReLU gate (produced by the graph data
        gradient of the block above); below: the saved tensors of block i - 1 when THIS block's graph data gradient is to do the
        same for it.  Returns (dX, sums-for-the-block-below or None)."""
        V, dev = self.V, dY.device
        pre = "l%d." % i
        X, g, u, r, y = sb["X"], sb["g"], sb["u"], sb["r"], sb["y"]
        T, To, pad, cin, f, s, kind = sb["T"], sb["To"], sb["pad"], sb["cin"], sb["f"], sb["s"], sb["kind"]
        n_in, n_out = B * T * V, B * To * V
        bn1, bn2 = self.bn[pre + "bn1"], self.bn[pre + "bn2"]
        rbn = self.bn.get(pre + "res_bn")
        self._tail_backward_sums(pre, sb, dY, n_out, gated, ops.bn_add_relu_bwd_reduce)
        rk = (rbn.k1, rbn.k2, rbn.k3) if kind == "conv" else None
        du = torch.empty_like(u)
        dr = torch.empty_like(r) if kind == "conv" else None
        dz = dY if (kind == "identity" and gated is None) else None  # in place: dY becomes the pre-ReLU gradient for the skip path (already gated: nothing to write)
        rec = self._recs[i]
        # (the bounds of du and dr -- operands of the data and weight gradients below -- are by-products of the pass)
        ops.bn_add_relu_bwd_apply(dY, y, u, r if kind == "conv" else None, (bn2.k1, bn2.k2, bn2.k3), rk, du, dr, dz,
                                  mask=sb.get("ymask"), amax_cell=rec.du, amax_dr_cell=rec.dr)
        # ---- temporal conv: weight / bias gradient, then data gradient fused with ReLU-mask + BN1 reductions
        wt = self.g[pre + "tcn.kernel"]
        flat_w = self.grad[self.offsets[pre + "tcn.kernel"]:self.offsets[pre + "tcn.bias"] + f]
        self._off_critical_path(lambda: ops.conv_wgrad(
            L.SAR_CONV_TEMPORAL, g, du, flat_w, B=B, V=V, T_src=T, T_out=To, Kc=f, M=f, taps=KT, stride=s, pad=pad,
            pro=(bn1.scale, bn1.shift), pro_relu=True, w_stride_tap=f * f, w_stride_c=f, wsize=wt.numel(), bsize=f,
            bf16=self.bf16, slabs=self._slabs, **(rec.twgrad or _NO_SPLIT)), g, du)
        wimg = self._img(pre + "tcn.b")
        wT = None
        if wimg is None:
            o = self._wT_off[pre + "tcn"]
            wT = self._wT[o:o + KT * f * f]                               # [tap][f][c], re-laid at the start of backward()
        dz1 = torch.empty((f, n_in), dtype=torch.float32, device=dev)
        pm = ops.conv_gemm(L.SAR_CONV_TEMPORAL, du, dz1, wT, f * f, f, B=B, V=V, T_src=To, T_out=T, Kc=f, M=f, taps=KT,
                           stride=s, pad=pad, transposed=True, epi=L.SAR_EPI_MASK, aux=g,
                           aux_affine=(bn1.scale, bn1.shift), aux_mean=bn1.mean, **self._arith(rec.tdgrad, wimg))
        self._bn_backward(pre + "bn1", pm, 2, 1, n_in)
        dg = dz1
        ops.affine2(dz1, g, (bn1.k1, bn1.k2, bn1.k3), dg, amax_cell=rec.dg)   # BN1 backward apply (in place; the bound of dg: by-product)
        flat_g = self.grad[self.offsets[pre + "gcn.kernel"]:self.offsets[pre + "gcn.bias"] + KS * f]
        if self.dense_A:
            return self._graph_backward_dense(i, sb, dg, dY, dr, B, flat_g), None
        # ---- graph conv: weight / bias gradient
        self._off_critical_path(lambda: ops.conv_wgrad(
            L.SAR_CONV_GRAPH, X, dg, flat_g, B=B, V=V, T_src=T, T_out=T, Kc=cin, M=f, taps=KS, tables=self.tab_fwd,
            w_stride_tap=f, w_stride_c=KS * f, wsize=cin * KS * f, bsize=KS * f, bf16=self.bf16, slabs=self._slabs,
            **(rec.gwgrad or _NO_SPLIT)), X, dg)
        dXres = self._residual_backward(i, sb, dr, B)
        # ---- graph conv data gradient (+ skip-path gradient)
        gimg = self._img(pre + "gcn.b")
        gT = None
        if gimg is None:
            o = self._wT_off[pre + "gcn"]
            gT = self._wT[o:o + KS * f * cin]                             # [k][f][c]
        dX = torch.empty((cin, n_in), dtype=torch.float32, device=dev)
        aux = dY if kind == "identity" else dXres
        even = kind == "conv" and aux is not None and rec.compact_skip   # dXres holds the even frames only
        if below is not None and aux is not None:
            # dX = gate_{i-1}(W^T dg . A^T + skip gradient) and block i - 1's BatchNorm-backward sums in one epilogue
            bn2b = self.bn["l%d.bn2" % (i - 1)]
            pm = ops.conv_gemm(L.SAR_CONV_GRAPH, dg, dX, gT, f * cin, cin, B=B, V=V, T_src=T, T_out=T, Kc=f, M=cin, taps=KS,
                               tables=self.tab_bwd, epi=L.SAR_EPI_ADD_GATE, aux=aux, aux2=below["u"], aux_mask=below["ymask"],
                               aux_mean=bn2b.mean, aux_even_frames=even, **self._arith(rec.gdgrad))
            return dX, pm
        ops.conv_gemm(L.SAR_CONV_GRAPH, dg, dX, gT, f * cin, cin, B=B, V=V, T_src=T, T_out=T, Kc=f, M=cin, taps=KS,
                      tables=self.tab_bwd, epi=L.SAR_EPI_ADD if aux is not None else L.SAR_EPI_NONE, aux=aux, aux_even_frames=even,
                      **self._arith(rec.gdgrad, gimg))
        return dX, None

    def _residual_backward(self, i, sb, dr, B):
        """weight gradient and data gradient of the strided 1x1 residual convolution (blocks 5 and 8); None otherwise"""
        if sb["kind"] != "conv":
            return None
        V, dev, pre = self.V, dr.device, "l%d." % i
        X, T, To, cin, f, s = sb["X"], sb["T"], sb["To"], sb["cin"], sb["f"], sb["s"]
        flat_r = self.grad[self.offsets[pre + "res.kernel"]:self.offsets[pre + "res.bias"] + f]
        rec = self._recs[i]
        rwgrad = (rec.rwgrad if T == s * To else None) or _NO_SPLIT      # (wgrad_tap1_split_kernel takes whole strides only)
        self._off_critical_path(lambda: ops.conv_wgrad(
            L.SAR_CONV_TEMPORAL, X, dr, flat_r, B=B, V=V, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s, pad=0,
            w_stride_tap=0, w_stride_c=f, wsize=cin * f, bsize=f, slabs=self._slabs, **rwgrad), X, dr)
        rimg = self._img(pre + "res.b")
        rT = None
        if rimg is None and pre + "res" in self._wT_off:
            o = self._wT_off[pre + "res"]
            rT = self._wT[o:o + f * cin]
        elif rimg is None:             # engines without the batched re-layout (ST-GIN)
            rT = torch.empty((f, cin), dtype=torch.float32, device=dev)
            ops.transpose(self.p[pre + "res.kernel"], rT, 1, cin, f)
        if rec.compact_skip:
            # the gradient through a stride-2 1x1 convolution is non-zero on EVEN input frames only: a dense 1x1 product over the To
            # frames (half the matrix work of the strided data gradient, half the bytes written), added by the graph data gradient's
            # epilogue on even frames (SAR_GRAPH_AUX_EVEN_FRAMES) -- the zeros are neither written nor read back
            dXc = torch.empty((cin, B * To * V), dtype=torch.float32, device=dev)
            ops.conv_gemm(L.SAR_CONV_TEMPORAL, dr, dXc, rT, 0, cin, B=B, V=V, T_src=To, T_out=To, Kc=f, M=cin, taps=1, stride=1, pad=0,
                          **self._arith(rec.rdgrad))
            return dXc
        dXres = torch.empty((cin, B * T * V), dtype=torch.float32, device=dev)
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, dr, dXres, rT, 0, cin, B=B, V=V, T_src=To, T_out=T, Kc=f, M=cin, taps=1,
                      stride=s, pad=0, transposed=True, bf16=self.bf16, packed=rimg)
        return dXres

    def _compact_skip(self, s, split_product=False):
        """the skip gradient of a conv-residual block as its even frames only (SAR_COMPACT_SKIP=0: the strided data gradient over all
        T frames): fp32-storage engines with gather tables and fp32 / split arithmetic.  Default ("fp32"): the fp32 engine, and the
        blocks of a split engine whose dense 1x1 product runs on conv_tap1_split_kernel (round 6; split_product).  Static per block:
        asked once, when the engine is built (BlockPlan.compact_skip)"""
        on = _COMPACT_SKIP == "1" or (_COMPACT_SKIP == "fp32" and (not self.split or split_product))
        return on and s == 2 and not self.bf16 and not self.cn8 and not self.dense_A and self.stock_backward

    def _graph_backward_dense(self, i, sb, dg, dY, dr, B, flat_g):
        """Backward of Conv2D(3F, 1x1) -> einsum with the trainable adjacency (models/gcn.py:229-237): dy3 = dg . A^T per
        slice, dA from (y3, dg), the 1x1 convolution's weight / bias / data gradients from (X, dy3)."""
        V, dev, pre = self.V, dg.device, "l%d." % i
        X, y3, T, cin, f, kind = sb["X"], sb["y3"], sb["T"], sb["cin"], sb["f"], sb["kind"]
        n_in = B * T * V
        dy3 = torch.empty_like(y3)
        self._dense_bwd_data(i, dg, dy3, f, B, T)
        if self.train_adjacency:
            self._dense_dA(i, y3, dg, f, B, T)
        self._off_critical_path(lambda: ops.conv_wgrad(
            L.SAR_CONV_TEMPORAL, X, dy3, flat_g, B=B, V=V, T_src=T, T_out=T, Kc=cin, M=KS * f, taps=1, stride=1, pad=0,
            w_stride_tap=0, w_stride_c=KS * f, wsize=cin * KS * f, bsize=KS * f, slabs=self._slabs), X, dy3)
        dXres = self._residual_backward(i, sb, dr, B)
        o = self._wT_off[pre + "gcn"]
        gT = self._wT[o:o + KS * f * cin]
        dX = torch.empty((cin, n_in), dtype=torch.float32, device=dev)
        aux = dY if kind == "identity" else dXres
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, dy3, dX, gT, 0, cin, B=B, V=V, T_src=T, T_out=T, Kc=KS * f, M=cin, taps=1, stride=1,
                      pad=0, transposed=True, epi=L.SAR_EPI_ADD if aux is not None else L.SAR_EPI_NONE, aux=aux)
        return dX

    # ------------------------------------------------------------------ training step
    def loss_and_grad(self, x, labels, global_batch_size=None, bucket_cb=None, need_dx=False):
        """main_gnn.py:221-233: loss = sum CE / global_batch; gradients of every trainable variable.  bucket_cb: backward().
        need_dx: returns (logits, loss, d loss / d x) as ResNet18Engine.loss_and_grad does."""
        logits = self.forward(x, training=True)
        N = x.shape[0]
        gbs = global_batch_size or N
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        dlogits = torch.empty_like(logits)
        ops.softmax_ce(logits, labels, 1.0 / gbs, loss, dlogits)
        dx = self.backward(dlogits, bucket_cb, need_dx)
        return (logits, loss, dx) if need_dx else (logits, loss)

    def sgd_step(self, lr, momentum=0.9):
        """tf.keras SGD(momentum, nesterov=True) over the flat buffers (main_gnn.py:312-314)."""
        self._set_lr(lr)
        ops.sgd_nesterov(self.flat, self.velocity, self.grad, self.lr_dev, momentum)

    def predict(self, x):
        """main_gnn.py:205-208: softmax(model(features, training=False))."""
        logits = self.forward(x, training=False)
        probs = torch.empty_like(logits)
        labels = torch.zeros(x.shape[0], dtype=torch.int64, device=x.device)
        ops.softmax_ce(logits, labels, 1.0, None, None, probs)
        return probs
