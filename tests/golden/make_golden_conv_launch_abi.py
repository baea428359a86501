"""Writes tests/golden/conv_launch_abi.json: what the convolution launch wrappers of sar_amd.ops / sar_amd.ops8 hand to the C ABI --
every entry point called, its scalar arguments, every descriptor field and every pointer by order of first appearance
(tests/abi_trace.py), in issue order -- for one train step of every engine arithmetic and for stand-alone calls that take every
branch of the wrappers' routing, of the weight gradient's default `nsplit` and of the slab and bound-cell hand-off.  Everything runs
on zero-filled CPU tensors; nothing is launched.

The fixture was written ONCE, at commit f3c171e ("ResNet-18 engine: one split-arithmetic plan, built at construction"), the parent
of the change that gave the wrappers one descriptor builder, one slab path and one bounds path, with no SAR_* knob set.  It is never
regenerated from the code under test: tests/test_conv_launch_abi.py imports cases() from here and replays them.

A case is (name, function); the function runs inside an AbiTrace and the case's record is the trace it leaves.  The fixture holds
a digest of three hex digits per recorded call (make_golden_split_schedule.digest), the cases in the order cases() yields them,
and the cases of FULL spelled out for reading."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import make_golden_split_schedule as S  # noqa: E402  (puts the repository on sys.path)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from abi_trace import AbiTrace  # noqa: E402

COMMIT = "f3c171e"
BLOCKS, CLIP = S.BLOCKS, S.CLIP
B, T = 2, 12
EPI = {"NONE": 0, "STATS": 1, "MASK": 2, "ADD": 3, "GATE": 4}
FULL = ("step STGCN f32_split", "cg9 fwd s2 16x24 V25 f16x3a STATS pro",
        "cg9 dgrad s1 16x24 V25 bf16x6 bf16 MASK handed", "cgG ntu 16x24 f16x3a GATE", "cgG ntu 16x24 - STATS partials_out",
        "wg9 s2p3 16x24 f16x3a n3 batch", "wgG 32x128 V25 - n- alone", "cn8 wgG ntu batch", "c2d 3x3s1 8x8 256x256 fwd f16x3a STATS kslab",
        "c2w w12 f16x3a alone", "c2w w8 f16x3a batch")


def Z(*shape, dtype=torch.float32):
    return torch.zeros(shape, dtype=dtype)


def rows(c, n, extra=4):
    """a (c, n) operand whose rows are `extra` elements apart beyond their length: a leading dimension that is not the row length"""
    return Z(c, n + extra)[:, :n]


def cn8(c, n):
    return Z((c + 7) // 8, n, 8, dtype=torch.bfloat16)


def cells():
    c = Z(2, dtype=torch.int32)
    return c[0:1], c[1:2]


def ntu(transpose=False):
    from sar_amd import ops, stgcn
    return ops.GraphTables(stgcn.ntu_adjacency().astype(np.float32), "cpu", transpose)


def dense(V=25, seed=0):
    """three weighted entries per column: every gather list is dense, no slice is the identity"""
    from sar_amd import ops
    rng = np.random.RandomState(seed)
    A = np.zeros((3, V, V), dtype=np.float32)
    for k in range(3):
        for w in range(V):
            A[k, rng.choice(V, 3, replace=False), w] = rng.uniform(0.1, 0.9, 3).astype(np.float32)
    return ops.GraphTables(A, "cpu")


def ring(V):
    """a sparse graph on V joints: identity, successor, predecessor (unit weights)"""
    from sar_amd import ops
    eye = np.eye(V, dtype=np.float32)
    return ops.GraphTables(np.stack([eye, np.roll(eye, 1, axis=1), np.roll(eye, -1, axis=1)]), "cpu")


# ------------------------------------------------------------------------------------------------ engine steps
def _stgcn_step(cls, **kw):
    def run():
        eng = cls(device="cpu", num_classes=7, blocks=BLOCKS, **kw)
        logits = eng.forward(torch.zeros(CLIP), training=True)
        eng.backward(torch.zeros_like(logits))
    return run


def _resnet_step(mode):
    def run():
        from sar_amd import resnet
        eng = resnet.ResNet18(device="cpu", num_classes=7, num_filters=8, mfma=mode)
        eng.loss_and_grad(torch.zeros(2, 1, 32, 32), torch.zeros(2, dtype=torch.int64), need_dx=True)
    return run


def engine_cases():
    from sar_amd import stgcn, stgin
    for mode in ("fp32", "bf16_operands", "bf16", "f32_split", "f32_split_bf16x6"):
        yield "step STGCN " + mode, _stgcn_step(stgcn.STGCN, mfma=mode)
    yield "step STGCN fp32 trainable_adjacency", _stgcn_step(stgcn.STGCN, mfma="fp32", trainable_adjacency=True)
    yield "step STGIN", _stgcn_step(stgin.STGIN)
    for mode in ("fp32", "f32_split", "f32_split_bf16x6"):
        yield "step ResNet18 " + mode, _resnet_step(mode)


# ------------------------------------------------------------------------------------------------ ops.conv_gemm
def _handed(split, bf16):
    """the operand image and the bound cells a caller that keeps its own hands in"""
    return dict(packed=Z(64, dtype=torch.uint8), bounds=cells() if split else None)


def _temporal(taps, transposed, stride, pad, Kc, M, V, split, bf16, epi, pro, handed):
    def run():
        from sar_amd import ops, _lib as L
        To = -(-T // stride)
        Ts, Td = (To, T) if transposed else (T, To)
        src, out = rows(Kc, B * Ts * V), rows(M, B * Td * V, 8)
        kw = dict(B=B, V=V, T_src=Ts, T_out=Td, Kc=Kc, M=M, taps=taps, stride=stride, pad=pad, transposed=transposed,
                  bias=None if transposed else Z(M), epi=EPI[epi], bf16=bf16, split=split)
        if pro:
            kw.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        if epi == "MASK":
            kw.update(aux=rows(M, B * Td * V, 12), aux_affine=(Z(M), Z(M)), aux_mean=Z(M))
        if handed:
            kw.update(_handed(split, bf16))
        ops.conv_gemm(L.SAR_CONV_TEMPORAL, src, out, Z(taps, Kc, M), (Kc * M if taps > 1 else 0), M, **kw)
    return run


def _name(*parts):
    return " ".join(p for p in parts if p)


def temporal_gemm_cases():
    shapes = [(16, 24, 25), (16, 20, 25), (8, 24, 25), (4, 24, 25), (16, 24, 18)]
    for tr, s, (Kc, M, V), split, bf16, epi, pro, handed in itertools.product(
            (False, True), (1, 2), shapes, (None, "f16x3a", "bf16x6", "bf16x3", "f16x3"), (False, True), ("NONE", "STATS", "MASK"),
            (False, True), (False, True)):
        if handed and not (split or bf16):
            continue
        yield (_name("cg9", "dgrad" if tr else "fwd", "s%d" % s, "%dx%d" % (Kc, M), "V%d" % V, split or "-", bf16 and "bf16",
                     epi, pro and "pro", handed and "handed"),
               _temporal(9, tr, s, 4 if s == 1 else 3, Kc, M, V, split, bf16, epi, pro, handed))
    for (tr, s, pad), (Kc, M), split, bf16, epi, handed in itertools.product(
            ((False, 1, 0), (False, 2, 0), (True, 1, 0), (True, 2, 0), (False, 1, 1)), ((16, 24), (8, 24)),
            (None, "f16x3a", "bf16x6", "bf16x3"), (False, True), ("NONE", "STATS"), (False, True)):
        if handed and not (split or bf16):
            continue
        yield (_name("cg1", "dgrad" if tr else "fwd", "s%dp%d" % (s, pad), "%dx%d" % (Kc, M), split or "-", bf16 and "bf16", epi,
                     handed and "handed"),
               _temporal(1, tr, s, pad, Kc, M, 25, split, bf16, epi, False, handed))


def _graph(tables, Kc, M, V, split, bf16, epi, even=False, one_tile=False, partials_out=False, handed=False, pro=False):
    def run():
        from sar_amd import ops, _lib as L
        n = B * T * V
        src, out = rows(Kc, n), rows(M, n, 8)
        kw = dict(B=B, V=V, T_src=T, T_out=T, Kc=Kc, M=M, taps=3, tables=tables(), epi=EPI[epi], bf16=bf16, split=split,
                  bias=Z(3 * M) if epi in ("NONE", "STATS") else None)
        if pro:
            kw.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        if epi in ("ADD", "GATE"):
            kw.update(aux=rows(M, B * (T // 2) * V if even else n, 12), aux_even_frames=even)
        if epi == "GATE":
            aux2 = rows(M, n, 4)
            kw.update(aux2=aux2, aux_mask=Z(M, aux2.stride(0) // 4, dtype=torch.uint8), aux_mean=Z(M))
        if handed:
            kw.update(_handed(split, bf16))
        old, ops.GRAPH_ONE_TILE_WG = ops.GRAPH_ONE_TILE_WG, one_tile
        try:
            r = ops.conv_gemm(L.SAR_CONV_GRAPH, src, out, Z(Kc, 3 * M), M, 3 * M, **kw)
            if partials_out:      # a caller-owned slice of a stacked partials tensor
                ops.conv_gemm(L.SAR_CONV_GRAPH, src, out, Z(Kc, 3 * M), M, 3 * M, partials_out=Z(2, M, r[1], 2)[1], **kw)
        finally:
            ops.GRAPH_ONE_TILE_WG = old
    return run


def graph_gemm_cases():
    for (tname, tables, V), (Kc, M), split, bf16, epi in itertools.product(
            (("ntu", ntu, 25), ("ntuT", lambda: ntu(True), 25), ("dense", dense, 25), ("ring18", lambda: ring(18), 18)),
            ((16, 24), (3, 64), (32, 64)), (None, "f16x3a", "bf16x6", "bf16x3"), (False, True), ("NONE", "STATS", "ADD", "GATE")):
        if epi == "GATE" and bf16:      # the gated epilogue is the fp32 and the split kernels'
            continue
        yield _name("cgG", tname, "%dx%d" % (Kc, M), split or "-", bf16 and "bf16", epi), _graph(tables, Kc, M, V, split, bf16, epi)
    for split in (None, "f16x3a", "bf16x6"):
        s = split or "-"
        yield _name("cgG ntu 16x24", s, "ADD even"), _graph(lambda: ntu(True), 16, 24, 25, split, False, "ADD", even=True)
        yield _name("cgG ntu 16x24", s, "GATE even"), _graph(lambda: ntu(True), 16, 24, 25, split, False, "GATE", even=True)
        yield _name("cgG ntu 16x24", s, "STATS one_tile"), _graph(ntu, 16, 24, 25, split, False, "STATS", one_tile=True)
        yield _name("cgG ntu 16x24", s, "ADD even one_tile"), _graph(lambda: ntu(True), 16, 24, 25, split, False, "ADD", even=True, one_tile=True)
        yield _name("cgG ntu 16x24", s, "STATS partials_out"), _graph(ntu, 16, 24, 25, split, False, "STATS", partials_out=True)
        yield _name("cgG ntu 16x24", s, "STATS handed"), _graph(ntu, 16, 24, 25, split or "f16x3", True, "STATS", handed=True)
        yield _name("cgG ntu 16x24", s, "NONE pro"), _graph(ntu, 16, 24, 25, split, False, "NONE", pro=True)


def nparts_cases():
    def run(**kw):
        def go():
            from sar_amd import ops
            ops.conv_gemm_nparts(B, 25, **kw)
        return go
    yield "nparts 1-tap s2", run(T_src=T, T_out=T // 2, Kc=16, M=24, taps=1, stride=2)
    yield "nparts 9-tap dgrad MASK", run(T_src=T // 2, T_out=T, Kc=24, M=16, taps=9, stride=2, pad=3, transposed=True, epi=EPI["MASK"])


# ------------------------------------------------------------------------------------------------ ops.conv_wgrad
def _finish(slabs, call):
    """slabs: "alone" = the wrapper reduces its own slab; "batch" = a SlabBatch, the call made twice (the second finds its slab),
    then flush()"""
    from sar_amd import ops
    if slabs == "alone":
        call(None)
        return
    sb = ops.SlabBatch()
    call(sb)
    call(sb)
    sb.flush()


def _wgrad(mode, taps, stride, pad, Kc, M, V, tables, split, bf16, nsplit, pro, bounds, slabs):
    def run():
        from sar_amd import ops
        To = -(-T // stride)
        graph = mode == 0
        wsize, bsize = Kc * taps * M, (3 * M if graph else M)
        src, dout, dW = rows(Kc, B * T * V), rows(M, B * To * V, 8), Z(wsize + bsize)
        kw = dict(B=B, V=V, T_src=T, T_out=To, Kc=Kc, M=M, taps=taps, stride=stride, pad=pad, tables=tables() if tables else None,
                  w_stride_tap=(M if graph else (Kc * M if taps > 1 else 0)), w_stride_c=(3 * M if graph else M), wsize=wsize,
                  bsize=bsize, nsplit=nsplit, bf16=bf16, split=split, bounds=cells() if bounds else None)
        if pro:
            kw.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        _finish(slabs, lambda sb: ops.conv_wgrad(mode, src, dout, dW, slabs=sb, **kw))
    return run


def wgrad_cases():
    splits = (None, "f16x3a", "bf16x6")
    for (s, pad), (Kc, M), split, bf16, nsplit, slabs in itertools.product(
            ((1, 4), (2, 3), (2, 4)), ((16, 24), (64, 72)), splits, (False, True), (None, 3), ("alone", "batch")):
        yield (_name("wg9", "s%dp%d" % (s, pad), "%dx%d" % (Kc, M), split or "-", bf16 and "bf16", "n%s" % (nsplit or "-"), slabs),
               _wgrad(1, 9, s, pad, Kc, M, 25, None, split, bf16, nsplit, False, False, slabs))
    for split, pro, bounds in itertools.product(splits, (False, True), (False, True)):
        yield (_name("wg9 s1p4 16x24", split or "-", pro and "pro", bounds and "bounds"),
               _wgrad(1, 9, 1, 4, 16, 24, 25, None, split, False, None, pro, bounds, "alone"))
    for s, split, bf16, nsplit, slabs in itertools.product((1, 2), splits, (False, True), (None, 3), ("alone", "batch")):
        yield (_name("wg1", "s%d" % s, "16x24", split or "-", bf16 and "bf16", "n%s" % (nsplit or "-"), slabs),
               _wgrad(1, 1, s, 0, 16, 24, 25, None, split, bf16, nsplit, False, False, slabs))
    for (Kc, M, V, tname, tables), split, pro, nsplit, slabs in itertools.product(
            ((3, 64, 25, "ntu", ntu), (32, 64, 25, "ntu", ntu), (32, 128, 25, "ntu", ntu), (32, 64, 18, "ring18", lambda: ring(18)),
             (32, 64, 25, "dense", dense)), splits, (False, True), (None, 3), ("alone", "batch")):
        yield (_name("wgG", "%dx%d" % (Kc, M), "V%d" % V, tname != "ntu" and tname, split or "-", pro and "pro", "n%s" % (nsplit or "-"),
                     slabs),
               _wgrad(0, 3, 1, 0, Kc, M, V, tables, split, False, nsplit, pro, False, slabs))


# ------------------------------------------------------------------------------------------------ sar_amd.ops8
def _cn8_gemm(mode, taps, stride, pad, transposed, Kc, M, tables, epi, pro):
    def run():
        from sar_amd import ops8
        To = -(-T // stride)
        Ts, Td = (To, T) if transposed else (T, To)
        src, out = cn8(Kc, B * Ts * 25 + 3), cn8(M, B * Td * 25 + 5)
        kw = dict(B=B, V=25, T_src=Ts, T_out=Td, Kc=Kc, M=M, taps=taps, stride=stride, pad=pad, transposed=transposed,
                  tables=tables() if tables else None, epi=EPI[epi], bias=Z(M if mode else 3 * M) if epi in ("NONE", "STATS") else None)
        if pro:
            kw.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        if epi == "MASK":
            kw.update(aux=cn8(M, B * Td * 25 + 7), aux_affine=(Z(M), Z(M)), aux_mean=Z(M))
        if epi in ("ADD", "GATE"):
            kw.update(aux=cn8(M, B * Td * 25 + 7))
        if epi == "GATE":
            ld2 = B * Td * 25 + 9
            kw.update(aux2=cn8(M, ld2), aux_mask=Z((M + 7) // 8, ld2, dtype=torch.uint8), aux_mean=Z(M))
        ops8.conv_gemm(mode, src, out, Z(64, dtype=torch.uint8), **kw)
    return run


def _cn8_wgrad(mode, taps, stride, pad, Kc, M, tables, pro, nsplit, slabs):
    def run():
        from sar_amd import ops8
        To = -(-T // stride)
        graph = mode == 0
        wsize, bsize = Kc * taps * M, (3 * M if graph else M)
        src, dout, dW = cn8(Kc, B * T * 25 + 3), cn8(M, B * To * 25 + 5), Z(wsize + bsize)
        kw = dict(B=B, V=25, T_src=T, T_out=To, Kc=Kc, M=M, taps=taps, stride=stride, pad=pad, tables=tables() if tables else None,
                  w_stride_tap=(M if graph else (Kc * M if taps > 1 else 0)), w_stride_c=(3 * M if graph else M), wsize=wsize,
                  bsize=bsize, nsplit=nsplit)
        if pro:
            kw.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        _finish(slabs, lambda sb: ops8.conv_wgrad(mode, src, dout, dW, slabs=sb, **kw))
    return run


def cn8_cases():
    for (tr, s), epi, pro in itertools.product(((False, 1), (False, 2), (True, 1), (True, 2)), ("NONE", "STATS", "MASK"), (False, True)):
        yield (_name("cn8 cg9", "dgrad" if tr else "fwd", "s%d" % s, epi, pro and "pro"),
               _cn8_gemm(1, 9, s, 4 if s == 1 else 3, tr, 16, 24, None, epi, pro))
    for (tr, s), epi in itertools.product(((False, 1), (False, 2), (True, 2)), ("NONE", "STATS")):
        yield _name("cn8 cg1", "dgrad" if tr else "fwd", "s%d" % s, epi), _cn8_gemm(1, 1, s, 0, tr, 16, 24, None, epi, False)
    for (tname, tables), epi in itertools.product((("ntu", ntu), ("ntuT", lambda: ntu(True)), ("dense", dense)),
                                                  ("NONE", "STATS", "ADD", "GATE")):
        if epi == "GATE" and tname == "dense":      # the gated epilogue is built for tables with SAR_GRAPH_FEW_DENSE
            continue
        yield _name("cn8 cgG", tname, epi), _cn8_gemm(0, 3, 1, 0, False, 16, 24, tables, epi, False)
    for slabs, nsplit in itertools.product(("alone", "batch"), (None, 3)):
        n = nsplit and "n3"
        yield _name("cn8 wg9 s1", n, slabs), _cn8_wgrad(1, 9, 1, 4, 16, 24, None, False, nsplit, slabs)
        yield _name("cn8 wg9 s2 pro", n, slabs), _cn8_wgrad(1, 9, 2, 3, 64, 72, None, True, nsplit, slabs)
        yield _name("cn8 wg1 s2", n, slabs), _cn8_wgrad(1, 1, 2, 0, 16, 24, None, False, nsplit, slabs)
        yield _name("cn8 wgG ntu", n, slabs), _cn8_wgrad(0, 3, 1, 0, 16, 24, ntu, False, nsplit, slabs)
        yield _name("cn8 wgG dense", n, slabs), _cn8_wgrad(0, 3, 1, 0, 16, 24, dense, False, nsplit, slabs)


# ------------------------------------------------------------------------------------------------ the 2-d convolutions
def _c2d(geo, split, epi, handed=False, kslab=False, even=False, pro=False):
    def run():
        from sar_amd import ops
        g = dict(geo, B=B)
        n_src, n_out = B * g["H_src"] * g["W_src"], B * g["H_out"] * g["W_out"]
        Kc, M, taps = g["Kc"], g["M"], g["KH"] * g["KW"]
        kw = dict(epi=EPI[epi], split=split, aux_even_pixels=even)
        if pro:
            g.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        if epi == "MASK":
            kw.update(aux=rows(M, n_out, 12), aux_affine=(Z(M), Z(M)), aux_mean=Z(M))
        if epi == "ADD":
            kw.update(aux=rows(M, n_src if even else n_out, 12))
        if handed:
            kw.update(_handed(split, False))
        if kslab:
            kw.update(kslab=lambda nfloats: Z(nfloats + 16))
        ops.conv2d_gemm(rows(Kc, n_src), rows(M, n_out, 8), Z(taps, Kc, M), Kc * M, M, **kw, **g)
    return run


def conv2d_cases():
    def geo(k, s, p, Hs, Ho, Kc=16, M=16, tr=False):
        return dict(Kc=Kc, M=M, H_src=Hs, W_src=Hs, H_out=Ho, W_out=Ho, KH=k, KW=k, stride=s, pad=p, transposed=tr)
    splits = (None, "f16x3a", "bf16x6")
    for hw, tr, split, epi, handed in itertools.product((16, 4), (False, True), splits, ("NONE", "STATS", "MASK"), (False, True)):
        if handed and not split:
            continue
        name = _name("c2d 3x3s1 %dx%d" % (hw, hw), "dgrad" if tr else "fwd", split or "-", epi, handed and "handed")
        yield name, _c2d(geo(3, 1, 1, hw, hw, tr=tr), split, epi, handed)      # (the 4x4 map is not split-eligible: 576 staged pixels)
    # the K-split workspace (sar_conv2d_gemm_split_slab_bytes > 0: an 8x8 map at 256 channels), from torch.empty and from the caller's provider
    for tr, split, epi, kslab in itertools.product((False, True), splits, ("NONE", "STATS"), (False, True)):
        yield (_name("c2d 3x3s1 8x8 256x256", "dgrad" if tr else "fwd", split or "-", epi, kslab and "kslab"),
               _c2d(geo(3, 1, 1, 8, 8, Kc=256, M=256, tr=tr), split, epi, kslab=kslab))
    for split, pro in itertools.product(splits, (False, True)):
        s = split or "-"
        yield _name("c2d 3x3s1 16x16 fwd Kc8", s, pro and "pro"), _c2d(geo(3, 1, 1, 16, 16, Kc=8), split, "STATS", pro=pro)
        yield _name("c2d 3x3s2 dgrad", s, pro and "pro"), _c2d(geo(3, 2, 1, 8, 16, tr=True), split, "NONE", pro=pro)
        yield _name("c2d 3x3s2 dgrad MASK", s, pro and "pro"), _c2d(geo(3, 2, 1, 8, 16, tr=True), split, "MASK", pro=pro)
        yield _name("c2d 3x3s2 dgrad ADD even", s, pro and "pro"), _c2d(geo(3, 2, 1, 8, 16, tr=True), split, "ADD", even=True, pro=pro)
        yield _name("c2d 3x3s2 dgrad ADD", s, pro and "pro"), _c2d(geo(3, 2, 1, 8, 16, tr=True), split, "ADD", pro=pro)
        yield _name("c2d 3x3s2 fwd", s, pro and "pro"), _c2d(geo(3, 2, 1, 16, 8), split, "STATS", pro=pro)
        yield _name("c2d 1x1s2 fwd", s, pro and "pro"), _c2d(geo(1, 2, 0, 16, 8), split, "STATS", pro=pro)
        yield _name("c2d 1x1s2 dgrad", s, pro and "pro"), _c2d(geo(1, 2, 0, 8, 16, tr=True), split, "NONE", pro=pro)
        yield _name("c2d stem 7x7s2", s, pro and "pro"), _c2d(geo(7, 2, 3, 32, 16, Kc=1, M=8), split, "STATS", pro=pro)


def _c2w(geo, split, bounds, slabs, pro=False):
    def run():
        from sar_amd import ops
        g = dict(geo, B=B)
        Kc, M, taps = g["Kc"], g["M"], g["KH"] * g["KW"]
        if pro:
            g.update(pro=(Z(Kc), Z(Kc)), pro_relu=True)
        src, dout, dW = rows(Kc, B * g["H_src"] * g["W_src"]), rows(M, B * g["H_out"] * g["W_out"], 8), Z(taps * Kc * M)
        if bounds == "src":
            bounds_ = (cells()[0], None)
        else:
            bounds_ = cells() if bounds else None
        _finish(slabs, lambda sb: ops.conv2d_wgrad(src, dout, dW, split=split, bounds=bounds_, slabs=sb, **g))
    return run


def conv2d_wgrad_cases():
    def geo(k, s, p, Hs, Ho, Kc=16, M=16):
        return dict(Kc=Kc, M=M, H_src=Hs, W_src=Hs, H_out=Ho, W_out=Ho, KH=k, KW=k, stride=s, pad=p)
    for w, split, bounds, slabs, pro in itertools.product((8, 16, 12), (None, "f16x3a", "bf16x6"), (False, True, "src"), ("alone", "batch"),
                                                         (False, True)):
        if bounds and not split:
            continue
        yield (_name("c2w w%d" % w, split or "-", bounds and ("bounds" if bounds is True else "src_bound"), pro and "pro", slabs),
               _c2w(geo(3, 1, 1, w, w), split, bounds, slabs, pro))
    for split, slabs in itertools.product((None, "f16x3a"), ("alone", "batch")):
        yield _name("c2w 1x1s2", split or "-", slabs), _c2w(geo(1, 2, 0, 16, 8), split, False, slabs)
        yield _name("c2w stem 7x7s2", split or "-", slabs), _c2w(geo(7, 2, 3, 32, 16, Kc=1, M=8), split, False, slabs)
        yield _name("c2w 3x3s2", split or "-", slabs), _c2w(geo(3, 2, 1, 16, 8, M=72), split, False, slabs)


GROUPS = (("engine", engine_cases), ("conv_gemm temporal", temporal_gemm_cases), ("conv_gemm graph", graph_gemm_cases),
          ("conv_gemm_nparts", nparts_cases), ("conv_wgrad", wgrad_cases), ("ops8", cn8_cases), ("conv2d_gemm", conv2d_cases),
          ("conv2d_wgrad", conv2d_wgrad_cases))


def cases():
    """(group, name, function), in the fixture's order"""
    for group, gen in GROUPS:
        for name, fn in gen():
            yield group, name, fn


def record(fn):
    """the calls one case leaves"""
    with AbiTrace() as tr:
        fn()
    return tr.calls


digest, first_difference = S.digest, S.first_difference


def write_fixture(out, commit, cases, FULL, generator):
    """the fixture of `generator` (a module's name): the digest of every case of cases(), the traces of the cases named in FULL"""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    digests, full, seen = {}, {}, set()
    for group, name, fn in cases():
        assert name not in seen, "two cases are named %r" % name
        seen.add(name)
        calls = record(fn)
        digests.setdefault(group, []).append(digest(calls))
        if name in FULL:
            full[name] = calls
    assert set(full) == set(FULL), set(FULL) - set(full)
    header = ("recorded at commit %s with no SAR_* knob set, on a machine without a GPU; digests: three hex digits per recorded call, "
              "per group the cases in the order of %s.cases()" % (commit, generator))
    with open(out, "w") as fh:
        fh.write('{"header": %s,\n"commit": %s,\n"digests": {\n' % (json.dumps(header), json.dumps(commit))
                 + ",\n".join("%s: [\n%s\n]" % (json.dumps(g), ",\n".join(json.dumps(d) for d in v)) for g, v in digests.items())
                 + '\n},\n"traces": {\n'
                 + ",\n".join("%s: [\n  %s\n]" % (json.dumps(k), ",\n  ".join(json.dumps(e, sort_keys=True) for e in v))
                              for k, v in full.items()) + "\n}}\n")
    print("wrote %d cases in %d groups, %d full traces, %d bytes" % (len(seen), len(digests), len(full), os.path.getsize(out)))


if __name__ == "__main__":
    write_fixture(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_launch_abi.json"), COMMIT, cases, FULL,
                  "make_golden_conv_launch_abi")
