"""What the convolution launch wrappers (sar_amd.ops: conv_gemm, conv_wgrad, conv_gemm_nparts, conv2d_gemm, conv2d_wgrad; sar_amd.ops8:
conv_gemm, conv_wgrad) hand to the C ABI is what tests/golden/conv_launch_abi.json recorded at the commit its header names (written
once by tests/golden/make_golden_conv_launch_abi.py): for one train step of every engine arithmetic and for stand-alone calls through
every branch of the wrappers, every library call in issue order with its scalar arguments, every descriptor field and every pointer by
order of first appearance (tests/abi_trace.py; a digest of three hex digits per call, so a mismatch names the first call that
differs).  And the two routing rules of sar_amd.ops as tables written out by hand.  CPU only: nothing is launched."""
import json
import os
import re
import sys
from types import SimpleNamespace

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_conv_launch_abi as G  # noqa: E402

with open(os.path.join(G.HERE, "conv_launch_abi.json")) as _fh:
    GOLD = json.load(_fh)

_READERS = ("ops.py", "ops8.py", "stgcn.py", "stgcn8.py", "resnet.py")


def knob_set():
    """the first SAR_* variable one of _READERS reads that the environment sets (the fixture was recorded with none), or None"""
    for f in _READERS:
        with open(os.path.join(ROOT, "skeleton-action-recognition_amd", "sar_amd", f)) as fh:
            for name in re.findall(r"environ(?:\.get\(|\[)\s*\"(SAR_[A-Z0-9_]+)\"", fh.read()):
                if name in os.environ:
                    return name
    return None


def test_the_fixture_names_its_commit_and_covers_every_case():
    assert GOLD["commit"] == G.COMMIT and G.COMMIT in GOLD["header"]
    count = {}
    for group, name, _ in G.cases():
        count[group] = count.get(group, 0) + 1
    assert count == {g: len(v) for g, v in GOLD["digests"].items()}
    assert set(GOLD["traces"]) == set(G.FULL)
    assert os.path.getsize(os.path.join(G.HERE, "conv_launch_abi.json")) <= os.path.getsize(os.path.join(G.HERE, "pathb_schedule.json"))


@pytest.mark.parametrize("group", [g for g, _ in G.GROUPS])
def test_every_case_hands_the_library_what_was_recorded(group):
    knob = knob_set()
    if knob is not None:
        pytest.skip("%s is set: the fixture was recorded with the default of every SAR_* knob" % knob)
    want = iter(GOLD["digests"][group])
    for g, name, fn in G.cases():
        if g != group:
            continue
        calls, rec = G.record(fn), next(want)
        got = G.digest(calls)
        if got != rec:      # the digest has three hex digits per call: name the first call that differs
            n = G.first_difference(got, rec)
            full = GOLD["traces"].get(name, [])      # (a few cases are spelled out in the fixture)
            recorded = full[n] if n < len(full) else ("digest " + rec[3 * n:3 * n + 3] if n < len(rec) // 3 else "nothing")
            pytest.fail("%s: call %d is %s; recorded: %s (%d calls, recorded %d)" % (
                name, n, calls[n] if n < len(calls) else "missing", recorded, len(calls), len(rec) // 3))


# ---- the routing rules, written out by hand (B = 2, T = 12: the shapes of the stand-alone cases)
G_, T_ = 0, 1                                     # SAR_CONV_GRAPH, SAR_CONV_TEMPORAL
NONE, STATS, GATE = 0, 1, 4                       # SAR_EPI_*
FEW = SimpleNamespace(g_flags=4, n_dense_lists=9)         # tables with SAR_GRAPH_FEW_DENSE (the NTU graph)
DENSE = SimpleNamespace(g_flags=0, n_dense_lists=75)      # every gather list dense
ARITHS = ("f16x3a", "bf16x6", "bf16x3", "f16x3")
# (mode, taps, transposed, stride, pad, Kc, M, V, tables, pro, epi) -> the arithmetics that stay, the route of a bf16 call without one
GEMM_ROUTES = [
    # 9-tap temporal: V = 25, 8 <= Kc <= 256, M % 8 == 0, stride 1 / 2, every arithmetic, both directions, with a folded prologue
    ((T_, 9, False, 1, 4, 16, 24, 25, None, None, NONE), ARITHS, "bf16"),
    ((T_, 9, True, 2, 3, 16, 24, 25, None, True, STATS), ARITHS, "bf16"),
    ((T_, 9, False, 2, 3, 16, 20, 25, None, None, NONE), (), None),            # M % 8 != 0: neither
    ((T_, 9, True, 1, 4, 8, 24, 25, None, None, NONE), ARITHS, None),            # Kc = 8: split, no bf16 operands (Kc < 16)
    ((T_, 9, False, 1, 4, 4, 24, 25, None, None, NONE), (), None),             # Kc = 4: neither
    ((T_, 9, False, 1, 4, 16, 24, 18, None, None, NONE), (), "bf16"),          # V = 18: the split kernels are V = 25
    ((T_, 9, True, 1, 4, 16, 24, 25, None, None, GATE), (), "bf16"),           # the gated epilogue: graph kernel only
    # 1-tap temporal: forward form only, Kc >= 16, pad 0, no prologue, bf16x6 / f16x3a only
    ((T_, 1, False, 1, 0, 16, 24, 25, None, None, NONE), ("f16x3a", "bf16x6"), "bf16"),
    ((T_, 1, False, 2, 0, 16, 24, 25, None, None, STATS), ("f16x3a", "bf16x6"), "bf16"),
    ((T_, 1, True, 1, 0, 16, 24, 25, None, None, NONE), (), "bf16"),
    ((T_, 1, True, 2, 0, 16, 24, 25, None, None, NONE), (), "bf16"),
    ((T_, 1, False, 1, 1, 16, 24, 25, None, None, NONE), (), "bf16"),
    ((T_, 1, False, 1, 0, 16, 24, 25, None, True, NONE), (), "bf16"),
    ((T_, 1, False, 1, 0, 8, 24, 25, None, None, NONE), (), None),
    # graph: V = 25, Kc a multiple of 16, M % 8 == 0, no prologue, tables with few dense lists, bf16x6 / f16x3a only
    ((G_, 3, False, 1, 0, 16, 24, 25, FEW, None, STATS), ("f16x3a", "bf16x6"), "bf16"),
    ((G_, 3, False, 1, 0, 16, 24, 25, FEW, None, GATE), ("f16x3a", "bf16x6"), "bf16"),
    ((G_, 3, False, 1, 0, 32, 64, 25, FEW, None, NONE), ("f16x3a", "bf16x6"), "bf16"),
    ((G_, 3, False, 1, 0, 3, 64, 25, FEW, None, STATS), (), None),
    ((G_, 3, False, 1, 0, 16, 24, 25, DENSE, None, STATS), (), "bf16"),
    ((G_, 3, False, 1, 0, 16, 24, 25, FEW, True, NONE), (), "bf16"),
    ((G_, 3, False, 1, 0, 16, 24, 18, FEW, None, NONE), (), "bf16"),
    ((G_, 3, False, 1, 0, 16, 24, 25, None, None, NONE), (), "bf16"),
]


def _g2(k, s, p, Hs, Ho, Kc=16, M=16, tr=False):
    return dict(Kc=Kc, M=M, H_src=Hs, W_src=Hs, H_out=Ho, W_out=Ho, KH=k, KW=k, stride=s, pad=p, transposed=tr)


# (geometry, aux_even_pixels, epi) -> does bf16x6 / f16x3a stay
CONV2D_ROUTES = [
    ((_g2(3, 1, 1, 16, 16), False, STATS), True),              # 3x3 / 1 / 1: a window of 18 x 18 = 324 staged pixels
    ((_g2(3, 1, 1, 16, 16, tr=True), False, 2), True),
    ((_g2(3, 1, 1, 8, 8, Kc=256, M=256), False, NONE), True),  # 4 images of 10 x 10 = 400
    ((_g2(3, 1, 1, 4, 4), False, NONE), False),                # 16 images of 6 x 6 = 576 > 512
    ((_g2(3, 1, 1, 16, 16, Kc=8), False, NONE), True),
    ((_g2(3, 1, 1, 16, 16, Kc=4), False, NONE), False),
    ((_g2(3, 1, 1, 16, 16, M=20), False, NONE), False),
    ((_g2(3, 1, 1, 16, 16), True, 3), False),                  # the compact skip gradient belongs to the stride-2 data gradient
    ((_g2(3, 2, 1, 8, 16, tr=True), False, NONE), True),       # 3x3 / 2 / 1 data gradient onto twice the size
    ((_g2(3, 2, 1, 8, 16, tr=True), True, 3), True),           # ... with the compact skip gradient added (SAR_EPI_ADD)
    ((_g2(3, 2, 1, 8, 16, tr=True), True, NONE), False),
    ((_g2(3, 2, 1, 8, 16, Kc=8, tr=True), False, NONE), False),
    ((_g2(3, 2, 1, 16, 8), False, STATS), False),              # its forward form
    ((_g2(1, 2, 0, 16, 8), False, STATS), False),
    ((_g2(7, 2, 3, 32, 16, Kc=1, M=8), False, STATS), False),  # the stem
]


def test_the_routes_of_conv_gemm_as_a_table():
    from sar_amd import ops
    assert ops.DEFAULT_SPLIT is None and ops.TAP1_SPLIT
    for (mode, taps, tr, s, pad, Kc, M, V, tables, pro, epi), stay, bf16_route in GEMM_ROUTES:
        geo = (mode, V, Kc, M, taps, s, tables, pro, tr, pad, epi)
        for split in ARITHS:
            for bf16 in (False, True):
                want = split if split in stay else (bf16_route if bf16 else None)
                assert ops.conv_gemm_route(split, bf16, *geo) == want, (geo[:6], tr, split, bf16)
        assert ops.conv_gemm_route(None, True, *geo) == ops.conv_gemm_route("default", True, *geo) == bf16_route, geo[:6]
        assert ops.conv_gemm_route(None, False, *geo) is None and ops.conv_gemm_route("default", False, *geo) is None


def test_the_routes_of_conv2d_gemm_as_a_table(monkeypatch):
    from sar_amd import ops
    for (geo, even, epi), stays in CONV2D_ROUTES:
        for split in ("f16x3a", "bf16x6"):
            assert ops.conv2d_gemm_route(split, aux_even_pixels=even, epi=epi, **geo) == (split if stays else None), (geo, even, epi)
        for split in (None, "default", "bf16x3", "f16x3"):      # no arithmetic, and the ones the 2-d kernels are not built in
            assert ops.conv2d_gemm_route(split, aux_even_pixels=even, epi=epi, **geo) is None
    monkeypatch.setattr(ops, "DEFAULT_SPLIT", "f16x3a")         # what "default" means is read at the call
    assert ops.conv2d_gemm_route("default", **_g2(3, 1, 1, 16, 16)) == "f16x3a"
    assert ops.conv_gemm_route("default", False, T_, 25, 16, 24, 9, 1) == "f16x3a"


def test_the_default_nsplit_of_conv_wgrad_case_by_case():
    """conv_wgrad_route / conv_wgrad_nsplit with a stand-in for the library's answer: B = 2, T_out = 12, V = 25"""
    from sar_amd import ops
    sp = (3, 2, 100)                                   # 3 workgroups per slab group, 2 slabs per group, 100 positions per tile
    geo = dict(B=2, V=25, T_out=12, Kc=16, M=24, stride=1)
    assert ops.conv_wgrad_route("f16x3a", True, T_, 25, 9, 1, 4, lambda a: sp) == ("f16x3a", sp)
    assert ops.conv_wgrad_route("f16x3a", True, T_, 25, 9, 1, 4, lambda a: (-2, 0, 0)) == ("bf16", None)      # not built: next in line
    assert ops.conv_wgrad_route("f16x3", True, T_, 25, 9, 2, 4, None) == (None, None)       # never asked; bf16 wants pad 3 at stride 2
    assert ops.conv_wgrad_route(None, True, G_, 25, 3, 1, 0, None) == (None, None)
    # split: one round of 512 slots over 3 workgroups = 170 groups, at most the 2 * ceil(300 / 100) = 6 tiles, times wk
    assert ops.conv_wgrad_nsplit("f16x3a", sp, None, T_, taps=9, **geo) == 12
    assert ops.conv_wgrad_nsplit("f16x3a", sp, 3, T_, taps=9, **geo) == 4               # rounded up to a multiple of wk
    assert ops.conv_wgrad_nsplit("bf16", None, 3, T_, taps=9, **geo) == 3 == ops.conv_wgrad_nsplit(None, None, 3, T_, taps=9, **geo)
    assert ops.conv_wgrad_nsplit("bf16", None, None, T_, taps=9, **geo) == 4            # 2 * ceil(12 / 8) tiles < 512 slots / 1 block
    assert ops.conv_wgrad_nsplit(None, None, None, G_, taps=3, **dict(geo, Kc=3, M=64)) == 1        # streaming: 600 of 4096 columns
    assert ops.conv_wgrad_nsplit(None, None, None, G_, taps=3, **dict(geo, Kc=32, M=128)) == 12     # fixed geometry: 2-frame tiles
    assert ops.conv_wgrad_nsplit(None, None, None, G_, taps=3, pro=True, **dict(geo, Kc=32, M=128)) == 6     # generic: 4-frame tiles
    assert ops.conv_wgrad_nsplit(None, None, None, T_, taps=9, **geo) == 6 == ops.conv_wgrad_nsplit(None, None, None, T_, taps=1, **geo)
