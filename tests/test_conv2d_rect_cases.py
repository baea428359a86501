"""CPU: the case tables of tests/conv2d_rect_cases.py are worth running.  Three properties, no library loaded:

  * sensitivity: the float64 reference of every case of groups A to G changes by more than 1e-2 (rel_err) when the same flat buffers
    are read as (W, H) images -- an H / W exchange in a kernel's geometry cannot pass the case.  Group G's 4 x 4 map is square, so
    every G case also gets the batch control: images 0 and 1 exchanged (several whole images share a tile there).
  * float32 band: the float32 CPU evaluation of the same reference stays under 1/4 of the bar the GPU test holds the kernel to
    (5e-6 of 2e-5, 2.5e-5 of 1e-4).  A failure means the case is badly conditioned: change its inputs, not the bar.
  * route table: the pure host functions (ops.conv2d_gemm_route / conv2d_split_applicable) and the Python restatement of launch_wgrad's
    tile choice, the stride-2 data-gradient dispatch, the max-pool tile grid and gemm_geometry's images per tile put every case on
    the path the table names; every path is hit, and the ragged last row tile (H_out % th != 0) holds where claimed."""
import pytest
import torch

import conv2d_rect_cases as RC
from util import rel_err

F32 = torch.float32
SENS = 1e-2


def _conv_args(group):
    """(cin, cout, k, s, H, W, B) of every conv_ref case of a group and the reference tensors its GPU test checks: (name, bar)"""
    if group == "A":
        return [((cin, cout, 3, 2, H, W, RC.A_BATCH), [("gh", RC.TOL), ("dz", RC.TOL), ("dz_sum", RC.TOL_SUM), ("dz_cen", RC.TOL_SUM)] +
                 ([("gh_even", RC.TOL)] if (cin, cout, H, W) in RC.A_PARITY else []))
                for cin, cout, H, W in RC.A_PARITY + RC.A_MASKED]
    if group == "B":
        return [((cin, cout, 1, 2, H, W, 2), [("y", RC.TOL), ("ysq", RC.TOL), ("gh", RC.TOL), ("gw", RC.TOL)]) for cin, cout, H, W in RC.B_CASES]
    if group == "C":
        return [((1, cout, 7, 2, H, W, 2), [("y", RC.TOL), ("ysq", RC.TOL), ("gw", RC.TOL)]) for cout, H, W in RC.C_CASES]
    if group == "F":
        return [((cin, cout, 3, s, H, W, 2), [("gw", RC.TOL)]) for cin, cout, s, H, W in RC.F_ALL]
    if group == "G":
        return [((cin, cout, 3, 1, H, W, B), [("y", RC.TOL), ("ysq", RC.TOL), ("dz", RC.TOL), ("dz_sum", RC.TOL_SUM), ("dz_cen", RC.TOL_SUM)])
                for cin, cout, H, W, B in RC.G_CASES]
    raise KeyError(group)


CONV_CASES = [(g,) + c for g in "ABCFG" for c in _conv_args(g)]
TENSORS = ("y", "gh", "gw", "dz", "gh_even")      # the controls are asked of the tensors, not of their per-channel sums


def _ids(cases):
    return ["%s-%s" % (c[0], "x".join(str(v) for v in c[1])) for c in cases]


@pytest.mark.parametrize("group,args,checked", CONV_CASES, ids=_ids(CONV_CASES))
def test_conv_cases_are_sensitive_and_well_conditioned(group, args, checked):
    ref, swapped, f32 = RC.conv_ref(*args), RC.conv_ref(*args, control="hw"), RC.conv_ref(*args, dtype=F32)
    H, W = args[4], args[5]
    for name, bar in checked:
        band = rel_err(f32[name], ref[name])
        line = "%s %s %-8s float32 band %.2e (bar %.1e)" % (group, args, name, band, bar)
        assert band < bar / 4, line
        if name in TENSORS and H != W:
            sens = rel_err(swapped[name], ref[name])
            line += ", H/W exchange %.2e" % sens
            assert sens > SENS, line
        if name in ("y", "dz") and group == "G":
            sens = rel_err(RC.conv_ref(*args, control="batch")[name], ref[name])
            line += ", batch exchange %.2e" % sens
            assert sens > SENS, line
        print(line)
    assert H != W or group == "G"      # only G may hold a square map (its control is the batch exchange)


@pytest.mark.parametrize("case", RC.D_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_stem_data_gradient_cases(case):
    ref, swapped, f32 = RC.stem_dgrad_ref(*case), RC.stem_dgrad_ref(*case, control="hw"), RC.stem_dgrad_ref(*case, dtype=F32)
    band, sens = rel_err(f32["dx"], ref["dx"]), rel_err(swapped["dx"], ref["dx"])
    print("D %s dx float32 band %.2e, H/W exchange of dout %.2e" % (case, band, sens))
    assert band < RC.TOL / 4 and sens > SENS
    B, M, H, W = case[:4]
    assert (B * H * W) % 256 != 0 and H != W


@pytest.mark.parametrize("case", RC.E_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_maxpool_cases(case):
    ref, swapped, f32 = RC.maxpool_ref(*case), RC.maxpool_ref(*case, control="hw"), RC.maxpool_ref(*case, dtype=F32)
    for name, bar in (("y", RC.TOL), ("gz", RC.TOL), ("gz_sum", RC.TOL_SUM), ("gz_cen", RC.TOL_SUM)):
        band = rel_err(f32[name], ref[name])
        line = "E %s %-6s float32 band %.2e (bar %.1e)" % (case, name, band, bar)
        assert band < bar / 4, line
        if name in ("y", "gz"):
            sens = rel_err(swapped[name], ref[name])
            line += ", H/W exchange %.2e" % sens
            assert sens > SENS, line
        print(line)


# ------------------------------------------------------------------------------------------------ the route table
def _route(r):
    """what the host functions and the restatement say of one row of RC.ROUTES, in the row's own keys"""
    from sar_amd import ops, _lib as L
    got, c = {}, r["case"]
    if r["group"] == "A":
        cin, cout, H, W = c
        Ho, Wo = RC.out_size(H, 3, 2, 1), RC.out_size(W, 3, 2, 1)
        geo = dict(B=RC.A_BATCH, Kc=cout, M=cin, H_src=Ho, W_src=Wo, H_out=H, W_out=W, KH=3, KW=3, stride=2, pad=1, transposed=True)
        got["dgrad"] = RC.dgrad_s2_route(H, W)
        got["split"] = ops.conv2d_split_applicable(epi=L.SAR_EPI_MASK, **geo)
        for arith in ("f16x3a", "bf16x6"):
            assert ops.conv2d_gemm_route(arith, epi=L.SAR_EPI_MASK, **geo) == (arith if got["split"] else None)
            # the compact aux exists on the parity classes only: a split launch of it needs the doubled image too
            assert ops.conv2d_gemm_route(arith, epi=L.SAR_EPI_ADD, aux_even_pixels=True, **geo) == (arith if got["dgrad"] == "parity" else None)
        assert ops.conv2d_gemm_route(None, epi=L.SAR_EPI_MASK, **geo) is None
    elif r["group"] == "E":
        got["tiles"] = RC.mpb_tiles(c[2], c[3])
    elif r["group"] == "F":
        cin, cout, s, H, W = c
        got["wgrad"], tile = RC.wgrad3x3_route(H, W, s)
        if "ragged" in r:
            got["ragged"] = RC.out_size(H, 3, s, 1) % tile["th"] != 0
    elif r["group"] == "G":
        cin, cout, H, W, B = c
        geo = dict(B=B, Kc=cin, M=cout, H_src=H, W_src=W, H_out=H, W_out=W, KH=3, KW=3, stride=1, pad=1)
        got["NI"], got["ntiles"] = RC.gemm_images_per_tile(B, H, W, False)
        assert RC.gemm_images_per_tile(B, H, W, True)[0] == got["NI"]      # the data gradient shares the tile the same way
        got["split"] = ops.conv2d_split_applicable(**geo)
        assert ops.conv2d_split_applicable(transposed=True, epi=L.SAR_EPI_MASK, **geo) == got["split"]
    return got


def test_route_table():
    hit = set()
    for r in RC.ROUTES:
        got = _route(r)
        want = {k: v for k, v in r.items() if k not in ("group", "case")}
        print("%s %-22s %s" % (r["group"], r["case"], got))
        assert got == want, (r, got)
        hit |= {got.get("dgrad"), got.get("wgrad")}
        if got.get("ragged"):
            hit.add(got["wgrad"] + " ragged")
        if got.get("tiles", (1, 1))[1] > 1:
            hit.add("tiles_w > 1")
        if got.get("NI", 1) > 1:
            hit.add("NI > 1")
    want = {"parity", "masked", "generic", "tiles_w > 1", "NI > 1"} | {"v%d ragged" % i for i in range(7)}
    assert want <= hit, want - hit
    # the tables and the route table name the same cases
    named = {(r["group"], r["case"]) for r in RC.ROUTES}
    assert named == ({("A", c) for c in RC.A_PARITY + RC.A_MASKED} | {("E", c) for c in RC.E_CASES} | {("F", c) for c in RC.F_ALL} |
                     {("G", c) for c in RC.G_CASES})


def test_restated_tiles_at_the_engine_shapes():
    """the restatement against what csrc/conv2d.hip's comments say of resnet18 at 256 x 256: every 3x3 layer on its variant, whole tiles"""
    for (H, s), v in {(64, 1): "v0", (32, 1): "v1", (64, 2): "v2", (16, 1): "v3", (32, 2): "v4", (8, 1): "v5", (16, 2): "v6"}.items():
        route, tile = RC.wgrad3x3_route(H, H, s)
        assert route == v and RC.out_size(H, 3, s, 1) % tile["th"] == 0, (H, s, route, tile)
    assert RC.mpb_tiles(128, 128) == (8, 1) and RC.mpb_tiles(30, 30) == (2, 1)      # the engine's and the kernel test's: tiles_w = 1
    assert RC.gemm_images_per_tile(2, 8, 8, False) == (2, 1) and RC.gemm_images_per_tile(2, 16, 16, False)[0] == 1
    # the stem at 48 x 80, 50 x 70, 64 x 40 (tests/test_gpu_resnet.py) and its tail
    assert [RC.dgrad_s2_route(*hw) for hw in ((12, 20), (6, 10), (3, 5))] == ["parity", "parity", "masked"]
    assert [RC.dgrad_s2_route(*hw) for hw in ((13, 18), (7, 9), (4, 5))] == ["masked"] * 3
    assert [RC.dgrad_s2_route(*hw) for hw in ((16, 10), (8, 5), (4, 3))] == ["parity", "masked", "masked"]
