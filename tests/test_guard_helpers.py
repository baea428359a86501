"""The guard-band helpers of tests/util.py on the CPU: the geometry they promise, and that one flipped element in any margin is seen."""
import pytest
import torch

from util import (MASK_FILL, NAN, SENTINEL, GuardedSlabs, Launch, assert_cn8_guards_untouched, assert_cn8_pad_lanes_zero,
                  assert_flat_guards_untouched, assert_guards_untouched, cn8_mask_bytes, cn8_units, cn8_values, guarded, guarded_cn8,
                  guarded_cn8_mask, guarded_flat)

CPU = torch.device("cpu")
C, N = 5, 12


@pytest.mark.parametrize("pad", [0, 4, 7])
def test_view_geometry(pad):
    src = torch.arange(C * N, dtype=torch.float32).view(C, N)
    view, whole = guarded(src, pad, NAN, CPU)
    assert whole.shape == (4 + C + 2, N + pad) and whole.is_contiguous()
    assert view.shape == (C, N) and view.stride(0) == N + pad and view.stride(1) == 1
    assert view.data_ptr() % 16 == 0 and view.data_ptr() == whole.data_ptr() + 4 * 4 * (N + pad)
    assert torch.equal(view, src)
    assert_guards_untouched(whole, (C, N), NAN)
    out, owhole = guarded((C, N), pad, SENTINEL, CPU)
    assert bool((owhole == SENTINEL).all()) and out.stride(0) == N + pad and out.data_ptr() % 16 == 0


@pytest.mark.parametrize("fill,dtype,other", [(SENTINEL, torch.float32, 1.0), (NAN, torch.float32, 0.0), (MASK_FILL, torch.uint8, 0)])
@pytest.mark.parametrize("margin", ["front rows", "back rows", "pad of a live row", "pad of the last live row"])
def test_one_flipped_element_in_any_margin_is_seen(fill, dtype, other, margin):
    pad = 7
    view, whole = guarded((C, N), pad, fill, CPU, dtype=dtype)
    view.fill_(3)                                        # the live region may hold anything
    assert_guards_untouched(whole, (C, N), fill)
    r, c = {"front rows": (3, N - 1), "back rows": (4 + C, 0), "pad of a live row": (4 + 1, N),
            "pad of the last live row": (4 + C - 1, N + pad - 1)}[margin]
    whole[r, c] = other
    with pytest.raises(AssertionError, match="overwritten"):
        assert_guards_untouched(whole, (C, N), fill)


def test_nan_fill_equals_itself_and_no_other_nan():
    view, whole = guarded((C, N), 4, NAN, CPU)
    assert_guards_untouched(whole, (C, N), NAN)
    whole.view(torch.int32)[0, 0] ^= 1                   # still a NaN, another bit pattern
    assert bool(torch.isnan(whole[0, 0]))
    with pytest.raises(AssertionError, match="overwritten"):
        assert_guards_untouched(whole, (C, N), NAN)


def test_flat_range():
    src = torch.arange(10, dtype=torch.float32)
    view, whole = guarded_flat(src, SENTINEL, CPU)
    assert whole.numel() == 26 and view.data_ptr() == whole.data_ptr() + 32 and torch.equal(view, src)
    assert_flat_guards_untouched(whole, 10, SENTINEL)
    for i in (7, 18, 0, 25):
        v, w = guarded_flat(10, NAN, CPU)
        assert_flat_guards_untouched(w, 10, NAN)
        w[i] = 0.0
        with pytest.raises(AssertionError, match="overwritten"):
            assert_flat_guards_untouched(w, 10, NAN)
    # float64 ranges (the spline pieces of the radar up-sampling) and int32 ranges (edge lists): NaN margins compare by bit pattern too
    for dtype, fill, other in ((torch.float64, NAN, 0.0), (torch.float64, SENTINEL, 1.0), (torch.int32, 1 << 30, 0)):
        v, w = guarded_flat(10, fill, CPU, dtype=dtype)
        assert v.data_ptr() % 16 == 0
        v.fill_(3)
        assert_flat_guards_untouched(w, 10, fill)
        w[18 if dtype == torch.int32 else 3] = other
        with pytest.raises(AssertionError, match="overwritten"):
            assert_flat_guards_untouched(w, 10, fill)
    with pytest.raises(AssertionError):
        guarded_flat(10, SENTINEL, CPU, k=6)


# ---- the CN8 helpers (planes of 16-byte units; tests/test_gpu_cn8_guard_bands.py)
C8, N8 = 20, 13        # 3 planes, 4 pad lanes in the last one


def _src8(C=C8, n=N8):
    return (torch.arange(C * n, dtype=torch.float32).view(C, n) % 97 - 40).bfloat16().float() + 1      # bf16-exact, no zeros


@pytest.mark.parametrize("pad", [0, 1, 67])
def test_cn8_view_geometry(pad):
    src = _src8()
    view, whole = guarded_cn8(src, pad, NAN, CPU)
    assert whole.dtype == torch.bfloat16 and whole.shape == (2 + 3 + 2, N8 + pad, 8) and whole.is_contiguous()
    assert view.shape == (3, N8 + pad, 8) and view.is_contiguous() and view.data_ptr() % 16 == 0
    assert view.data_ptr() == whole.data_ptr() + 2 * (N8 + pad) * 16
    assert torch.equal(cn8_values(view[:, :N8], C8), src)
    assert bool((view[2, :N8, C8 % 8:] == 0).all())                      # an input's pad lanes are zero
    assert_cn8_pad_lanes_zero(view, C8, N8)
    assert_cn8_guards_untouched(whole, C8, N8, NAN)
    out, owhole = guarded_cn8((C8, N8), pad, SENTINEL, CPU)
    assert bool((owhole == SENTINEL).all()) and out.shape == (3, N8 + pad, 8) and out.is_contiguous()
    assert_cn8_guards_untouched(owhole, C8, N8, SENTINEL)
    with pytest.raises(AssertionError, match="pad lane"):                  # an output's pad lanes start as the sentinel
        assert_cn8_pad_lanes_zero(out, C8, N8)


@pytest.mark.parametrize("fill,other", [(SENTINEL, 1.0), (NAN, 0.0)])
@pytest.mark.parametrize("margin", ["front plane", "back plane", "pad column", "pad column of the last plane"])
def test_cn8_one_flipped_guard_unit_is_seen(fill, other, margin):
    pad = 67
    view, whole = guarded_cn8((C8, N8), pad, fill, CPU)
    view[:, :N8] = 3                                                     # the live region may hold anything
    assert_cn8_guards_untouched(whole, C8, N8, fill)
    g, c, j = {"front plane": (1, N8 - 1, 0), "back plane": (2 + 3, 0, 7), "pad column": (2 + 1, N8, 3),
               "pad column of the last plane": (2 + 2, N8 + pad - 1, 5)}[margin]
    whole[g, c, j] = other
    with pytest.raises(AssertionError, match=r"plane %d, column %d\), lane %d .*overwritten.*\(1 elements" % (g - 2, c, j)):
        assert_cn8_guards_untouched(whole, C8, N8, fill)


def test_cn8_flipped_pad_lane_is_seen():
    view, whole = guarded_cn8(_src8(), 1, NAN, CPU)
    assert_cn8_pad_lanes_zero(view, C8, N8, "x")
    view[2, 5, 6] = 0.5                                                  # channel 22 of a 20-channel tensor
    with pytest.raises(AssertionError, match="pad lane 6 .channel 22 >= 20. of column 5"):
        assert_cn8_pad_lanes_zero(view, C8, N8, "x")
    view[2, 5, 6] = -0.0                                                 # a zero of either sign is a zero
    assert_cn8_pad_lanes_zero(view, C8, N8, "x")
    view[1, 5, 6] = float("inf")                                         # a live lane of a full plane is no pad lane
    assert_cn8_pad_lanes_zero(view, C8, N8, "x")
    full, _ = guarded_cn8((16, N8), 1, SENTINEL, CPU)                   # C % 8 == 0: there are none
    assert_cn8_pad_lanes_zero(full, 16, N8, "x")


def test_cn8_nan_fill_equals_itself_and_no_other_nan():
    view, whole = guarded_cn8((C8, N8), 1, NAN, CPU)
    assert bool(torch.isnan(whole).all())                                # the bf16 quiet NaN survives torch.full
    assert_cn8_guards_untouched(whole, C8, N8, NAN)
    whole.view(torch.int16)[0, 0, 0] ^= 1                                # still a NaN, another bit pattern
    assert bool(torch.isnan(whole[0, 0, 0]))
    with pytest.raises(AssertionError, match="overwritten"):
        assert_cn8_guards_untouched(whole, C8, N8, NAN)


@pytest.mark.parametrize("C", [3, 8, 20, 64])
def test_cn8_host_layout_writer_round_trips_against_the_definition(C):
    n = 29
    x = torch.randn(C, n, generator=torch.Generator().manual_seed(C)).bfloat16().float()
    units = cn8_units(x)
    G = (C + 7) // 8
    assert units.shape == (G, n, 8) and units.dtype == torch.bfloat16
    for c in range(G * 8):                                               # unit (g, col)[j] = channel 8 g + j, zero beyond C
        want = x[c] if c < C else torch.zeros(n)
        assert torch.equal(units[c // 8, :, c % 8].float(), want), c
    assert torch.equal(cn8_values(units, C), x)
    with pytest.raises(AssertionError, match="representable"):
        cn8_units(torch.full((C, n), 1.0 + 2.0 ** -12))


def test_cn8_mask_bytes_and_their_guards():
    keep = _src8() % 3 > 0
    mb = cn8_mask_bytes(keep)
    assert mb.shape == (3, N8) and mb.dtype == torch.uint8
    for c in range(24):
        assert torch.equal(((mb[c // 8] >> (c % 8)) & 1).bool(), keep[c] if c < C8 else torch.zeros(N8, dtype=torch.bool)), c
    view, whole = guarded_cn8_mask(mb, 67, CPU)
    assert whole.shape == (2 + 3 + 2, N8 + 67) and view.shape == (3, N8 + 67) and view.is_contiguous()
    assert torch.equal(view[:, :N8], mb)
    assert_guards_untouched(whole, (3, N8), MASK_FILL, 2, 2)
    for r, c in ((1, 0), (5, N8 - 1), (3, N8), (4, N8 + 66)):
        _, w = guarded_cn8_mask((3, N8), 67, CPU)
        w[r, c] = 0
        with pytest.raises(AssertionError, match="overwritten"):
            assert_guards_untouched(w, (3, N8), MASK_FILL, 2, 2)


# ---- the launch record and the guarded slabs of the weight gradients (tests/test_gpu_split_guard_bands.py)

def _cpu_reduce(slab, nsplit, n, out):
    out[:n] = slab[:nsplit, :n].sum(0)


def test_guarded_slabs_geometry_and_reduction():
    nsplit, n = 3, 10
    out = torch.zeros(n)
    batch = GuardedSlabs(CPU, _cpu_reduce)
    slab = batch.slab(out, nsplit, n)
    view, whole, _, _ = batch.items[0]
    assert slab.shape == (nsplit, n) and slab.is_contiguous() and slab.data_ptr() == whole.data_ptr() + 32 and slab.data_ptr() % 16 == 0
    assert whole.numel() == nsplit * n + 16 and bool(torch.isnan(slab).all()) and bool((whole[:8] == SENTINEL).all()) and bool((whole[-8:] == SENTINEL).all())
    batch.check_guards()
    batch.check_nothing_written()
    with pytest.raises(AssertionError, match="never written"):
        batch.check_finite()
    slab.copy_(torch.arange(nsplit * n, dtype=torch.float32).view(nsplit, n))
    batch.add(slab, nsplit, n, out)
    assert torch.equal(out, torch.arange(n, dtype=torch.float32) * 3 + 30)
    batch.check_finite()
    batch.check_guards()
    with pytest.raises(AssertionError, match="written by a rejected call"):
        batch.check_nothing_written()
    with pytest.raises(AssertionError, match="not a slab of this batch"):
        batch.add(torch.zeros(nsplit, n), nsplit, n, out)


@pytest.mark.parametrize("where", ["one element no workgroup wrote", "one element past the last slab", "one element in front of the first slab"])
def test_guarded_slabs_see_a_missing_and_a_stray_write(where):
    nsplit, n = 4, 6
    out = torch.zeros(n)
    batch = GuardedSlabs(CPU, _cpu_reduce)
    slab = batch.slab(out, nsplit, n)
    slab.fill_(1.0)
    whole = batch.items[0][1]
    if where == "one element no workgroup wrote":
        slab[2, 5] = NAN
        batch.add(slab, nsplit, n, out)
        batch.check_guards()
        assert not bool(torch.isfinite(out).all())                        # it reaches the reduced gradient
        with pytest.raises(AssertionError, match="element 5 of slab 2 of a .4, 6. slab buffer was never written"):
            batch.check_finite()
        return
    whole[8 + nsplit * n if where == "one element past the last slab" else 7] = 0.0
    batch.check_finite()
    with pytest.raises(AssertionError, match="overwritten"):
        batch.check_guards()


def test_launch_record_on_the_cpu():
    class Wide(Launch):
        IN_BACK = 16
    g = Wide(CPU, 7)
    x = g.inp(torch.ones(C, N))
    assert x.stride(0) == N + 7 and x.storage_offset() == 4 * (N + 7) and x.untyped_storage().nbytes() == 4 * (4 + C + 16) * (N + 7)
    out, flat = g.out("out", C, N), g.flat("flat", 9)
    out.fill_(2.0)
    flat.fill_(1.0)
    g.ref("relative to max |want|", out, torch.full((C, N), 2.0 + 1e-5), 1e-5)
    g.ref("relative to a stated scale", out, torch.full((C, N), 2.0 + 1e-3), 1e-5, scale=1000.0)
    g.ref("bitwise", lambda: flat, torch.ones(9), 0)
    g.check()
    g.ref("too far", out, torch.full((C, N), 2.1), 1e-5)
    with pytest.raises(AssertionError, match="too far"):
        g.check()
    g.refs.pop()
    out[0, 0] = NAN
    with pytest.raises(AssertionError, match="not finite"):
        g.check()
    out[0, 0] = 2.0
    g.outs["out"][1][4 + C, 0] = 0.0                                       # the first guard row behind the output
    with pytest.raises(AssertionError, match="overwritten"):
        g.check()
    with pytest.raises(AssertionError, match="written by a rejected call"):
        g.check_nothing_written()
    slabs = g.slab_batch(_cpu_reduce)
    assert g.slabs == [slabs]


# ---- kept inputs, int64 label ranges, in-place buffers and outputs whose specified result is NaN (tests/test_gpu_head_edges.py)

def test_kept_inputs_and_label_ranges_on_the_cpu():
    class Kept(Launch):
        KEEP_INPUTS = True
    g = Kept(CPU, 7)
    x = g.inp(torch.ones(C, N))
    labels = g.flat_in(torch.arange(6, dtype=torch.int64).view(2, 3), fill=1 << 40)
    name, whole, copy = g.ins[1]
    assert len(g.ins) == 2 and labels.dtype == torch.int64 and labels.shape == (2, 3) and labels.data_ptr() % 16 == 0
    assert whole.numel() == 6 + 16 and bool((whole[:8] == 1 << 40).all()) and bool((whole[-8:] == 1 << 40).all())
    assert torch.equal(labels.reshape(-1), torch.arange(6)) and copy.data_ptr() != whole.data_ptr()
    cell = g.flat_in(torch.tensor([0.1]))
    assert cell.shape == (1,) and bool(torch.isnan(g.ins[2][1][:8]).all())
    g.check()
    for t, where in ((labels, (1, 2)), (x, (0, 0)), (g.ins[1][1], 3), (g.ins[0][1], (0, 0))):   # a live element, a margin: each is seen
        old = t[where].clone()
        t[where] = 77
        with pytest.raises(AssertionError, match="of an input's allocation were modified"):
            g.check()
        t[where] = old
        g.check()
    assert not Launch(CPU, 0).ins and Launch(CPU, 0).inp(torch.ones(C, N)).shape == (C, N) and not Launch.KEEP_INPUTS


def test_in_place_buffers_and_nan_results_on_the_cpu():
    g = Launch(CPU, 0)
    w = g.flat("w", torch.arange(5, dtype=torch.float32))
    assert torch.equal(w, torch.arange(5.0)) and bool((g.flats["w"][1][:8] == SENTINEL).all())
    loss = g.flat("loss", 1)
    loss[0] = NAN
    with pytest.raises(AssertionError, match="loss .pad 0.: not finite"):
        g.check()
    g.nan_ok = {"loss"}
    g.check()
    w[4] = float("inf")                                  # the exemption is by name
    with pytest.raises(AssertionError, match="w .pad 0.: not finite"):
        g.check()
    w[4] = 4.0
    g.flats["loss"][1][0] = 0.0                          # and does not cover the guards
    with pytest.raises(AssertionError, match="overwritten"):
        g.check()
