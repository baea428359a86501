"""The guard-band helpers of tests/util.py on the CPU: the geometry they promise, and that one flipped element in any margin is seen."""
import pytest
import torch

from util import MASK_FILL, NAN, SENTINEL, assert_flat_guards_untouched, assert_guards_untouched, guarded, guarded_flat

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
    with pytest.raises(AssertionError):
        guarded_flat(10, SENTINEL, CPU, k=6)
