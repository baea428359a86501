"""csrc/augment.hip between poisoned guards: x, params and out each sit inside one larger allocation whose margins hold NaN, in
front of and behind the live range (tests/util.py `guarded`).  After the launch the margins are bitwise what they were, every element
of out -- pre-filled with NaN -- has been written, and the result is still the float64 restatement's: a read of a margin would have
carried its NaN into the output."""
import numpy as np
import pytest
import torch

import augment_reference as A
from sar_amd.augment import ClipAugment
from test_gpu_augment import judge, raw_clip
from util import NAN, assert_guards_untouched, guarded

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("shape", [(3, 3, 37, 25, 2), (2, 3, 5, 32, 4)])
@pytest.mark.parametrize("crop", [True, False])
def test_guards_untouched_and_out_fully_written(shape, crop):
    from sar_amd import ops
    dev = torch.device("cuda:0")
    N, _, T, V, M = shape
    x = np.stack([raw_clip(70 + n, T=T, V=V, M=M) for n in range(N)])
    x[0, :, T - 2:] = 0                                        # trailing padding: the window ends before the allocation does
    x[-1] = 0                                                  # a null clip is written too (zeros)
    tab = ClipAugment(rot=0.3, scale=0.1, shift=0.2, crop=0.5, seed=3).table(N, 0, 0)
    tab[0, :2] = 1.0                                           # the last window the contract allows: b + Lc = L
    xv, xw = guarded(torch.from_numpy(x).reshape(1, -1), 0, NAN, dev)
    pv, pw = guarded(torch.from_numpy(tab).reshape(1, -1), 0, NAN, dev)
    ov, ow = guarded((1, x.size), 0, NAN, dev)
    assert xv.is_contiguous() and pv.is_contiguous() and ov.is_contiguous()
    got = ops.augment_clips(xv.view(shape), pv.view(N, 16), crop=crop, out=ov.view(shape))
    torch.cuda.synchronize()
    what = "augment %s crop=%s" % (shape, crop)
    assert_guards_untouched(xw, (1, x.size), NAN, what=what + " x")
    assert_guards_untouched(pw, (1, tab.size), NAN, what=what + " params")
    assert_guards_untouched(ow, (1, x.size), NAN, what=what + " out")
    assert not bool(torch.isnan(ov).any()), "%s: an element of out was not written" % what
    assert np.array_equal(xv.cpu().numpy().reshape(shape), x) and np.array_equal(pv.cpu().numpy().reshape(N, 16), tab)
    judge(got.cpu().numpy(), x, tab, crop, what)
    assert not got[-1].any()
