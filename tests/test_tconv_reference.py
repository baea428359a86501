"""CPU: the float64 restatement of TemporalConv (tests/tconv_reference.py) against torch.nn.functional.conv2d in float64 and float64
autograd, over the cases of tests/tconv_cases.py; its geometry against sar_amd.ops.tconv_geometry and sar_amd.stgcn.same_pad; and the
distance of its float32 run from float64, which has to stay below the GPU tests' TOL so that their band rule cannot hide a wrong
kernel."""
import pytest
import torch
import torch.nn.functional as F

import tconv_cases as K
import tconv_reference as R
from util import rel_err

TOL = 2e-5


def torch_conv(x, W, bias, T_out, k, s, d, pad):
    """the same layer as F.conv2d; F.pad carries the uneven padding (behind: whatever the last window still reads)"""
    T = x.shape[2]
    behind = max((T_out - 1) * s + (k - 1) * d + 1 - T - pad, 0)
    xp = F.pad(x, (0, 0, pad, behind))
    w = W[:, 0].permute(2, 1, 0).unsqueeze(-1)          # (k, C, M) -> (M, C, k, 1)
    return F.conv2d(xp, w, bias, stride=(s, 1), dilation=(d, 1))[:, :, :T_out]


@pytest.mark.parametrize("case", K.CASES + [K.SLICE], ids=K.case_id)
def test_restatement_equals_conv2d_and_autograd_in_float64(case):
    N, C, M, T, V, k, d, s, padding = case
    (x, W, bias, dout), r64, _ = K.reference(case)
    T_out, pad = R.geometry(T, k, s, d, padding)
    xa, Wa, ba = (t.clone().requires_grad_(True) for t in (x, W, bias))
    out = torch_conv(xa, Wa, ba, T_out, k, s, d, pad)
    assert out.shape == r64["out"].shape == (N, M, T_out, V)
    out.backward(dout)
    for name, want in (("out", out.detach()), ("dx", xa.grad), ("dW", Wa.grad), ("dbias", ba.grad)):
        e = rel_err(r64[name], want)
        assert e < 1e-12, "%s: %.3e" % (name, e)


@pytest.mark.parametrize("case", K.CASES + [K.SLICE], ids=K.case_id)
def test_float32_restatement_is_within_tol_of_float64(case):
    _, r64, r32 = K.reference(case)
    for name in K.QUANTITIES:
        e = rel_err(r32[name], r64[name])
        assert e < TOL, "%s: the float32 restatement is %.3e from float64" % (name, e)


def test_geometry_restates_both_padding_rules():
    from sar_amd import ops
    from sar_amd.stgcn import same_pad
    for T in range(1, 40):
        for s in (1, 2):
            assert R.geometry(T, 9, s, 1, "same") == same_pad(T, 9, s)[:2] == ops.tconv_geometry(T, 9, s, 1, "same")
            for k in range(1, 10):
                for d in (1, 2, 3, 8):
                    T_out, pad = R.geometry(T, k, s, d, "same")
                    assert (T_out, pad) == ops.tconv_geometry(T, k, s, d, "same") and T_out == -(-T // s) and 0 <= pad <= (k - 1) * d
                    for p in (0, 1, (k - 1) * d // 2, (k - 1) * d):
                        if T + 2 * p - d * (k - 1) - 1 >= 0:
                            want = F.conv2d(torch.zeros(1, 1, T, 1), torch.zeros(1, 1, k, 1), stride=(s, 1), dilation=(d, 1), padding=(p, 0)).shape[2]
                            assert R.geometry(T, k, s, d, p) == (want, p) == ops.tconv_geometry(T, k, s, d, p)
    with pytest.raises(ValueError):
        ops.tconv_geometry(3, 9, 1, 1, 0)                # no output frame
    with pytest.raises(ValueError):
        ops.tconv_geometry(3, 9, 1, 1, "valid")


def test_case_list_reaches_what_it_says():
    """SAME (3, 4) at the stride-2 ST-GCN shape, a dilation beyond T, both parities of T at stride 2"""
    assert R.geometry(12, 9, 2, 1, "same") == (6, 3) and (6 - 1) * 2 + 8 + 1 - 12 - 3 == 4
    assert R.geometry(5, 3, 1, 8, "same") == (5, 8) and R.geometry(1, 5, 1, 4, "same") == (1, 8)
    assert len(R.pairs(1, 1, 5, 1, 4, 8)) == 1             # of 5 taps one reads a frame
    assert {c[3] % 2 for c in K.CASES if c[7] == 2 and c[5] > 1} == {0, 1}
