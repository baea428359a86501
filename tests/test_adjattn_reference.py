"""CPU: tests/adjattn_reference.py, the float64 oracle of the AdaptiveAdjacency tests, is pinned here against torch autograd of the
literal formulation (conv -> permute / view -> matmul -> softmax over axis -2, one subset at a time), every case of tests/adjattn_cases.py
is shown to have logits that are neither flat nor saturated, and the reason theta has no bias is pinned: the softmax over v removes it."""
import pytest
import torch

import adjattn_cases as K
import adjattn_reference as R
from util import rel_err


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_hand_written_backward_is_autograd_of_the_literal_formulation(case):
    (x, A, tk, pk, pb, dA_eff), r64, _ = K.reference(case)
    leaves = [t.clone().requires_grad_() for t in (x, A, tk, pk, pb)]
    lit = R.literal(*leaves)
    want = torch.autograd.grad(lit, leaves, dA_eff)
    assert rel_err(r64["A_eff"], lit) < 1e-12
    for name, w in zip(("dx", "dA", "dtheta_kernel", "dphi_kernel", "dphi_bias"), want):
        if case[3] == 1 and name != "dA":
            assert not bool(w.abs().gt(1e-12).any())        # (autograd's own zeros; the hand-written ones are exact, below)
        else:
            assert rel_err(r64[name], w) < 1e-12, name


@pytest.mark.parametrize("case", [c for c in K.CASES if c[3] > 1], ids=K.case_id)
def test_logits_are_neither_flat_nor_saturated(case):
    _, r64, _ = K.reference(case)
    assert abs(R.column_std(r64["S"]) - K.LOGIT_STD) < 1e-9
    assert r64["S"].abs().max().item() <= 40
    assert (r64["P"].sum(dim=2) - 1).abs().max().item() < 1e-12


def test_float32_restatement_is_close_to_float64():
    worst = max(rel_err(r32[q], r64[q]) for case in K.CASES for _, r64, r32 in [K.reference(case)] for q in K.QUANTITIES)
    print("float32 restatement from float64, worst quantity over the cases: %.2e" % worst)
    assert worst < 2e-5


def test_one_vertex_gives_p_one_and_zero_gradients():
    case = K.LISTED[4]
    assert case[3] == 1
    (x, A, tk, pk, pb, dA_eff), r64, r32 = K.reference(case)
    for r in (r64, r32):
        assert torch.equal(r["P"], torch.ones_like(r["P"]))
        for name in ("dx", "dtheta_kernel", "dphi_kernel", "dphi_bias", "dS", "dtheta", "dphi"):
            assert not bool(r[name].any()), name
        assert torch.equal(r["dA"], dA_eff.to(r["dA"].dtype).sum(dim=0))


@pytest.mark.parametrize("case", [K.LISTED[0], K.LISTED[3], K.LISTED[5]], ids=K.case_id)
def test_a_bias_on_theta_has_no_gradient(case):
    """b_e adds b_e sum_t phi[e, t, w] to every v of column w, and the softmax over v removes it"""
    x, A, tk, pk, pb, dA_eff = K.make_case(case)
    tb = (0.1 * torch.randn(tk.shape[1], generator=torch.Generator().manual_seed(3), dtype=torch.float64)).requires_grad_()
    pbl = pb.clone().requires_grad_()
    gt, gp = torch.autograd.grad(R.literal(x, A, tk, pk, pbl, theta_bias=tb), (tb, pbl), dA_eff)
    assert gp.norm().item() > 0 and gt.norm().item() < 1e-12 * gp.norm().item()


def test_channel_k_ce_plus_e_belongs_to_subset_k():
    """zeroing subset 1's columns of theta.kernel makes subset 1's logits zero (P uniform) and leaves the other subsets' alone"""
    case = K.LISTED[0]
    x, A, tk, pk, pb, _ = K.make_case(case)
    V, Ce = case[3], case[5]
    tk0 = tk.clone()
    tk0[:, Ce:2 * Ce] = 0
    a, b = R.forward(x, A, tk, pk, pb)[1]["P"], R.forward(x, A, tk0, pk, pb)[1]["P"]
    assert torch.equal(a[:, 0], b[:, 0]) and torch.equal(a[:, 2], b[:, 2])
    assert (b[:, 1] - 1.0 / V).abs().max().item() < 1e-15
