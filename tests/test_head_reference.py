"""tests/head_reference.py pinned on the CPU, at every shape and on the very inputs tests/test_gpu_head_edges.py launches
(tests/head_cases.py), two ways:

a. against torch float64 (cross_entropy, batch_norm in training and eval mode with its moving statistics, autograd, permute,
   as_strided) and the oracles' optimizer steps, to 1e-12;
b. sensitivity: on those inputs each reference differs from a named near miss by at least 100x the bar the GPU file asserts for
   the case, so a kernel that computes the near miss cannot pass."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import head_cases as H
import head_reference as R
from oracle import resnet as ORES
from oracle import stgcn as O

BAR = 1e-12
F32, F64 = np.float32, np.float64
t64 = lambda a: torch.from_numpy(np.asarray(a, dtype=F64))


def close(got, want, what=""):
    got, want = np.asarray(got, dtype=F64), want.detach().numpy() if torch.is_tensor(want) else np.asarray(want, dtype=F64)
    assert got.shape == want.shape, "%s: shape %s against %s" % (what, got.shape, want.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isinf(got), np.isinf(want)), what
    fin = np.isfinite(want)
    e = H.rel(got[fin], want[fin]) if fin.any() else 0.0
    assert e < BAR, "%s: %.3e" % (what, e)


def far(a, b, bar, what):
    """the near miss `a` is at least 100 bars from the reference `b` (a NaN where the reference is finite is as far as can be)"""
    a, b = np.asarray(a, dtype=F64), np.asarray(b, dtype=F64)
    e = H.rel(a, b)
    assert not e < 100 * bar, "%s: the near miss is only %.3e from the reference (bar %.1e)" % (what, e, bar)


# ---------------------------------------------------------------------------------------------------- a. pins
@pytest.mark.parametrize("TV", H.POOL_TV)
def test_pooling_against_autograd(TV):
    for N in H.POOL_N:
        for Mp in H.POOL_MP:
            for C in H.POOL_C:
                y, dfeat = H.pool_inputs(TV, N, Mp, C)
                yt = t64(y).requires_grad_(True)
                feat = yt.view(C, N * Mp, TV).mean(2).t().reshape(N, Mp, C).mean(1)        # tests/test_gpu_stgcn_kernels.py's head
                close(R.pool_fwd(y, N, Mp, TV), feat, "feat")
                close(R.pool_bwd(dfeat, N, Mp, TV), torch.autograd.grad(feat, yt, t64(dfeat))[0], "dy")
                if Mp == 2:                                                                 # b. a mean over TV only is twice as large
                    far(np.asarray(y, F64).reshape(C, N, Mp * TV).sum(2).T / TV, R.pool_fwd(y, N, Mp, TV), H.TOL, "pooling by TV only")
                    far(np.repeat((np.asarray(dfeat, F64).T / TV)[:, :, None], Mp * TV, 2).reshape(C, -1), R.pool_bwd(dfeat, N, Mp, TV), H.TOL,
                        "pool backward by TV only")


@pytest.mark.parametrize("C", H.FC_C)
def test_dense_layer_against_autograd(C):
    pairs = [(K, N) for K in H.FC_K for N in H.FC_N] + [(K, N) for c, K in H.FC_BWD if c == C for N in H.FC_N]
    for K, N in pairs:
        c = H.fc_inputs(C, K, N)
        feat, W, b = (t64(c[k]).requires_grad_(True) for k in ("feat", "W", "bias"))
        out = feat @ W + b
        close(R.fc_fwd(c["feat"], c["W"], c["bias"]), out, "logits")
        close(R.fc_fwd(c["feat"], c["W"], None), feat @ W, "logits without bias")
        gf, gW, gb = torch.autograd.grad(out, (feat, W, b), t64(c["dlogits"]))
        dW, db, dfeat = R.fc_bwd(c["feat"], c["W"], c["dlogits"])
        close(dW, gW, "dW"), close(db, gb, "dbias"), close(dfeat, gf, "dfeat")
        far(R.fc_fwd(c["feat"], c["W"], None), R.fc_fwd(c["feat"], c["W"], c["bias"]), H.TOL, "logits with the bias dropped")


@pytest.mark.parametrize("regime,K", [(r, K) for r in H.CE_REGIMES for K in H.CE_K if H.ce_inputs(r, 1, K) is not None])
def test_cross_entropy_against_torch(regime, K):
    for N in H.CE_N:
        x, labels = H.ce_inputs(regime, N, K)
        xt = t64(x).requires_grad_(True)
        loss = F.cross_entropy(xt, torch.from_numpy(labels), reduction="sum") * H.CE_INV
        l, d, p = R.softmax_ce(x, labels, H.CE_INV)
        close(l, loss, "loss"), close(d, torch.autograd.grad(loss, xt)[0], "dlogits"), close(p, torch.softmax(xt, 1), "probs")
        close(l, O.loss_fn(t64(x), torch.from_numpy(labels), 16), "the oracle's loss")
        assert np.isfinite(l) and np.isfinite(d).all() and np.isfinite(p).all()
        if regime == "c":
            assert abs(l / (N * H.CE_INV) - 200) < 1e-9 and np.count_nonzero(R.softmax_ce(x, labels, H.CE_INV, dt=F32)[2]) == N


@pytest.mark.parametrize("K", H.CE_BAD_K)
def test_cross_entropy_labels_without_a_class(K):
    x, labels, bad = H.ce_bad_inputs(K)
    l, d, p = R.softmax_ce(x, bad, H.CE_INV)
    l0, d0, p0 = R.softmax_ce(x, labels, H.CE_INV)
    assert np.isnan(l) and np.isnan(d[[1, 3]]).all() and np.array_equal(d[[0, 2, 4]], d0[[0, 2, 4]]) and np.array_equal(p, p0)


@pytest.mark.parametrize("n", H.OPT_N)
def test_optimizer_steps_against_the_oracles(n):
    w0, gs = H.nesterov_inputs(n)
    p, vel = {"w": t64(w0).clone()}, {}
    for g, (w, v) in zip(gs, H.run_nesterov(n, F64)):
        O.sgd_nesterov_step(p, {"w": t64(g)}, vel, H.SGD_LR, H.SGD_MOM)
        close(w, p["w"], "nesterov w"), close(v, vel["w"], "nesterov v")
    for t0 in (0, 999):
        w0, m0, v0, gs, t = H.adam_inputs(n, t0)
        p, st = {"w": t64(w0).clone()}, {"t": t0, "m.w": t64(m0).clone(), "v.w": t64(v0).clone()}
        for g, (w, m, v) in zip(gs, H.run_adam(n, t0, F64)):
            ORES.adam_step(p, {"w": t64(g)}, st, H.ADAM_LR, (H.ADAM_B1, H.ADAM_B2), H.ADAM_EPS)
            close(w, p["w"], "adam w"), close(m, st["m.w"], "adam m"), close(v, st["v.w"], "adam v")
        assert st["t"] == t0 + len(gs)
        if n > 1:                                        # g = 0 throughout: no update, and no 0 / 0
            assert all(s[0][0] == w0[0] for s in H.run_adam(n, t0, F64)) and all(s[0][0] == w0[0] for s in H.run_adam(n, t0, F32))


@pytest.mark.parametrize("regimes,nparts", H.BN_CASES)
def test_bn_finalize_against_torch_batch_norm(regimes, nparts):
    """on the values whose sums the GPU file's partials are, with the partials left in float64: torch's batch_norm gives the
    statistics, the affine and the moving update.  The variance is held to 1e-9 absolute and not to 1e-12: E x^2 - mean^2 at
    |mean| = 1000 cancels six of float64's sixteen digits, in any evaluation from (sum, sum of squares)."""
    C = len(regimes)
    c = H.bn_case(regimes, nparts)
    vals = np.stack([np.full(c["count"], 3.7 if g == "one" else 1000.37) if g in ("const", "one") else
                     H.rng("bn", g, nparts).standard_normal((nparts, H.BN_CHUNK)).reshape(-1) + (1000.0 if g == "far" else 0.0)
                     for g in regimes])
    n = vals.shape[1]
    exact = np.stack([vals.reshape(C, nparts, -1).sum(2), (vals * vals).reshape(C, nparts, -1).sum(2)], axis=2)
    for g, rounded, ex in zip(regimes, c["partials"], exact):
        assert g == "const" or np.array_equal(rounded, ex.astype(F32)), "the pin runs on other values than the GPU file's partials"
    for unbiased in (0, 1):
        got = R.bn_finalize(exact, n, H.BN_EPS, H.BN_MOM, unbiased, c["gamma"], c["beta"], c["rm"], c["rv"])
        x = t64(vals.T.copy())                                                       # (n, C)
        rm, rv = t64(c["rm"]).clone(), t64(c["rv"]).clone()
        if n > 1:
            y = F.batch_norm(x, rm, rv, t64(c["gamma"]), t64(c["beta"]), True, 1 - H.BN_MOM, H.BN_EPS)   # torch: unbiased moving variance
            mean, var = x.mean(0), x.var(0, unbiased=False)
            want_rv = rv if unbiased else H.BN_MOM * t64(c["rv"]) + (1 - H.BN_MOM) * var
            assert H.rel(got["mean"], mean.numpy()) < BAR and H.rel(got["running_mean"], rm.numpy()) < BAR
            assert np.abs(got["var"] - var.numpy()).max() < 1e-9 and np.abs(got["running_var"] - want_rv.numpy()).max() < 1e-9
            xs = x.numpy() * got["scale"]                                           # (x scale + shift cancels down from |x scale|)
            assert np.abs(xs + got["shift"] - y.numpy()).max() < 1e-12 * np.abs(xs).max()
        else:
            assert got["var"][0] == 0 and got["running_var"][0] == H.BN_MOM * F64(c["rv"][0]) and got["mean"][0] == 3.7
        # eval mode from the updated moving statistics
        sc, sh = R.bn_eval_affine(c["gamma"], c["beta"], got["running_mean"], got["running_var"], H.BN_EPS)
        ye = F.batch_norm(x, t64(got["running_mean"]), t64(got["running_var"]), t64(c["gamma"]), t64(c["beta"]), False, 0.0, H.BN_EPS)
        assert H.rel(x.numpy() * sc + sh, ye.numpy()) < BAR


@pytest.mark.parametrize("C", H.BN_EVAL_C)
def test_bn_eval_affine_against_torch(C):
    c = H.bn_eval_inputs(C)
    x = t64(H.randn(H.rng("x", C), 4, C))
    sc, sh = R.bn_eval_affine(c["gamma"], c["beta"], c["rm"], c["rv"], H.BN_EPS)
    close(x.numpy() * sc + sh, F.batch_norm(x, t64(c["rm"]), t64(c["rv"]), t64(c["gamma"]), t64(c["beta"]), False, 0.0, H.BN_EPS), "eval")
    sc1, sh1 = R.bn_eval_affine(None, None, c["rm"], c["rv"], H.BN_EPS)
    close(x.numpy() * sc1 + sh1, F.batch_norm(x, t64(c["rm"]), t64(c["rv"]), None, None, False, 0.0, H.BN_EPS), "eval without affine")
    assert sc1[0] == 1 / np.sqrt(F64(F32(H.BN_EPS)) * 0 + H.BN_EPS)                  # moving variance 0: rstd = 1 / sqrt(eps)


@pytest.mark.parametrize("nparts", H.BN_NPARTS)
@pytest.mark.parametrize("centered", [0, 1])
def test_bn_backward_finalisation_against_autograd(nparts, centered):
    """float64 partials (nothing rounded): dgamma, dbeta and dx = k1 dz + k2 x + k3 are autograd's through a training-mode batch_norm"""
    c = H.bnb_case(nparts, centered, F64)
    C = H.BNB_C
    x = t64(c["x"].reshape(C, -1).T.copy()).requires_grad_(True)
    gam, bet = t64(c["gamma"]).requires_grad_(True), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = F.batch_norm(x, None, None, gam, bet, True, 0.1, H.BN_EPS)
    dz = t64(c["dz"].reshape(C, -1).T.copy())
    gx, gg, gb = torch.autograd.grad(y, (x, gam, bet), dz)
    got = R.bn_bwd_finalize(c["s1"], c["s2"], centered, c["count"], c["gamma"], c["mean"], c["rstd"])
    assert H.rel(got["dgamma"], gg.numpy()) < BAR and H.rel(got["dbeta"], gb.numpy()) < BAR
    assert H.rel(dz.numpy() * got["k1"] + x.detach().numpy() * got["k2"] + got["k3"], gx.numpy()) < BAR
    # b. `centered` exchanged, on the float32 partials the GPU file passes
    c32 = H.bnb_case(nparts, centered)
    ref = R.bn_bwd_finalize(c32["s1"], c32["s2"], centered, c32["count"], c32["gamma"], c32["mean"], c32["rstd"])
    wrong = R.bn_bwd_finalize(c32["s1"], c32["s2"], 1 - centered, c32["count"], c32["gamma"], c32["mean"], c32["rstd"])
    for k in ("dgamma", "k2", "k3"):
        far(wrong[k], ref[k], H.TOL, "centered exchanged: " + k)


@pytest.mark.parametrize("batch,Rr,Cc", H.TRANSPOSE)
def test_transpose_against_torch(batch, Rr, Cc):
    x = H.randn(H.rng("tr", batch, Rr, Cc), batch, Rr, Cc)
    assert np.array_equal(R.transpose(x, batch, Rr, Cc), torch.from_numpy(x).permute(0, 2, 1).contiguous().view(-1).numpy())


@pytest.mark.parametrize("case", H.PERMUTE3, ids=[c[0] for c in H.PERMUTE3])
def test_permute3_against_torch(case):
    what, n, d0, d1, d2, s0, s1, s2 = case
    src = np.arange(n, dtype=F32)
    want = torch.as_strided(torch.from_numpy(src), (d0, d1, d2), (s0, s1, s2)).contiguous().view(-1).numpy()
    assert np.array_equal(R.permute3(src, d0, d1, d2, s0, s1, s2), want)
    t = torch.from_numpy(src)
    if what.startswith("models/gcn.py: (N, C, inner)"):              # and against torch.permute where the map is one
        assert np.array_equal(want, t.view(H._N, H._C, H._I).permute(1, 0, 2).contiguous().view(-1).numpy())
    if what.startswith("conv2d: OIHW -> (tap, c, m)"):
        assert np.array_equal(want, t.view(H._COUT, H._CIN, H._TAPS).permute(2, 1, 0).contiguous().view(-1).numpy())
    if what.startswith("conv2d: OIHW -> (tap, m, c)"):
        assert np.array_equal(want, t.view(H._COUT, H._CIN, H._TAPS).permute(2, 0, 1).contiguous().view(-1).numpy())
    if what.startswith("models/stgcn_debug.py: (N, C, T, V)"):
        assert np.array_equal(want, t.view(H._N, H._C * H._T, H._V).permute(1, 0, 2).contiguous().view(-1).numpy())


def test_permute_batch_layout():
    src = np.arange(H.PB_SRC, dtype=F32)
    out = H.permute_batch_expected(src, -7.25)
    big = H.PB_BIG
    assert out[0] == 7 and np.array_equal(out[1:big + 1], 300 + 2 * np.arange(big)) and np.all(out[big + 1:big + 6] == -7.25)
    assert np.array_equal(out[big + 6:], 296 - np.arange(257)) and out.size == H.PB_DST
    ranges = sorted((it[1], it[1] + it[2] * it[3] * it[4]) for it in H.PB_ITEMS)
    assert all(a[1] <= b[0] for a, b in zip(ranges, ranges[1:])) and ranges[0][1] == ranges[1][0]        # disjoint, two adjacent
    assert [it[1] for it in H.PB_ITEMS] != sorted(it[1] for it in H.PB_ITEMS)


# ---------------------------------------------------------------------------------------------------- b. sensitivity
def _ce_without_max(x, labels, inv, dt=F32):
    x = x.astype(dt)
    e = np.exp(x)
    se = e.sum(axis=1, keepdims=True)
    p = e / se
    return ((np.log(se[:, 0]) - x[np.arange(len(labels)), labels]).sum() * dt(inv)), p


def _ce_as_minus_log_p(x, labels, inv, dt=F32):
    p = R.softmax_ce(x, labels, inv, dt=dt)[2]
    return (-np.log(p[np.arange(len(labels)), labels])).sum() * dt(inv)


def test_cross_entropy_near_misses_fail_on_the_regimes_made_for_them():
    """evaluated in float32, as a kernel would: without the max subtraction exp(1e4) overflows (regime b); -log(p[label]) is inf where
    the label's probability underflows (regime c)"""
    with np.errstate(all="ignore"):
        for N in H.CE_N:
            for K in H.CE_K:
                x, labels = H.ce_inputs("b", N, K)
                l, _, p = R.softmax_ce(x, labels, H.CE_INV)
                lw, pw = _ce_without_max(x, labels, H.CE_INV)
                far(lw, l, H.BAND * H.float32_distance("shifted loss"), "loss without the max subtraction")
                far(pw, p, H.BAND * H.float32_distance("shifted probs"), "probs without the max subtraction")
                if K > 1:
                    x, labels = H.ce_inputs("c", N, K)
                    far(_ce_as_minus_log_p(x, labels, H.CE_INV), R.softmax_ce(x, labels, H.CE_INV)[0], H.TOL, "loss as -log p[label]")
                    assert np.isfinite(R.softmax_ce(x, labels, H.CE_INV, dt=F32)[0])


def _adam_without_bias_correction(w, m, v, g, t, lr, b1, b2, eps, dt):
    return R.adam_step(w, m, v, g, 10 ** 9, lr, b1, b2, eps, dt=dt)               # b ** t = 0


def _adam_eps_inside_the_root(w, m, v, g, t, lr, b1, b2, eps, dt):
    _, m, v = R.adam_step(w, m, v, g, t, lr, b1, b2, eps, dt=dt)
    return np.asarray(w, dt) - lr / (1 - b1 ** t) * m / np.sqrt(v / (1 - b2 ** t) + eps), m, v


@pytest.mark.parametrize("n", H.OPT_N)
def test_optimizer_near_misses(n):
    w0, gs = H.nesterov_inputs(n)
    ref = H.run_nesterov(n, F64)
    w, v, plain = w0.astype(F64), np.zeros(n), []
    for g in gs:                                          # momentum without the look-ahead term: w <- w + v
        v = H.SGD_MOM * v - H.SGD_LR * g
        w = w + v
        plain.append(w)
    bar = H.BAND * H.float32_distance("nesterov update")
    for a, b in zip(H.updates(w0, plain), H.updates(w0, [s[0] for s in ref])):
        far(a, b, bar, "nesterov without the look-ahead")
    far(plain[-1], ref[-1][0], H.OPT_TOL, "nesterov without the look-ahead: w")
    for t0 in (0, 999):
        w0 = H.adam_inputs(n, t0)[0]
        ref = H.updates(w0, [s[0] for s in H.run_adam(n, t0, F64)])
        for wrong in (_adam_without_bias_correction, _adam_eps_inside_the_root):
            for i, (a, b) in enumerate(zip(H.updates(w0, [s[0] for s in H.run_adam(n, t0, F64, step=wrong)]), ref)):
                far(a, b, H.BAND * H.float32_distance(H.adam_metric(t0, i)), "%s, step %d" % (wrong.__name__, t0 + 1 + i))


@pytest.mark.parametrize("regimes,nparts", H.BN_CASES)
def test_bn_finalize_near_misses(regimes, nparts):
    c = H.bn_case(regimes, nparts)
    ref = R.bn_finalize(c["partials"], c["count"], H.BN_EPS, H.BN_MOM, 1, c["gamma"], c["beta"], c["rm"], c["rv"])
    p = c["partials"].astype(F64)
    mean = p[:, :, 0].sum(1) / c["count"]
    var = p[:, :, 1].sum(1) / c["count"] - mean * mean
    if "const" in regimes:                               # variance without the clamp
        i = regimes.index("const")
        assert var[i] < -1e-4 and ref["var"][i] == 0 and ref["rstd"][i] == 1 / np.sqrt(H.BN_EPS)
        if len(regimes) == 1:
            with np.errstate(invalid="ignore"):
                far(1 / np.sqrt(var + H.BN_EPS), ref["rstd"], H.TOL, "rstd without the clamp")
    if nparts == 1 and regimes != ("one",):              # count = 6: 1 / (count - 1) is large.  The switch sits in the one-thread epilogue
        biased = R.bn_finalize(c["partials"], c["count"], H.BN_EPS, H.BN_MOM, 0, c["gamma"], c["beta"], c["rm"], c["rv"])
        if "const" not in regimes:
            far(biased["running_var"], ref["running_var"], H.TOL, "biased instead of unbiased moving variance")
    if regimes == ("one",):
        assert np.isfinite(ref["running_var"]).all() and ref["var"][0] >= 0


def test_the_float32_yardsticks_are_what_design_md_records():
    """X of every `4 X` bar: printed, and held to the decade DESIGN.md section 4.3 states so that a change of the inputs shows"""
    want = {"adam update, step 1": (1e-6, 1e-5), "adam update, steps 2 and 3": (1e-6, 1e-4), "adam update, step 1000": (1e-8, 1e-6),
            "nesterov update": (1e-8, 1e-5),
            "shifted probs": (1e-5, 1e-2), "shifted dlogits": (1e-5, 1e-2), "shifted loss": (1e-6, 1e-2), "far channel": (1e-4, 1.0)}
    for k, (lo, hi) in want.items():
        x = H.float32_distance(k)
        print("float32 evaluation against float64, %s: %.3e" % (k, x))
        assert lo <= x <= hi, (k, x)
