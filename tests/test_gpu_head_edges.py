"""The kernels that end every training step of every engine -- pooling, the dense layer, cross entropy, both optimizers, the BatchNorm
finalisations and the weight re-layouts (csrc/elementwise.hip, sar_adam_f32 / sar_permute3_f32 in csrc/conv2d.hip) -- against
tests/head_reference.py in float64, at the smallest shapes that reach every branch of their index arithmetic (tests/head_cases.py
says which shape is there for which branch), between poisoned guards.

Every output and every in-place buffer (w, v, m, the moving statistics) is a guarded range of tests/util.py with -7.25 around it,
every input one with NaN around it (labels: a label no class has).  After each launch, through util.Launch.check: the float64 bar,
every guard bit for bit, everything finite except where NaN is the specified result, every input's allocation unmodified.  Each
flat case runs twice through util.drive: the second run must repeat the first bit for bit (no atomics, a fixed order in every
reduction); the pooling kernels, the only ones with a leading dimension, run tight and with pads 4 and 7 as in
tests/test_gpu_guard_bands.py.

Bars: TOL = 2e-5 norm-wise and the 1e-6 of the optimizer state are those of tests/test_gpu_stgcn_kernels.py (test_head_loss_and_sgd,
test_graph_conv_forward_and_stats); Adam's w, m and v take the 1e-6 too.  A metric no earlier test has a bar for -- the optimizer
UPDATE w_t - w_(t-1), regime (b) of the cross entropy -- is held to 4x the distance of head_reference evaluated in float32 from its
float64 evaluation (head_cases.float32_distance; tests/test_head_reference.py prints and pins the figures).  The mean-1000 channel
is held to TOL alone: a float32 evaluation of E x^2 - mean^2 is 11 % off there, 4x that is no bar, and the figure is only printed."""
import itertools

import numpy as np
import pytest
import torch

import head_cases as H
import head_reference as R
from util import SENTINEL, Launch, _bits, drive, rel_err

pytestmark = pytest.mark.gpu
TOL, OPT_TOL = H.TOL, H.OPT_TOL
PADS = [4, 7]
F32, F64 = np.float32, np.float64
NO_LABEL = 1 << 40               # around the labels: a read of it is a label outside [0, K) and makes the loss NaN


class HL(Launch):
    KEEP_INPUTS = True


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


def twice(dev, fn):
    """two runs of a flat case: the five assertions on each, and the second bitwise the first"""
    return drive(dev, fn, 0, launch=HL)


def untouched(g, name, n):
    """an output the call does not name: allocated, not passed, must still hold the sentinel"""
    buf = g.flat(name, n)
    g.ref(name + " (absent: untouched)", lambda: buf, torch.full((n,), SENTINEL), 0)


def band(metric, what, got, want):
    """a metric without an earlier bar: within 4x the float32 evaluation's distance"""
    x, e = H.float32_distance(metric), rel_err(got, want)
    print("%s: float32 evaluation %.3e, kernel %.3e, bar %.3e" % (what, x, e, H.BAND * x))
    assert e <= H.BAND * x, "%s: %.3e > 4 x %.3e" % (what, e, x)


# ---------------------------------------------------------------------------------------------------- pooling
@pytest.mark.parametrize("pad", PADS)
@pytest.mark.parametrize("TV", H.POOL_TV)
def test_pooling_forward_and_backward(dev, TV, pad):
    from sar_amd import ops
    for N in H.POOL_N:
        for Mp, C in itertools.product(H.POOL_MP, H.POOL_C):
            y, dfeat = H.pool_inputs(TV, N, Mp, C)
            feat_ref, dy_ref = T(R.pool_fwd(y, N, Mp, TV)), T(R.pool_bwd(dfeat, N, Mp, TV))

            def fn(g):
                feat, dy = g.flat("feat", N * C), g.out("dy", C, N * Mp * TV)
                ops.pool_fwd(g.inp(T(y)), N * Mp, TV, Mp, feat.view(N, C))
                ops.pool_bwd(g.flat_in(T(dfeat)), N * Mp, TV, Mp, dy)
                g.ref("pooled features TV %d N %d Mp %d C %d" % (TV, N, Mp, C), lambda: feat.view(N, C), feat_ref, TOL)
                g.ref("pool backward", dy, dy_ref, TOL)
            drive(dev, fn, pad, launch=HL)
            twice(dev, fn)


# ---------------------------------------------------------------------------------------------------- dense layer
@pytest.mark.parametrize("C", H.FC_C)
def test_dense_forward(dev, C):
    from sar_amd import ops
    for K, N, with_bias in itertools.product(H.FC_K, H.FC_N, (True, False)):
        c = H.fc_inputs(C, K, N)
        want = T(R.fc_fwd(c["feat"], c["W"], c["bias"] if with_bias else None)).reshape(-1)

        def fn(g):
            logits = g.flat("logits", N * K)
            ops.fc_fwd(g.flat_in(T(c["feat"])), g.flat_in(T(c["W"])), g.flat_in(T(c["bias"])) if with_bias else None, logits.view(N, K))
            g.ref("logits C %d K %d N %d bias %d" % (C, K, N, with_bias), lambda: logits, want, TOL)
        twice(dev, fn)


@pytest.mark.parametrize("mode", ["all", "dW and dbias only", "dfeat only"])
@pytest.mark.parametrize("C,K", H.FC_BWD)
def test_dense_backward(dev, C, K, mode):
    from sar_amd import ops
    for N in H.FC_N:
        c = H.fc_inputs(C, K, N)
        dW_ref, db_ref, df_ref = (T(a).reshape(-1) for a in R.fc_bwd(c["feat"], c["W"], c["dlogits"]))

        def fn(g):
            feat, W, dl = g.flat_in(T(c["feat"])), g.flat_in(T(c["W"])), g.flat_in(T(c["dlogits"]))
            dW = db = dfeat = None
            if mode != "dfeat only":
                dW, db = g.flat("dW", C * K), g.flat("dbias", K)
                g.ref("dW C %d K %d N %d" % (C, K, N), lambda: dW, dW_ref, TOL)
                g.ref("dbias", lambda: db, db_ref, TOL)
            else:
                untouched(g, "dW", C * K), untouched(g, "dbias", K)
            if mode != "dW and dbias only":
                dfeat = g.flat("dfeat", N * C)
                g.ref("dfeat", lambda: dfeat, df_ref, TOL)
            else:
                untouched(g, "dfeat", N * C)
            ops.fc_bwd(feat, W, dl, None if dW is None else dW.view(C, K), db, None if dfeat is None else dfeat.view(N, C))
        twice(dev, fn)


# ---------------------------------------------------------------------------------------------------- cross entropy
def ce_launch(g, ops, x, labels, N, K, outs=("loss", "dlogits", "probs"), tag=""):
    """one launch; the outputs not in `outs` are allocated, not passed, and must stay untouched"""
    bufs = {}
    for name, n in (("loss", 1), ("dlogits", N * K), ("probs", N * K)):
        if name in outs:
            bufs[name] = g.flat(name + tag, n)
        else:
            untouched(g, name + tag, n)
    d, p = bufs.get("dlogits"), bufs.get("probs")
    ops.softmax_ce(g.flat_in(T(x)), g.flat_in(T(labels), fill=NO_LABEL), H.CE_INV, bufs.get("loss"),
                   None if d is None else d.view(N, K), None if p is None else p.view(N, K))
    return bufs


@pytest.mark.parametrize("regime,K", [(r, K) for r in H.CE_REGIMES for K in H.CE_K if H.ce_inputs(r, 1, K) is not None])
def test_cross_entropy(dev, regime, K):
    """(regimes (c) and (d) need a second class: no K = 1)"""
    from sar_amd import ops
    for N in H.CE_N:
        x, labels = H.ce_inputs(regime, N, K)
        l_ref, d_ref, p_ref = R.softmax_ce(x, labels, H.CE_INV)
        if regime == "b":                                    # probs and dlogits: those of the UNSHIFTED logits
            _, d_ref, p_ref = R.softmax_ce(H.ce_inputs("a", N, K)[0], labels, H.CE_INV)
        what = "regime %s N %d K %d: " % (regime, N, K)

        def fn(g):
            g.bufs = b = ce_launch(g, ops, x, labels, N, K)
            if regime != "b":
                g.ref(what + "loss", lambda: b["loss"], T(np.array([l_ref])), TOL)
                g.ref(what + "dlogits", lambda: b["dlogits"], T(d_ref).reshape(-1), TOL)
                g.ref(what + "probs", lambda: b["probs"], T(p_ref).reshape(-1), TOL)
        tight, _ = twice(dev, fn)
        b = {k: v.cpu() for k, v in tight.bufs.items()}
        if regime == "b":
            band("shifted loss", what + "loss", b["loss"], T(np.array([l_ref])))
            band("shifted dlogits", what + "dlogits", b["dlogits"], T(d_ref).reshape(-1))
            band("shifted probs", what + "probs", b["probs"], T(p_ref).reshape(-1))
        if regime == "c":                                    # loss = 200 per row, and the underflowed probabilities are exactly 0
            assert abs(b["loss"].item() / (N * H.CE_INV) - 200) < 200 * TOL
            p = b["probs"].view(N, K)
            assert int((p == 0).sum()) == N * (K - 1) and bool((p.max(dim=1).values == 1).all())
        if regime == "d":
            assert int((b["probs"] == 0).sum()) == N and int((b["dlogits"] == 0).sum()) == N


@pytest.mark.parametrize("N,K", [(5, 65), (3, 10)])
def test_cross_entropy_optional_outputs(dev, N, K):
    from sar_amd import ops
    x, labels = H.ce_inputs("a", N, K)
    l_ref, d_ref, p_ref = R.softmax_ce(x, labels, H.CE_INV)
    want = {"loss": T(np.array([l_ref])), "dlogits": T(d_ref).reshape(-1), "probs": T(p_ref).reshape(-1)}
    for r in range(4):
        for outs in itertools.combinations(("loss", "dlogits", "probs"), r):
            def fn(g):
                b = ce_launch(g, ops, x, labels, N, K, outs)
                for k in outs:
                    g.ref("%s of %s" % (k, outs), lambda k=k: b[k], want[k], TOL)
            twice(dev, fn)


@pytest.mark.parametrize("K", H.CE_BAD_K)
def test_cross_entropy_labels_without_a_class(dev, K):
    """regime (e): labels K and -1 in a batch of 5.  The loss is NaN, those rows' dlogits are NaN; the other rows' dlogits and all
    probs are bitwise those of the same batch with valid labels"""
    from sar_amd import ops
    x, labels, bad = H.ce_bad_inputs(K)
    l_ref, d_ref, p_ref = R.softmax_ce(x, bad, H.CE_INV)
    good_rows = [0, 2, 4]

    def fn(g):
        g.nan_ok = {"loss bad", "dlogits bad"}
        g.good = ce_launch(g, ops, x, labels, 5, K, tag=" good")
        g.bad = ce_launch(g, ops, x, bad, 5, K, tag=" bad")
        g.ref("probs", lambda: g.bad["probs"], T(p_ref).reshape(-1), TOL)
        g.ref("dlogits of the rows with a class", lambda: g.bad["dlogits"].view(5, K)[good_rows], T(d_ref[good_rows]), TOL)
    tight, again = drive(dev, fn, 0, bitwise=False, launch=HL)
    for g in (tight, again):
        d, d0 = g.bad["dlogits"].view(5, K), g.good["dlogits"].view(5, K)
        assert bool(torch.isnan(g.bad["loss"]).all()) and bool(torch.isnan(d[[1, 3]]).all()) and np.isnan(l_ref)
        assert torch.equal(d[good_rows], d0[good_rows]) and torch.equal(g.bad["probs"], g.good["probs"])
        assert bool(torch.isfinite(g.good["loss"]).all())
    for k in ("loss", "dlogits", "probs"):                  # determinism, NaN included
        assert torch.equal(_bits(tight.bad[k]), _bits(again.bad[k])) and torch.equal(tight.good[k], again.good[k])


# ---------------------------------------------------------------------------------------------------- optimizers
@pytest.mark.parametrize("n", H.OPT_N)
def test_sgd_nesterov(dev, n):
    from sar_amd import ops
    w0, gs = H.nesterov_inputs(n)
    ref = H.run_nesterov(n, F64)

    def fn(g):
        w, v = g.flat("w", T(w0)), g.flat("v", torch.zeros(n))
        lr = g.flat_in(T(np.array([H.SGD_LR], dtype=F32)))
        g.states = []
        for gi in gs:
            ops.sgd_nesterov(w, v, g.flat_in(T(gi)), lr, H.SGD_MOM)
            g.states.append((w.cpu().clone(), v.cpu().clone()))
    tight, _ = twice(dev, fn)
    for t, ((w, v), (wr, vr)) in enumerate(zip(tight.states, ref)):
        assert rel_err(w, T(wr)) < OPT_TOL and rel_err(v, T(vr)) < OPT_TOL, "step %d" % (t + 1)
    for t, (u, ur) in enumerate(zip(H.updates(w0, [s[0].numpy() for s in tight.states]), H.updates(w0, [s[0] for s in ref]))):
        band("nesterov update", "n %d step %d: w_t - w_(t-1)" % (n, t + 1), T(u), T(ur))


@pytest.mark.parametrize("t0", [0, 999])
@pytest.mark.parametrize("n", H.OPT_N)
def test_adam(dev, n, t0):
    """steps 1, 2, 3 from the zero state and step 1000 from a running m and v, w = 0 before both (the first w IS the update);
    element 0 has g = 0 throughout and m = v = 0: its update is exactly 0, not 0 / 0"""
    from sar_amd import ops
    w0, m0, v0, gs, t = H.adam_inputs(n, t0)
    ref = H.run_adam(n, t0, F64)

    def fn(g):
        w, m, v = g.flat("w", T(w0)), g.flat("m", T(m0)), g.flat("v", T(v0))
        lr = g.flat_in(T(np.array([H.ADAM_LR], dtype=F32)))
        g.states = []
        for i, gi in enumerate(gs):
            step = g.flat_in(T(np.array([t + i], dtype=F32)))
            ops.adam(w, m, v, g.flat_in(T(gi)), lr, step, H.ADAM_B1, H.ADAM_B2, H.ADAM_EPS)
            g.states.append((w.cpu().clone(), m.cpu().clone(), v.cpu().clone()))
    tight, _ = twice(dev, fn)
    for i, ((w, m, v), (wr, mr, vr)) in enumerate(zip(tight.states, ref)):
        e = rel_err(w, T(wr)), rel_err(m, T(mr)), rel_err(v, T(vr))
        print("adam n %d step %d: w %.2e m %.2e v %.2e" % (n, t + i, *e))
        assert max(e) < OPT_TOL, "step %d: %s" % (t + i, e)              # test_head_loss_and_sgd's bar for optimizer state
        if n > 1:
            assert w[0].item() == w0[0] and m[0].item() == 0 and v[0].item() == 0
    for i, (u, ur) in enumerate(zip(H.updates(w0, [s[0].numpy() for s in tight.states]), H.updates(w0, [s[0] for s in ref]))):
        band(H.adam_metric(t0, i), "adam n %d step %d: w_t - w_(t-1)" % (n, t + i), T(u), T(ur))


# ---------------------------------------------------------------------------------------------------- BatchNorm
BN_VARIANTS = [("everything", True, True, True), ("bare", False, False, False), ("moving statistics only", False, False, True)]


@pytest.mark.parametrize("regimes,nparts", H.BN_CASES, ids=["%s-%d" % ("+".join(r), n) for r, n in H.BN_CASES])
def test_bn_finalize(dev, regimes, nparts):
    from sar_amd import ops
    C = len(regimes)
    c = H.bn_case(regimes, nparts)
    for (variant, affine, stats, moving), unbiased in itertools.product(BN_VARIANTS, (0, 1)):
        ref = R.bn_finalize(c["partials"], c["count"], H.BN_EPS, H.BN_MOM, unbiased, c["gamma"] if affine else None,
                            c["beta"] if affine else None, c["rm"] if moving else None, c["rv"] if moving else None)
        what = "%s nparts %d, %s, unbiased %d: " % ("+".join(regimes), nparts, variant, unbiased)

        def fn(g):
            part = g.flat_in(T(c["partials"]))
            gam, bet = (g.flat_in(T(c["gamma"])), g.flat_in(T(c["beta"]))) if affine else (None, None)
            o = g.o = {k: g.flat(k, C) for k in ("scale", "shift") + (("mean", "rstd") if stats else ())}
            if not stats:
                untouched(g, "mean", C), untouched(g, "rstd", C)
            rm, rv = g.flat("running_mean", T(c["rm"])), g.flat("running_var", T(c["rv"]))
            if moving:
                o["running_mean"], o["running_var"] = rm, rv
            else:
                g.ref("running_mean (absent: untouched)", lambda: rm, T(c["rm"]), 0)
                g.ref("running_var (absent: untouched)", lambda: rv, T(c["rv"]), 0)
            ops.bn_finalize(part, nparts, C, c["count"], H.BN_EPS, H.BN_MOM, unbiased, gam, bet, rm if moving else None,
                            rv if moving else None, o.get("mean"), o.get("rstd"), o["scale"], o["shift"])
            for k in o:
                g.ref(what + k, lambda k=k: o[k], T(ref[k]), TOL)
        tight, _ = twice(dev, fn)
        if regimes == ("far",) and stats:                    # a record, no assertion: rstd is held to TOL above; any float32 evaluation is ~11 % off
            print("%srstd: float32 evaluation %.3e, kernel %.3e" % (what, H.float32_distance("far channel"), rel_err(tight.o["rstd"].cpu(), T(ref["rstd"]))))
        if "const" in regimes and stats:                     # the clamp: var = 0 exactly, rstd = 1 / sqrt(eps) to float32
            i = regimes.index("const")
            assert tight.o["rstd"][i].item() == F32(1.0 / np.sqrt(F64(F32(H.BN_EPS))))


BNB_VARIANTS = [("everything", True, True, True), ("no k1..k3", True, True, False), ("k1..k3 only, no gamma", False, False, True)]


@pytest.mark.parametrize("centered", [0, 1])
@pytest.mark.parametrize("nparts", H.BN_NPARTS)
def test_bn_backward_finalize(dev, nparts, centered):
    from sar_amd import ops
    C = H.BNB_C
    c = H.bnb_case(nparts, centered)
    for (slots, off1, off2), (variant, with_gamma, grads, ks) in itertools.product(H.BNB_LAYOUTS, BNB_VARIANTS):
        ref = R.bn_bwd_finalize(c["s1"], c["s2"], centered, c["count"], c["gamma"] if with_gamma else None, c["mean"], c["rstd"])
        what = "nparts %d centered %d slots %d offsets (%d, %d), %s: " % (nparts, centered, slots, off1, off2, variant)

        def fn(g):
            part = g.flat_in(T(H.bnb_buffer(c, slots, off1, off2)))          # NaN in the slots the call does not name
            gam = g.flat_in(T(c["gamma"])) if with_gamma else None
            mean, rstd = g.flat_in(T(c["mean"])), g.flat_in(T(c["rstd"]))
            o = {}
            for k, on in (("dgamma", grads), ("dbeta", grads), ("k1", ks), ("k2", ks), ("k3", ks)):
                if on:
                    o[k] = g.flat(k, C)
                    g.ref(what + k, lambda k=k: o[k], T(ref[k]), TOL)
                else:
                    untouched(g, k, C)
            ops.bn_bwd_finalize(part, nparts, slots * nparts, slots, off1, off2, C, c["count"], gam, mean, rstd, o.get("dgamma"),
                                o.get("dbeta"), o.get("k1"), o.get("k2"), o.get("k3"), centered=bool(centered))
        twice(dev, fn)


@pytest.mark.parametrize("affine", [True, False])
@pytest.mark.parametrize("C", H.BN_EVAL_C)
def test_bn_eval_affine(dev, C, affine):
    from sar_amd import ops
    c = H.bn_eval_inputs(C)
    sc, sh = R.bn_eval_affine(c["gamma"] if affine else None, c["beta"] if affine else None, c["rm"], c["rv"], H.BN_EPS)

    def fn(g):
        scale, shift = g.flat("scale", C), g.flat("shift", C)
        ops.bn_eval_affine(g.flat_in(T(c["gamma"])) if affine else None, g.flat_in(T(c["beta"])) if affine else None,
                           g.flat_in(T(c["rm"])), g.flat_in(T(c["rv"])), H.BN_EPS, scale, shift)
        g.ref("eval scale C %d" % C, lambda: scale, T(sc), TOL)
        g.ref("eval shift", lambda: shift, T(sh), TOL)
    twice(dev, fn)


# ---------------------------------------------------------------------------------------------------- re-layouts (exact copies: bitwise)
@pytest.mark.parametrize("batch,Rr,Cc", H.TRANSPOSE)
def test_transpose(dev, batch, Rr, Cc):
    from sar_amd import ops
    x = H.randn(H.rng("tr", batch, Rr, Cc), batch * Rr * Cc)
    want = T(R.transpose(x, batch, Rr, Cc))

    def fn(g):
        out = g.flat("out", x.size)
        ops.transpose(g.flat_in(T(x)), out, batch, Rr, Cc)
        g.ref("transpose", lambda: out, want, 0)
    twice(dev, fn)


@pytest.mark.parametrize("case", H.PERMUTE3, ids=[c[0] for c in H.PERMUTE3])
def test_permute3(dev, case):
    from sar_amd import ops
    what, n, d0, d1, d2, s0, s1, s2 = case
    x = H.randn(H.rng("p3", what), n)
    want = T(R.permute3(x, d0, d1, d2, s0, s1, s2))          # (asserts that the index map stays inside the source)

    def fn(g):
        out = g.flat("out", d0 * d1 * d2)
        ops.permute3(g.flat_in(T(x)), out, d0, d1, d2, s0, s1, s2)
        g.ref(what, lambda: out, want, 0)
    twice(dev, fn)


def test_permute3_batch(dev):
    """items of 262 147, 257 and 1 elements in one launch sized by the largest; the 5-element gap between two destination ranges
    keeps the sentinel (it is part of the expected buffer)"""
    from sar_amd import ops
    x = H.randn(H.rng("pb"), H.PB_SRC)
    want = T(H.permute_batch_expected(x, SENTINEL))          # (asserts that every item's index map stays inside the source)
    assert max(it[1] + it[2] * it[3] * it[4] for it in H.PB_ITEMS) == H.PB_DST
    pb = ops.PermuteBatch()
    for it in H.PB_ITEMS:
        pb.add(*it)
    pb.finalize(dev)
    assert pb.max_elems == H.PB_BIG

    def fn(g):
        dst = g.flat("dst", H.PB_DST)
        pb.run(g.flat_in(T(x)), dst)
        g.ref("permute3_batch", lambda: dst, want, 0)
    twice(dev, fn)


# ---------------------------------------------------------------------------------------------------- argument errors
def _raw(name, *args):
    """an entry point itself, where the wrapper in sar_amd.ops cannot express the call (a NULL it dereferences, a size it derives)"""
    from sar_amd import _lib as L
    L.check(getattr(L.load(), name)(*[L.ptr(a) if torch.is_tensor(a) else a for a in args], L.stream_ptr()), name)


def _bad_calls():
    """(what, fn(g, ops)): the SAR_REQUIRE conditions of the entry points above.  Every call names guarded outputs -- fresh ones
    hold the sentinel, in-place buffers ones --, none may be written"""
    def f(g, *shape):
        return g.flat_in(torch.ones(*shape))

    def o(g, name, *shape):
        return g.flat(name, int(np.prod(shape))).view(*shape)
    ones = lambda g, name, n: g.flat(name, torch.ones(n))
    part = lambda g: f(g, 2, 3, 2)
    return [
        ("pool_fwd: B no multiple of Mp", lambda g, ops: ops.pool_fwd(g.inp(torch.ones(3, 30)), 3, 10, 2, o(g, "feat", 1, 3))),
        ("pool_fwd: ld < B TV", lambda g, ops: ops.pool_fwd(g.inp(torch.ones(3, 30)), 4, 10, 2, o(g, "feat", 2, 3))),
        ("pool_fwd: no output", lambda g, ops: (o(g, "feat", 1, 3), ops.pool_fwd(g.inp(torch.ones(3, 20)), 2, 10, 2, None))),
        ("pool_bwd: B no multiple of Mp", lambda g, ops: ops.pool_bwd(f(g, 1, 3), 3, 10, 2, g.out("dy", 3, 30))),
        ("pool_bwd: no input", lambda g, ops: ops.pool_bwd(None, 2, 10, 2, g.out("dy", 3, 20))),
        ("fc_fwd: no W", lambda g, ops: ops.fc_fwd(f(g, 2, 3), None, None, o(g, "logits", 2, 4))),
        ("fc_fwd: N = 0", lambda g, ops: _raw("sar_fc_fwd_f32", f(g, 2, 3), f(g, 3, 4), None, 0, 3, 4, o(g, "logits", 2, 4))),
        ("softmax_ce: no labels", lambda g, ops: _raw("sar_softmax_ce_f32", f(g, 2, 4), None, 2, 4, 0.5, o(g, "loss", 1), o(g, "dlogits", 2, 4), None)),
        ("softmax_ce: K = 0", lambda g, ops: _raw("sar_softmax_ce_f32", f(g, 2, 4), g.flat_in(torch.zeros(2, dtype=torch.int64), fill=NO_LABEL), 2, 0, 0.5,
                                                  o(g, "loss", 1), o(g, "dlogits", 2, 4), None)),
        ("fc_bwd: dW without dbias", lambda g, ops: ops.fc_bwd(f(g, 2, 3), f(g, 3, 4), f(g, 2, 4), o(g, "dW", 3, 4), None, o(g, "dfeat", 2, 3))),
        ("fc_bwd: no output at all", lambda g, ops: (o(g, "dW", 3, 4), ops.fc_bwd(f(g, 2, 3), f(g, 3, 4), f(g, 2, 4), None, None, None))),
        ("sgd_nesterov: no lr cell", lambda g, ops: ops.sgd_nesterov(ones(g, "w", 5), ones(g, "v", 5), f(g, 5), None, 0.9)),
        ("sgd_nesterov: n = 0", lambda g, ops: _raw("sar_sgd_nesterov_f32", ones(g, "w", 5), ones(g, "v", 5), f(g, 5), 0, f(g, 1), 0.9)),
        ("adam: no step cell", lambda g, ops: ops.adam(ones(g, "w", 5), ones(g, "m", 5), ones(g, "v", 5), f(g, 5), f(g, 1), None)),
        ("adam: n = 0", lambda g, ops: _raw("sar_adam_f32", ones(g, "w", 5), ones(g, "m", 5), ones(g, "v", 5), f(g, 5), 0, f(g, 1), f(g, 1), 0.9, 0.999, 1e-8)),
        ("bn_finalize: moving mean without moving variance",
         lambda g, ops: ops.bn_finalize(part(g), 3, 2, 6, 1e-3, 0.9, 1, None, None, ones(g, "rm", 2), None, None, None, o(g, "scale", 2), o(g, "shift", 2))),
        ("bn_finalize: no shift", lambda g, ops: ops.bn_finalize(part(g), 3, 2, 6, 1e-3, 0.9, 1, None, None, None, None, None, None, o(g, "scale", 2), None)),
        ("bn_finalize: count = 0", lambda g, ops: ops.bn_finalize(part(g), 3, 2, 0, 1e-3, 0.9, 1, None, None, None, None, None, None, o(g, "scale", 2), o(g, "shift", 2))),
        ("bn_finalize: nparts = 0", lambda g, ops: ops.bn_finalize(part(g), 0, 2, 6, 1e-3, 0.9, 1, None, None, None, None, None, None, o(g, "scale", 2), o(g, "shift", 2))),
        ("bn_bwd_finalize: k1 without k2",
         lambda g, ops: ops.bn_bwd_finalize(part(g), 3, 6, 2, 0, 1, 2, 6, None, f(g, 2), f(g, 2), o(g, "dgamma", 2), o(g, "dbeta", 2), o(g, "k1", 2), None, o(g, "k3", 2))),
        ("bn_bwd_finalize: no mean", lambda g, ops: ops.bn_bwd_finalize(part(g), 3, 6, 2, 0, 1, 2, 6, None, None, f(g, 2), o(g, "dgamma", 2), o(g, "dbeta", 2))),
        ("bn_eval_affine: no moving variance", lambda g, ops: _raw("sar_bn_eval_affine_f32", None, None, f(g, 2), None, 1e-3, 2, o(g, "scale", 2), o(g, "shift", 2))),
        ("bn_eval_affine: C = 0", lambda g, ops: _raw("sar_bn_eval_affine_f32", None, None, f(g, 2), f(g, 2), 1e-3, 0, o(g, "scale", 2), o(g, "shift", 2))),
        ("transpose: R = 0", lambda g, ops: ops.transpose(f(g, 6), o(g, "out", 6), 1, 0, 6)),
        ("transpose: no output", lambda g, ops: (o(g, "out", 6), ops.transpose(f(g, 6), None, 1, 2, 3))),
        ("permute3: d1 = 0", lambda g, ops: ops.permute3(f(g, 6), o(g, "out", 6), 2, 0, 3, 3, 1, 1)),
        ("permute3: no source", lambda g, ops: ops.permute3(None, o(g, "out", 6), 1, 2, 3, 6, 3, 1)),
    ]


@pytest.mark.parametrize("what", [w for w, _ in _bad_calls()])
def test_argument_errors_write_nothing(dev, what):
    from sar_amd import ops, _lib as L
    call = dict(_bad_calls())[what]
    g = HL(dev, 0)
    with pytest.raises(L.SarError):
        call(g, ops)
    torch.cuda.synchronize()
    g.check_guards()
    g.check_inputs()
    inplace = {"w": 1.0, "v": 1.0, "m": 1.0, "rm": 1.0}      # in-place buffers started as ones, outputs as the sentinel
    for name, (view, whole) in list(g.outs.items()) + list(g.flats.items()):
        assert bool((view == inplace.get(name, SENTINEL)).all()), "%s: written by a rejected call" % name


def test_permute3_batch_argument_errors(dev):
    from sar_amd import _lib as L
    g = HL(dev, 0)
    src, dst = g.flat_in(torch.ones(8)), g.flat("dst", 8)
    table = torch.zeros(56, dtype=torch.uint8, device=dev)
    for items, nitems, max_elems in ((None, 1, 8), (table, 0, 8), (table, 1, 0), (table, 65536, 8)):
        with pytest.raises(L.SarError):
            L.check(L.load().sar_permute3_batch_f32(L.ptr(src), L.ptr(dst), L.ptr(items), nitems, max_elems, L.stream_ptr()), "sar_permute3_batch_f32")
    torch.cuda.synchronize()
    g.check_nothing_written()
    g.check_inputs()
