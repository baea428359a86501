"""The seven kernels of csrc/pgc.hip (ProjectionGraphConv(64, 32)) one at a time against tests/pgc_reference.py in float64, at the
sizes and regimes of tests/pgc_cases.py (which says what each is there for; tests/test_pgc_reference.py proves every case
admissible on the CPU), between poisoned guards (tests/util.py).

Each entry point is called through sar_amd._lib on its own.  Its inputs are the float64 reference's values rounded to float32, never
the previous kernel's output, and its reference is the float64 formula of that kernel on exactly those rounded inputs: a wrong
kernel is named by its own test, and its neighbour cannot compensate.  Every buffer the wrappers of sar_amd/ops.py allocate with
torch.empty -- q, the three partial arrays, saved, dsaved, the per-sample slab -- is here a guarded range with -7.25 around it; every
input one with NaN around it, and kept: no launch may modify an input's allocation.  Every case runs tight (ld = B P) and padded
(ld = B P + 7, and x with a further 3: ld_x != ld_out), and the two runs must agree bit for bit.  A field of `saved` / `dsaved` that a
kernel has no business reading is NaN.

Bars (pgc_cases.bar; both are the project's, there is no "k x float32" band in this file): 2e-5 norm-wise for the single-pass
outputs q, the partial sums, out, dh, dW, dbias; 1e-4 for everything behind the l2-normalise or the softmax backward.  dS and dqs
scale with 1 / qs and are compared vertex by vertex, each on its own scale (the starved vertex is 1e23 times the others); in the
dead regime the two clamped channels are 1e6 times the others, so what they dominate is also compared without them."""
import types

import pytest
import torch

import pgc_cases as K
import pgc_reference as R
from util import NAN, SENTINEL, Launch, _bits, drive, guarded, rel_err

pytestmark = pytest.mark.gpu
C, J, CJ = K.C, K.J, K.C * K.J
FWD_PART, DH_PART, BWD_PART, SAVED, DSAVED, SLAB = 2080, 2048, 4096, 11360, 2080, 8256
O_S, O_ZP, O_ZN, O_G, O_H, O_A, O_QS, O_N2 = 0, CJ, 2 * CJ, 3 * CJ, 4 * CJ, 5 * CJ, 5 * CJ + J * J, 5 * CJ + J * J + J
FIELDS = {"S": (O_S, (C, J)), "zp": (O_ZP, (C, J)), "zn": (O_ZN, (C, J)), "g": (O_G, (C, J)), "h": (O_H, (C, J)), "A": (O_A, (J, J)),
          "qs": (O_QS, (1, J)), "n2": (O_N2, (C,))}
PAD, X_EXTRA = 7, 3
NPARTS = [1, 2, 5]
SHARES = [0.4, 0.3, 0.15, 0.1, 0.05]
cases = pytest.mark.parametrize("case", K.CASES, ids=K.IDS)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib, ops
    assert (ops.PGC_FWD_PART, ops.PGC_DH_PART, ops.PGC_BWD_PART, ops.PGC_SAVED, ops.PGC_DSAVED, ops.PGC_SLAB) == \
        (FWD_PART, DH_PART, BWD_PART, SAVED, DSAVED, SLAB)
    _lib.load()
    return torch.device("cuda:0")


def nparts_of(P):
    """tiles of 128 columns, four per workgroup (csrc/pgc.hip); NOT asked of the library: a buffer sized by a wrong answer hides it"""
    return -(-(-(-P // 128)) // 4)


def launch_nparts(P):
    """the partial count the library will launch with must be the one the buffers are sized for, before anything is launched"""
    from sar_amd import _lib
    G = nparts_of(P)
    assert _lib.load().sar_pgc_nparts(P) == G, "sar_pgc_nparts(%d) = %d, not %d" % (P, _lib.load().sar_pgc_nparts(P), G)
    return G


class PL(Launch):
    KEEP_INPUTS = True

    def __init__(self, dev, pad, label=""):
        super().__init__(dev, pad)
        self.dists, self.label = [], label

    def inp(self, src, extra=0):
        view, whole = guarded(src.float(), self.pad + extra, NAN, self.dev, self.FRONT, self.IN_BACK)
        self.ins.append(("input %d" % len(self.ins), whole, whole.clone()))
        return view

    def dist(self, case, name, got, want, what=None):
        """`got` (a callable) judged as pgc_cases.distance judges the quantity `name`, against pgc_cases.bar(name)"""
        self.dists.append((case, name, got, want, what or name))

    def check(self):
        super().check()
        for case, name, got, want, what in self.dists:
            e = K.distance(case, name, got(), want)
            print("%s | %s-B%d-P%d | %s (pad %d): %.2e" % (self.label, case["regime"], case["B"], case["P"], what, self.pad, e))
            assert e < K.bar(name), "%s (pad %d): %.3e >= %.1e" % (what, self.pad, e, K.bar(name))


def run(dev, fn, label):
    return drive(dev, fn, PAD, launch=lambda d, pad: PL(d, pad, label))


def ok(rc, name):
    from sar_amd import _lib
    _lib.check(rc, name)


def P_(t):
    from sar_amd import _lib
    return _lib.ptr(t)


def stream():
    from sar_amd import _lib
    return _lib.stream_ptr()


def cn(t):
    """(B, C, P) -> CN [C][B P]"""
    return t.permute(1, 0, 2).reshape(t.shape[1], -1).contiguous().float()


def from_cn(t, B):
    return t.detach().cpu().reshape(t.shape[0], B, -1).permute(1, 0, 2)


def q_rows(q):
    """(B, P, J) -> [J][B P], flat"""
    return q.permute(2, 0, 1).reshape(-1).contiguous().float()


def q_of(flat, B, P):
    return flat.detach().cpu().view(J, B, P).permute(1, 2, 0)


def f64(t):
    """the float64 value of what a float32 buffer holds"""
    return t.float().double()


def setup(case):
    c = K.build(*case)
    ctx, grads, taps = K.reference(*case)
    cen, var, W, b = (t.reshape(-1) for t in c["prm"])
    cen64, s64 = cen.double().view(C, J), torch.sigmoid(var.double()).view(C, J)
    return types.SimpleNamespace(c=c, B=c["B"], P=c["P"], n=c["B"] * c["P"], ctx=ctx, grads=grads, taps=taps, cen=cen, var=var,
                                 W=W, b=b, cen64=cen64, s64=s64, W64=c["prm"][2][0].double(), b64=b.double())


def saved_of(ctx, B, only=None):
    """the (B, SAVED) float32 array of the forward pass's per-sample results; only = the fields the kernel may read, the others NaN"""
    sv = torch.full((B, SAVED), NAN, dtype=torch.float32)
    for k, (off, shape) in FIELDS.items():
        if only is None or k in only:
            sv[:, off:off + ctx[k][0].numel()] = ctx[k].reshape(B, -1).float()
    return sv


def field(flat, B, name):
    off, shape = FIELDS[name]
    n = 1
    for v in shape:
        n *= v
    return flat.detach().cpu().view(B, SAVED)[:, off:off + n].reshape((B,) + shape)


def shares(t, n):
    """(B, E) float64 -> (B, n, E) float32: n unequal shares, and the float64 sum of what was rounded"""
    w = torch.tensor(SHARES[:n], dtype=torch.float64)
    parts = (t[:, None, :] * (w / w.sum())[None, :, None]).float()
    return parts, parts.double().sum(1)


# ------------------------------------------------------------------------------------------------ sar_pgc_nparts
def test_nparts_at_the_edges(dev):
    from sar_amd import _lib
    lib = _lib.load()
    for P in [1, 3, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1024, 1025, 1536, 1537, 7500, 1 << 33]:
        assert lib.sar_pgc_nparts(P) == nparts_of(P), P
    assert [nparts_of(P) for P in (1, 512, 513, 1024, 1025)] == [1, 1, 2, 2, 3]
    assert lib.sar_pgc_nparts(0) == 0 and lib.sar_pgc_nparts(-1) == 0 and lib.sar_pgc_nparts(-(1 << 40)) == 0


# ------------------------------------------------------------------------------------------------ sar_pgc_assign_f32
@cases
def test_assign(dev, case):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B, P, G = a.B, a.P, launch_nparts(a.P)
    # the float64 sums of each workgroup's own four tiles
    S_ref = torch.stack([torch.einsum("bcp,bpj->bcj", a.ctx["x"][:, :, g * 512:(g + 1) * 512], a.ctx["q"][:, g * 512:(g + 1) * 512])
                         for g in range(G)], 1)
    qs_ref = torch.stack([a.ctx["q"][:, g * 512:(g + 1) * 512].sum(1) for g in range(G)], 1)

    def fn(g):
        x = g.inp(cn(a.c["x"]), X_EXTRA)
        q, part = g.flat("q", J * a.n), g.flat("part", B * G * FWD_PART)
        ok(lib.sar_pgc_assign_f32(P_(x), x.stride(0), B, P, P_(g.flat_in(a.cen)), P_(g.flat_in(a.var)), P_(q), P_(part), stream()),
           "sar_pgc_assign_f32")
        parts = lambda: part.cpu().view(B, G, FWD_PART)
        g.dist(a.c, "q", lambda: q_of(q, B, P), a.ctx["q"])
        g.dist(a.c, "S", lambda: parts()[:, :, :CJ].reshape(B, G, C, J), S_ref, "S, each workgroup's partial")
        g.dist(a.c, "qs", lambda: parts()[:, :, CJ:], qs_ref, "qs, each workgroup's partial")
        g.dist(a.c, "S", lambda: parts()[:, :, :CJ].double().sum(1), a.ctx["S"], "S summed in float64")
        g.dist(a.c, "qs", lambda: parts()[:, :, CJ:].double().sum(1), a.ctx["qs"], "qs summed in float64")
        g.ref("q columns sum to 1", lambda: q.view(J, a.n).double().sum(0), torch.ones(a.n, dtype=torch.float64), 1e-6)
    tight, _ = run(dev, fn, "assign")
    if a.c["regime"] == "clamp":
        q = q_of(tight.flats["q"][0], B, P)
        b, p, j = a.c["exact"][1]                                         # a column that is one vertex's center: a one-hot row
        assert q[b, p, j].item() == 1.0 and q[b, p].sum().item() == 1.0
        b, p, j, _ = a.c["sub"]                                           # d = 0 and 0 < d <= 1e-12: both clamped to the same logit
        assert q[b, p, j].item() == q[b, p, K.J_EXACT_A].item() and abs(q[b, p, j].item() - 0.5) < 1e-6
        b, p, j, _ = a.c["near"]
        assert abs(q[b, p, j].item() - a.ctx["q"][b, p, j].item()) < 1e-6 and abs(q[b, p, j].item() - 0.5) < 1e-3
    if a.c["regime"] == "starved":
        qs = tight.flats["part"][0].cpu().view(B, G, FWD_PART)[:, :, CJ + K.STARVED].double().sum(1)
        # on its own scale: q = exp(-d / 2) / sum with d of a few hundred, summed over 64 channels in float32: d is good to
        # 64 ulp(d) = 64 * 3e-5 in the worst case, q to half of that relative -- 1e-3; the bar is ten times that
        assert qs.min().item() > 0 and rel_err(qs, a.ctx["qs"][:, 0, K.STARVED]) < 1e-2


# ------------------------------------------------------------------------------------------------ sar_pgc_small_fwd_f32
@pytest.mark.parametrize("nparts", NPARTS)
@cases
def test_small_fwd(dev, case, nparts):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B = a.B
    parts, fed = shares(torch.cat([a.ctx["S"].reshape(B, -1), a.ctx["qs"].reshape(B, -1)], 1), nparts)
    S_, qs = fed[:, :CJ].view(B, C, J), fed[:, CJ:].view(B, 1, J)
    want = dict(R.pgc_graph(S_, qs, a.cen64, a.s64, a.W64, a.b64), S=S_, qs=qs)

    def fn(g):
        saved = g.flat("saved", B * SAVED)
        ok(lib.sar_pgc_small_fwd_f32(P_(g.flat_in(parts.reshape(-1))), B, nparts, P_(g.flat_in(a.cen)), P_(g.flat_in(a.var)),
                                     P_(g.flat_in(a.W)), P_(g.flat_in(a.b)), P_(saved), stream()), "sar_pgc_small_fwd_f32")
        for k in FIELDS:
            g.dist(a.c, k, lambda k=k: field(saved, B, k), want[k])
    tight, _ = run(dev, fn, "small_fwd nparts %d" % nparts)
    if a.c["regime"] == "dead":
        sv = tight.flats["saved"][0]
        zp, zn, n2 = field(sv, B, "zp"), field(sv, B, "zn"), field(sv, B, "n2")
        assert bool((zp[:, K.DEAD] == 0).all()) and bool((zn[:, K.DEAD] == 0).all()) and bool((n2[:, K.DEAD] == 0).all())
        for k, got in (("zp", zp), ("zn", zn)):                          # the faint channel on its own scale: 0 < n2 < 1e-12
            e = rel_err(got[:, K.FAINT], want[k][:, K.FAINT])
            assert e < K.TOL2, (k, e)
        assert bool(((n2[:, K.FAINT].double() - want["n2"][:, K.FAINT]).abs() <= K.TOL2 * want["n2"][:, K.FAINT]).all())
        assert 0 < n2[:, K.FAINT].min().item() and n2[:, K.FAINT].max().item() < K.EPS


# ------------------------------------------------------------------------------------------------ sar_pgc_project_f32
@cases
def test_project(dev, case):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B, P = a.B, a.P
    qf, sv = q_rows(a.ctx["q"]), saved_of(a.ctx, B, only=("h",))
    want = a.c["x"].double() + torch.einsum("bpj,bfj->bfp", f64(a.ctx["q"]), f64(a.ctx["h"]))

    def fn(g):
        x, out = g.inp(cn(a.c["x"]), X_EXTRA), g.out("out", C, a.n)
        assert x.stride(0) != out.stride(0)
        ok(lib.sar_pgc_project_f32(P_(x), x.stride(0), P_(g.flat_in(qf)), P_(g.flat_in(sv.reshape(-1))), B, P, P_(out), out.stride(0),
                                   stream()), "sar_pgc_project_f32")
        g.dist(a.c, "out", lambda: from_cn(out, B), want)
    run(dev, fn, "project")


# ------------------------------------------------------------------------------------------------ sar_pgc_bwd_reduce_f32
@cases
def test_bwd_reduce(dev, case):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B, P, G = a.B, a.P, launch_nparts(a.P)
    qf, dout, q64 = q_rows(a.ctx["q"]), a.c["dout"].double(), f64(a.ctx["q"])
    want = torch.stack([torch.einsum("bfp,bpj->bfj", dout[:, :, g * 512:(g + 1) * 512], q64[:, g * 512:(g + 1) * 512]) for g in range(G)], 1)

    def fn(g):
        d, part = g.inp(cn(a.c["dout"])), g.flat("part", B * G * DH_PART)
        ok(lib.sar_pgc_bwd_reduce_f32(P_(d), d.stride(0), P_(g.flat_in(qf)), B, P, P_(part), stream()), "sar_pgc_bwd_reduce_f32")
        g.dist(a.c, "dh", lambda: part.cpu().view(B, G, C, J), want, "dh, each workgroup's partial")
        g.dist(a.c, "dh", lambda: part.cpu().view(B, G, C, J).double().sum(1), want.sum(1), "dh summed in float64")
    run(dev, fn, "bwd_reduce")


# ------------------------------------------------------------------------------------------------ sar_pgc_small_bwd_f32
@pytest.mark.parametrize("nparts", NPARTS)
@cases
def test_small_bwd(dev, case, nparts):
    """the starved cases: s qs^2 underflows in float32, dS and dqs must come out finite (Launch.check) and right"""
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B = a.B
    parts, dh = shares(a.taps["dh"].reshape(B, -1), nparts)
    sv = saved_of(a.ctx, B)
    fed = {k: f64(a.ctx[k]) for k in FIELDS}
    want = R.pgc_graph_backward(dict(fed, s=a.s64, W=a.W64), dh.view(B, C, J))

    def fn(g):
        dsaved, slab = g.flat("dsaved", B * DSAVED), g.flat("slab", B * SLAB)
        ok(lib.sar_pgc_small_bwd_f32(P_(g.flat_in(parts.reshape(-1))), B, nparts, P_(g.flat_in(a.var)), P_(g.flat_in(a.W)),
                                     P_(g.flat_in(sv.reshape(-1))), P_(dsaved), P_(slab), stream()), "sar_pgc_small_bwd_f32")
        ds, sl = (lambda: dsaved.cpu().view(B, DSAVED)), (lambda: slab.cpu().view(B, SLAB))
        g.dist(a.c, "dS", lambda: ds()[:, :CJ].reshape(B, C, J), want["dS"])
        g.dist(a.c, "dqs", lambda: ds()[:, CJ:], want["dqs"])
        g.dist(a.c, "dW", lambda: sl()[:, :C * C].reshape(B, C, C), want["dW"])
        g.dist(a.c, "dbias", lambda: sl()[:, C * C:C * C + C], want["dbias"])
        g.dist(a.c, "pool_c", lambda: sl()[:, C * C + C:C * C + C + CJ].reshape(B, C, J), want["pool_c"])
        g.dist(a.c, "pool_s", lambda: sl()[:, C * C + C + CJ:].reshape(B, C, J), want["pool_s"])
    run(dev, fn, "small_bwd nparts %d" % nparts)


# ------------------------------------------------------------------------------------------------ sar_pgc_bwd_column_f32
def column_launch(lib, g, a, sv, dsv, G):
    x, d = g.inp(cn(a.c["x"]), X_EXTRA), g.inp(cn(a.c["dout"]), 1)
    dx, part = g.out("dx", C, a.n), g.flat("part", a.B * G * BWD_PART)
    ok(lib.sar_pgc_bwd_column_f32(P_(x), x.stride(0), P_(d), d.stride(0), P_(g.flat_in(q_rows(a.ctx["q"]))), P_(g.flat_in(sv.reshape(-1))),
                                  P_(g.flat_in(dsv.reshape(-1))), P_(g.flat_in(a.cen)), P_(g.flat_in(a.var)), a.B, a.P, P_(dx), dx.stride(0),
                                  P_(part), stream()), "sar_pgc_bwd_column_f32")
    return dx, part


@cases
def test_bwd_column(dev, case):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B, P, G = a.B, a.P, launch_nparts(a.P)
    sv = saved_of(a.ctx, B, only=("h",))
    dsv = torch.cat([a.taps["dS"].reshape(B, -1), a.taps["dqs"].reshape(B, -1)], 1).float()
    want = R.pgc_column_backward(a.c["x"].double(), a.c["dout"].double(), f64(a.ctx["q"]), f64(a.ctx["h"]), f64(a.taps["dS"]),
                                 f64(a.taps["dqs"]), a.cen64, a.s64)

    def fn(g):
        dx, part = column_launch(lib, g, a, sv, dsv, G)
        sums = lambda: part.cpu().view(B, G, 2, C, J).double().sum(1)
        g.dist(a.c, "dx", lambda: from_cn(dx, B), want["dx"])
        g.dist(a.c, "col_c", lambda: sums()[:, 0], want["col_c"])
        g.dist(a.c, "col_s", lambda: sums()[:, 1], want["col_s"])
    run(dev, fn, "bwd_column")


@pytest.mark.parametrize("case", [c for c in K.CASES if c[0] == "clamp"], ids=[i for i in K.IDS if i.startswith("clamp")])
def test_bwd_column_clamp_passes_no_gradient(dev, case):
    """dS = dqs = 0 and dout = 0 at the two probed elements (pgc_cases.build): dx there is -sum_j dl z / s alone, and every vertex but
    the probed one is either at z = 0 or takes no weight.  `sub` (0 < d <= 1e-12, clamped): dl z / s would be 1e-6 and must be absent;
    `near` (2e-12 <= d <= 1e-11): it must be there.  Both to a thousandth of that term."""
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    B, P, G = a.B, a.P, launch_nparts(a.P)
    sv, dsv = saved_of(a.ctx, B, only=("h",)), torch.zeros(B, DSAVED)
    zero = torch.zeros_like(a.taps["dS"])
    want = R.pgc_column_backward(a.c["x"].double(), a.c["dout"].double(), f64(a.ctx["q"]), f64(a.ctx["h"]), zero, zero[:, 0], a.cen64, a.s64)

    def fn(g):
        dx, _ = column_launch(lib, g, a, sv, dsv, G)
        g.dist(a.c, "dx", lambda: from_cn(dx, B), want["dx"])
    tight, _ = run(dev, fn, "bwd_column_clamp_passes_no_gradient")
    dx = from_cn(tight.outs["dx"][0], B).double()
    for k, masked in (("sub", True), ("near", False)):
        b, p, j, ch = a.c[k]
        term = (want["dl_free"][b, p, j] * (a.c["x"][b, ch, p].double() - a.cen64[ch, j]) / a.s64[ch, j] ** 2).item()
        assert abs(term) > 1e-9 and (want["dl"][b, p, j].item() == 0) == masked
        err = abs(dx[b, ch, p].item() - want["dx"][b, ch, p].item())
        print("%s: dl z / s = %.3e, dx %.3e, reference %.3e" % (k, term, dx[b, ch, p].item(), want["dx"][b, ch, p].item()))
        assert err <= 1e-3 * abs(term), (k, err, term)
        assert (abs(want["dx"][b, ch, p].item()) <= 1e-3 * abs(term)) == masked      # the reference itself: absent / present


# ------------------------------------------------------------------------------------------------ sar_pgc_param_grad_f32
@cases
def test_param_grad(dev, case):
    from sar_amd import _lib
    lib, a = _lib.load(), setup(case)
    colsum = torch.cat([a.taps["col_c"].sum(0).reshape(-1), a.taps["col_s"].sum(0).reshape(-1)]).float()
    pooled = torch.cat([a.taps["pool_c"].sum(0).reshape(-1), a.taps["pool_s"].sum(0).reshape(-1)]).float()
    v = lambda t, i: f64(t)[i * CJ:(i + 1) * CJ].view(C, J)
    dcen, dvar = R.pgc_param_grad(v(colsum, 0), v(colsum, 1), v(pooled, 0), v(pooled, 1), a.s64)

    def fn(g):
        gc, gv = g.flat("dcenters", CJ), g.flat("dvariance", CJ)
        ok(lib.sar_pgc_param_grad_f32(P_(g.flat_in(colsum)), P_(g.flat_in(pooled)), P_(g.flat_in(a.var)), P_(gc), P_(gv), stream()),
           "sar_pgc_param_grad_f32")
        g.dist(a.c, "dcenters", lambda: gc.cpu().view(1, C, 1, J), dcen.view(1, C, 1, J))
        g.dist(a.c, "dvariance", lambda: gv.cpu().view(1, C, 1, J), dvar.view(1, C, 1, J))
    run(dev, fn, "param_grad")


# ------------------------------------------------------------------------------------------------ the whole layer (sar_amd/ops.py)
def layer(dev, g, a, x, dout, B):
    from sar_amd import ops
    P = a.P
    cen, var, W, b = (t.contiguous().to(dev) for t in a.c["prm"])
    xg, dg = g.inp(cn(x), X_EXTRA), g.inp(cn(dout), 1)
    out, dx = g.out("out", C, B * P), g.out("dx", C, B * P)
    gc, gv, gwb = g.flat("g_centers", CJ), g.flat("g_variance", CJ), g.flat("g_kernel | g_bias", C * C + C)
    q, sv = ops.pgc_forward(xg, B, P, cen, var, W, b, out)
    ops.pgc_backward(xg, dg, q, sv, B, P, cen, var, W, dx, gc.view(cen.shape), gv.view(var.shape), gwb)
    g.part("q", q)
    g.part("saved", sv)
    return dict(out=out, dx=dx, q=q, saved=sv, gc=gc, gv=gv, gwb=gwb)


@cases
def test_whole_layer(dev, case):
    """ops.pgc_forward / ops.pgc_backward at every case: the bars of the kernels, nothing wider; tight and padded bitwise equal; at
    B = 3 each sample alone is bitwise the batch's slice (the partial count depends on P only)"""
    a = setup(case)
    B, P = a.B, a.P
    want = K.quantities(a.c, a.ctx, a.grads, a.taps)
    keep = {}

    def fn(g):
        r = layer(dev, g, a, a.c["x"], a.c["dout"], B)
        keep[g.pad] = r
        g.dist(a.c, "out", lambda: from_cn(r["out"], B), want["out"])
        g.dist(a.c, "q", lambda: q_of(r["q"], B, P), want["q"])
        g.dist(a.c, "dx", lambda: from_cn(r["dx"], B), want["dx"])
        g.dist(a.c, "dcenters", lambda: r["gc"].cpu().view(1, C, 1, J), want["dcenters"])
        g.dist(a.c, "dvariance", lambda: r["gv"].cpu().view(1, C, 1, J), want["dvariance"])
        g.dist(a.c, "dW", lambda: r["gwb"].cpu()[:C * C].view(1, C, C), want["dW"])
        g.dist(a.c, "dbias", lambda: r["gwb"].cpu()[C * C:], want["dbias"])
    run(dev, fn, "whole_layer")
    for k in ("q", "saved"):                                             # the buffers ops allocates, tight against padded
        assert torch.equal(_bits(keep[0][k]), _bits(keep[PAD][k])), k
    if B == 3:
        full = keep[0]
        out_f, dx_f, q_f = from_cn(full["out"], B), from_cn(full["dx"], B), q_of(full["q"], B, P)
        for b in range(B):
            g = PL(dev, 0)
            one = layer(dev, g, a, a.c["x"][b:b + 1], a.c["dout"][b:b + 1], 1)
            torch.cuda.synchronize()
            g.check_guards()
            assert torch.equal(from_cn(one["out"], 1)[0], out_f[b]), b
            assert torch.equal(from_cn(one["dx"], 1)[0], dx_f[b]), b
            assert torch.equal(q_of(one["q"], 1, P)[0], q_f[b]), b


# ------------------------------------------------------------------------------------------------ rejected calls
def test_rejected_calls_launch_nothing(dev):
    """NULL operands, B < 1, B > 65535, P < 1, ld < B P for each strided operand, nparts < 1: the argument error, the entry point named,
    and every guarded buffer -- outputs, internal buffers, inputs -- as it was"""
    from sar_amd import _lib
    lib, a = _lib.load(), setup(("init", 2, 128))
    B, P, G = a.B, a.P, nparts_of(a.P)
    g = PL(dev, PAD)
    x, dout = g.inp(cn(a.c["x"])), g.inp(cn(a.c["dout"]))
    out, dx = g.out("out", C, a.n), g.out("dx", C, a.n)
    t = dict(x=x, dout=dout, out=out, dx=dx, cen=g.flat_in(a.cen), var=g.flat_in(a.var), W=g.flat_in(a.W), bias=g.flat_in(a.b),
             q=g.flat("q", J * a.n), fpart=g.flat("fpart", B * G * FWD_PART), dpart=g.flat("dpart", B * G * DH_PART),
             cpart=g.flat("cpart", B * G * BWD_PART), saved=g.flat("saved", B * SAVED), dsaved=g.flat("dsaved", B * DSAVED),
             slab=g.flat("slab", B * SLAB), colsum=g.flat("colsum", BWD_PART), pooled=g.flat("pooled", BWD_PART),
             gc=g.flat("gc", CJ), gv=g.flat("gv", CJ))
    good = dict({k: v.data_ptr() for k, v in t.items()}, B=B, P=P, nparts=G, ld_x=x.stride(0), ld_dout=dout.stride(0),
                ld_out=out.stride(0), ld_dx=dx.stride(0))
    n = 0
    for name, (call, ptrs, lds, has_B, has_P, has_nparts) in K.entry_points(lib).items():
        bad = [{k: None} for k in ptrs] + [{k: B * P - 1} for k in lds]
        bad += [{"B": 0}, {"B": -1}, {"B": 65536, **{k: 65536 * P for k in lds}}] if has_B else []
        bad += [{"P": 0}, {"P": -3}] if has_P else []
        bad += [{"nparts": 0}, {"nparts": -1}] if has_nparts else []
        for change in bad:
            rc = call(types.SimpleNamespace(**dict(good, **change)))
            assert rc == _lib.SAR_E_ARG, "%s with %s returned %d" % (name, change, rc)
            assert name[:-4].encode() in lib.sar_last_error_string(), (name, change, lib.sar_last_error_string())
            n += 1
    assert n == 38 + 7 + 6 * 3 + 4 * 2 + 2 * 2          # pointers, leading dimensions, B (param_grad has none), P, nparts
    torch.cuda.synchronize()
    g.check_nothing_written()
    g.check_guards()
    g.check_inputs()


def test_wrappers_raise_value_error_before_the_library(dev, monkeypatch):
    """the operand checks of sar_amd/operands.py (O.on_gpu, O.cn_matrix): a ValueError, raised before anything is allocated or launched"""
    from sar_amd import _lib, ops
    a = setup(("init", 2, 128))
    B, P = a.B, a.P
    g = PL(dev, PAD)
    cen, var, W, b = (t.contiguous().to(dev) for t in a.c["prm"])
    x, dout, out, dx = g.inp(cn(a.c["x"])), g.inp(cn(a.c["dout"])), g.out("out", C, a.n), g.out("dx", C, a.n)
    gc, gv, gwb = g.flat("gc", CJ), g.flat("gv", CJ), g.flat("gwb", C * C + C)
    q, sv = torch.zeros(J, a.n, device=dev), torch.zeros(B, SAVED, device=dev)

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(_lib, "load", no_library)
    wide = torch.zeros(C, 2 * a.n, device=dev)
    for bad, match in ((x.double(), "float32"), (x.cpu(), "CUDA"), (x[:63], "64 rows"), (x[:, :-1], "columns"), (wide[:, ::2], "unit column stride"),
                       (x.reshape(-1)[:C * a.n], "2-D"), (None, "float32")):
        with pytest.raises(ValueError, match=match):
            ops.pgc_forward(bad, B, P, cen, var, W, b, out)
        with pytest.raises(ValueError, match=match):
            ops.pgc_forward(x, B, P, cen, var, W, b, bad)
        with pytest.raises(ValueError, match=match):
            ops.pgc_backward(x, bad, q, sv, B, P, cen, var, W, dx, gc.view(cen.shape), gv.view(var.shape), gwb)
        with pytest.raises(ValueError, match=match):
            ops.pgc_backward(x, dout, q, sv, B, P, cen, var, W, bad, gc.view(cen.shape), gv.view(var.shape), gwb)
    for Bb, Pb in ((0, P), (B, 0), (-1, P)):
        with pytest.raises(ValueError, match="B >= 1 and P >= 1"):
            ops.pgc_forward(x, Bb, Pb, cen, var, W, b, out)
    with pytest.raises(ValueError, match="g_kernel_bias"):
        ops.pgc_backward(x, dout, q, sv, B, P, cen, var, W, dx, gc.view(cen.shape), gv.view(var.shape), gwb[:-1])
    torch.cuda.synchronize()
    g.check_nothing_written()
    g.check_guards()
    g.check_inputs()
