"""The cases of tests/test_gpu_pgc_edges.py (csrc/pgc.hip, ProjectionGraphConv(64, 32)), shared with tests/test_pgc_reference.py so
that the CPU file proves every case admissible -- finite in float64, every built condition met, the float32 restatement close to
float64 -- before the GPU file holds the kernels to a fixed bar on it.  Every input is a float32 value, so float64 and the kernels
see the same numbers.

Sizes.  The column passes (assign, bwd reduce, bwd column) take tiles of 128 columns, four per workgroup, so sar_pgc_nparts steps
at P = 512 k + 1; the projection takes 256 columns per workgroup.  P = 1, 3: one ragged tile; 127 / 128 / 129: a tile's edge;
255 / 256 / 257: the projection's edge; 512 / 513: the last full workgroup of four tiles and the first second partial; 1025: a third.
V plays no part in these kernels, P is free.

Regimes.
  init     centers at the engine's glorot scale (init_pgc(scale=0.1)).
  wide     init_pgc(scale=1.0), the draw of tests/test_gpu_stpgcn.py.
  starved  vertex STARVED's center moved away along every channel until its float64 qs = sum_p q lies in [1e-30, 1e-20] in every
           sample: qs > 0 in float32 but s qs^2 is not.  Built by bisection, not found by seed.
  clamp    column A: vertex J_EXACT_A's center IS the column (d = 0, clamped) and J_SUB's differs from it in one channel by a few
           ulp with 0 < d <= 1e-12 (clamped, but z != 0: the only place where "the clamp passes no gradient" can be seen, q is about
           1/2 each); column B: J_EXACT_B's center is the column (a one-hot row of q); column C: J_NEAR's center differs in one channel
           with d in [2e-12, 1e-11] (just above the clamp, gradient passes) and J_TWIN's with d about 1e-9 (nothing special: it
           shares the column's weight, so that dl of J_NEAR is of order one and not q (1 - q) = 0).
  dead     channel DEAD of x all zero (block 0's output is post-ReLU) with centers[DEAD, :] = 0: zp = 0 and n2 = 0 exactly; channel
           FAINT of x scaled down with centers[FAINT, :] = 0 until 0 < n2 < 1e-12: the clamped branch of the l2-normalise with
           zn != 0, where the backward pass's two branches differ.
Out of the table: qs == 0 in float32 (the reference model divides by zero too), variance so negative that sigmoid underflows, and
x scaled by 4 ("far": the float32 restatement is 8e-5 from float64 there, tests/test_pgc_reference.py)."""
import functools

import torch

import pgc_reference as R
from util import rel_err

C, J = 64, 32
EPS = R.EPS
TOL1, TOL2 = 2e-5, 1e-4          # single-pass outputs; everything behind the normalisation or the softmax backward
F32_BAR = 1.25e-5                # admissibility: the float32 restatement's distance from float64, every compared quantity
STARVED, BAND = 5, (1e-30, 1e-20)
J_EXACT_A, J_SUB, J_EXACT_B, J_NEAR, J_TWIN = 3, 11, 20, 7, 26
DEAD, FAINT, FAINT_BAND = 9, 40, (2e-14, 9e-13)

# (regime, B, P): every P at least once, B = 1 and B = 3 at least five times each.  The small P stand under `init`: with the wide draw a
# vertex of a three-column sample has qs below 1e-30 by itself
CASES = [("init", 1, 1), ("init", 3, 3), ("init", 2, 128), ("init", 3, 257), ("init", 1, 512),
         ("wide", 1, 129), ("wide", 2, 255), ("wide", 3, 256), ("wide", 1, 513), ("wide", 2, 1025),
         ("starved", 1, 129), ("starved", 2, 127), ("starved", 2, 1025),
         ("clamp", 2, 129), ("clamp", 1, 255), ("clamp", 3, 1025),
         ("dead", 1, 255), ("dead", 3, 128), ("dead", 2, 513)]
IDS = ["%s-B%d-P%d" % c for c in CASES]
STARVED_BASE = {129: 0.1, 127: 0.1, 1025: 1.0}      # the draw under a starved case: wide at the size where the default draw fails


def _draw(B, P, scale):
    """the recipe of tests/test_gpu_stpgcn.py: _layer_case"""
    seed = B * 100 + P
    g = torch.Generator().manual_seed(seed)
    x = torch.relu(torch.randn(B, C, P, generator=g))
    p = R.init_pgc({}, seed + 1, dtype=torch.float32, scale=scale)
    dout = torch.randn(B, C, P, generator=g)
    return x, [p[k].clone() for k in R.NAMES], dout


def _forward64(x, prm):
    return R.pgc_forward(x.double(), *(t.double() for t in prm))[1]


def _starve(x, prm):
    """move centers[:, STARVED] towards -inf (x >= 0: away from every column) until log10 qs is -25 on average"""
    base = prm[0][0, :, 0, STARVED].clone()

    def log_qs(t):
        prm[0][0, :, 0, STARVED] = base - t
        return torch.log10(_forward64(x, prm)["qs"][:, 0, STARVED])

    lo, hi = 0.0, 16.0
    assert log_qs(hi).max().item() < -25
    for _ in range(40):
        mid = 0.5 * (lo + hi)
        if log_qs(mid).mean().item() > -25:
            lo = mid
        else:
            hi = mid
    log_qs(hi)


def _ulps(v, k):
    """the float32 k ulps above the float32 v"""
    return (v.view(torch.int32) + k).view(torch.float32)


def _near(x, prm, b, p, j, lo, hi, skip=()):
    """centers[:, j] = column (b, p) of x but for one channel, k ulps up, so that d = ((k ulp) / s)^2 lies in [lo, hi] in float64"""
    cen, s = prm[0], torch.sigmoid(prm[1].double())[0, :, 0, j]
    cen[0, :, 0, j] = x[b, :, p]
    for c in range(C):
        v = x[b, c, p].reshape(1)
        if not 0.25 < v.item() < 3.9 or c in skip:
            continue
        for k in range(1, 400):
            d = (((_ulps(v, k).double() - v.double()) / s[c]) ** 2).item()
            if lo <= d <= hi:
                cen[0, c, 0, j] = _ulps(v, k)[0]
                return c
            if d > hi:
                break
    raise AssertionError("no channel of column (%d, %d) reaches a distance in [%g, %g]" % (b, p, lo, hi))


@functools.lru_cache(maxsize=None)
def build(regime, B, P):
    """dict(x (B, 64, P), prm = [centers, variance, kernel, bias] in the model's shapes, dout (B, 64, P)), all float32, and the
    marks of the regime"""
    scale = {"init": 0.1, "starved": STARVED_BASE.get(P, 0.1)}.get(regime, 1.0)
    x, prm, dout = _draw(B, P, scale)
    case = dict(regime=regime, B=B, P=P, x=x, prm=prm, dout=dout)
    if regime == "starved":
        _starve(x, prm)
    if regime == "clamp":
        a, b, c = (0, P // 2), (B - 1, P - 1), (B // 2, 5)
        prm[0][0, :, 0, J_EXACT_A] = x[a[0], :, a[1]]
        prm[0][0, :, 0, J_EXACT_B] = x[b[0], :, b[1]]
        case["sub"] = a + (J_SUB, _near(x, prm, a[0], a[1], J_SUB, 2e-13, 8e-13))
        case["near"] = c + (J_NEAR, _near(x, prm, c[0], c[1], J_NEAR, 3e-12, 9e-12))
        case["twin"] = c + (J_TWIN, _near(x, prm, c[0], c[1], J_TWIN, 5e-10, 2e-9, skip=(case["near"][3],)))   # another channel
        case["exact"] = [a + (J_EXACT_A,), b + (J_EXACT_B,)]
        for bb, pp, _, ch in (case["sub"], case["near"]):      # dx there is then dS q^T and the dl term alone: the latter, of the
            dout[bb, ch, pp] = 0                               # order of 1e-6, is not lost in the rounding of a dout of order one
    if regime == "dead":
        x[:, DEAD] = 0
        prm[0][0, DEAD] = 0
        prm[0][0, FAINT] = 0
        full = x[:, FAINT].clone()
        alpha = 1e-7
        for _ in range(3):                        # n2 is alpha^2 times a factor that hardly moves with alpha
            x[:, FAINT] = full * alpha
            alpha *= (5e-13 / _forward64(x, prm)["n2"][:, FAINT].max().item()) ** 0.5
    return case


@functools.lru_cache(maxsize=None)
def reference(regime, B, P, dtype=torch.float64):
    """(ctx, grads, taps) of tests/pgc_reference.py in `dtype` on the case's float32 inputs"""
    c = build(regime, B, P)
    _, ctx = R.pgc_forward(c["x"].to(dtype), *(t.to(dtype) for t in c["prm"]))
    taps = {}
    grads = R.pgc_backward(ctx, c["dout"].to(dtype), taps)
    return ctx, grads, taps


@functools.lru_cache(maxsize=None)
def staged32(regime, B, P):
    """the taps of the backward pass in float32 FROM the float64 forward rounded to float32: what a backward kernel is given in
    tests/test_gpu_pgc_edges.py, and so the float32 figure that belongs to a per-kernel comparison"""
    ctx = {k: (v.float() if torch.is_tensor(v) else v) for k, v in reference(regime, B, P)[0].items()}
    taps = {}
    R.pgc_backward(ctx, build(regime, B, P)["dout"], taps)
    return taps


def quantities(case, ctx, grads, taps):
    """name -> tensor: everything a kernel hands on, as tests/test_gpu_pgc_edges.py compares it"""
    out = ctx["x"] + torch.einsum("bpj,bfj->bfp", ctx["q"], ctx["h"])
    return dict(q=ctx["q"], S=ctx["S"], qs=ctx["qs"], zp=ctx["zp"], n2=ctx["n2"], zn=ctx["zn"], A=ctx["A"], g=ctx["g"], h=ctx["h"],
                out=out, dh=taps["dh"], dS=taps["dS"], dqs=taps["dqs"], pool_c=taps["pool_c"], pool_s=taps["pool_s"],
                col_c=taps["col_c"], col_s=taps["col_s"], dx=grads[0].reshape(out.shape), dcenters=grads[1], dvariance=grads[2],
                dW=grads[3], dbias=grads[4])


SINGLE_PASS = ("q", "S", "qs", "out", "dh", "dW", "dbias")     # held to TOL1, everything else to TOL2
PER_VERTEX = ("dS", "dqs")       # trailing axis j, scaled by 1 / qs: a starved vertex is 1e23 times the others


def per_vertex_err(got, want):
    """the worst over the vertices j (the last axis) of rel_err of that vertex's slice: each vertex on its own scale"""
    return max(rel_err(got[..., j], want[..., j]) for j in range(want.shape[-1]))


def live_rows(case, t, axis):
    """t without the channels whose clamped l2-normalise makes them 1e6 times the others (dead regime), along `axis`"""
    if case["regime"] != "dead":
        return t
    keep = [c for c in range(C) if c not in (DEAD, FAINT)]
    return t.index_select(axis, torch.tensor(keep, device=t.device))


def distance(case, name, got, want):
    """the figure a quantity is judged by: norm-wise (util.rel_err); per vertex for what scales with 1 / qs; for what the dead and
    the faint channel dominate, the worse of the whole tensor and of the other channels alone"""
    got, want = got.detach().double().cpu().reshape(want.shape), want.detach().double().cpu()
    if name in PER_VERTEX:
        e = per_vertex_err(got, want)
        if name != "dqs":
            e = max(e, per_vertex_err(live_rows(case, got, 1), live_rows(case, want, 1)))
        return e
    e = rel_err(got, want)
    if name in ("dx", "dcenters", "dvariance", "pool_c", "pool_s", "col_c", "col_s"):
        e = max(e, rel_err(live_rows(case, got, 1), live_rows(case, want, 1)))
    return e


def bar(name):
    return TOL1 if name in SINGLE_PASS else TOL2


# ---- the seven entry points, for the rejected-argument tests (tests/test_pgc_abi.py on the CPU, tests/test_gpu_pgc_edges.py between guards)
def entry_points(lib):
    """name -> (call(a), pointer operands, leading dimensions, takes B, takes P, takes nparts)"""
    s = None
    return {
        "sar_pgc_assign_f32": (lambda a: lib.sar_pgc_assign_f32(a.x, a.ld_x, a.B, a.P, a.cen, a.var, a.q, a.fpart, s),
                               ("x", "cen", "var", "q", "fpart"), ("ld_x",), True, True, False),
        "sar_pgc_small_fwd_f32": (lambda a: lib.sar_pgc_small_fwd_f32(a.fpart, a.B, a.nparts, a.cen, a.var, a.W, a.bias, a.saved, s),
                                  ("fpart", "cen", "var", "W", "bias", "saved"), (), True, False, True),
        "sar_pgc_project_f32": (lambda a: lib.sar_pgc_project_f32(a.x, a.ld_x, a.q, a.saved, a.B, a.P, a.out, a.ld_out, s),
                                ("x", "q", "saved", "out"), ("ld_x", "ld_out"), True, True, False),
        "sar_pgc_bwd_reduce_f32": (lambda a: lib.sar_pgc_bwd_reduce_f32(a.dout, a.ld_dout, a.q, a.B, a.P, a.dpart, s),
                                   ("dout", "q", "dpart"), ("ld_dout",), True, True, False),
        "sar_pgc_small_bwd_f32": (lambda a: lib.sar_pgc_small_bwd_f32(a.dpart, a.B, a.nparts, a.var, a.W, a.saved, a.dsaved, a.slab, s),
                                  ("dpart", "var", "W", "saved", "dsaved", "slab"), (), True, False, True),
        "sar_pgc_bwd_column_f32": (lambda a: lib.sar_pgc_bwd_column_f32(a.x, a.ld_x, a.dout, a.ld_dout, a.q, a.saved, a.dsaved, a.cen, a.var,
                                                                       a.B, a.P, a.dx, a.ld_dx, a.cpart, s),
                                   ("x", "dout", "q", "saved", "dsaved", "cen", "var", "dx", "cpart"), ("ld_x", "ld_dout", "ld_dx"),
                                   True, True, False),
        "sar_pgc_param_grad_f32": (lambda a: lib.sar_pgc_param_grad_f32(a.colsum, a.pooled, a.var, a.gc, a.gv, s),
                                   ("colsum", "pooled", "var", "gc", "gv"), (), False, False, False),
    }
