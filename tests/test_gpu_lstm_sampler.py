"""TemporalSampler (models/lstm_sampler.py on csrc/lstm.hip): the recurrent kernels, the top-k, the frame gather and the module end to
end, against tests/lstm_reference.py in float64 (pinned by tests/test_lstm_reference.py).

Error bar.  A recurrence compounds rounding over T steps, so the project's per-kernel bar (rel_err < 2e-5, tests/util.py) is not
assumed.  The yardstick is the FLOAT32 CPU run of the same reference against its float64 run on the same inputs; the GPU's bar for a
quantity is max(2e-5, 4 x that float32-CPU error) -- the factor 4 for the different summation order inside the dot products (MFMA
k-blocks against a sequential loop) and the device's exp.  Every comparison prints both errors.  Worst seen on MI355X (GPU / float32
CPU): WORST below, from a run of this file -- at most 6.4e-7 on the GPU against at most 6.1e-7 for float32 on the CPU, so every bar
was its 2e-5 floor; DESIGN.md section 3.17 holds the same figures.

The top-k and the gather are exact (element for element / bitwise); dvalues has the plain 2e-5 bar.
The module's selection is compared with the stable descending top-k of the DEVICE's own scores, and its output and gradients with
the reference evaluated at the device's indices: a near-tie that falls differently in float32 and float64 cannot fail a case."""
import functools

import pytest
import torch

import lstm_reference as R
from models.lstm_sampler import TemporalSampler
from sar_amd import _lib, ops
from util import NAN, SENTINEL, assert_flat_guards_untouched, assert_guards_untouched, guarded, guarded_flat, rel_err

pytestmark = pytest.mark.gpu
BAR = 2e-5
# worst (GPU error, float32-CPU error) per group of comparisons, measured on MI355X; every bar was the 2e-5 floor (4 x the float32-CPU
# error never reached it)
WORST = {
    "recurrent kernels, forward (h, gates, c)": (6.4e-7, 3.0e-7),        # gates at (u 64, N 19, T 37)
    "recurrent kernels, backward (dz)": (2.5e-7, 2.0e-7),                # (u 128, N 5, T 12) / (u 5, N 3, T 7)
    "module: scores, out": (4.1e-7, 2.1e-7),                             # out of [64, 20] at (5, 3, 37, 25)
    "module: parameter gradients and dx": (4.6e-7, 6.1e-7),              # [64] at (2, 3, 300, 25): recurrent_kernel / kernel of layer 0
    "gather: dvalues (plain 2e-5 bar)": (9.2e-8, None),
}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def tm(a):
    """(N, T, R) -> the stack's CN matrix [R][T N], time-major columns t N + n"""
    N, T, Rr = a.shape
    return a.permute(2, 1, 0).reshape(Rr, T * N).contiguous()


def within(what, got, want, ref32):
    """got (device) against want (float64) under the bar max(2e-5, 4 x the float32-CPU error of the same quantity)"""
    e, e32 = rel_err(got, want), rel_err(ref32, want)
    bar = max(BAR, 4 * e32)
    print("%s: gpu %.2e, float32 cpu %.2e, bar %.2e" % (what, e, e32, bar))
    assert e < bar, "%s: %.3e >= %.3e (float32 cpu %.3e)" % (what, e, bar, e32)


# ---------------------------------------------------------------------------------------------- 1. the recurrent kernels alone
REC_CASES = [(1, 1, 1), (1, 3, 5), (5, 3, 7), (20, 17, 9), (64, 19, 37), (128, 5, 12)]


def _rec_reference(zin, U, dh, dtype):
    """z = zin + h U as a layer whose kernel is the identity and whose bias is zero (both exact in every dtype)"""
    u = U.shape[0]
    z = zin.to(dtype).requires_grad_(True)
    h, gates, c = R.lstm_layer(z, torch.eye(4 * u, dtype=dtype), U.to(dtype), torch.zeros(4 * u, dtype=dtype), return_state=True)
    dz, = torch.autograd.grad(h, z, dh.to(dtype))
    return tuple(tm(t.detach()) for t in (h, gates, c, dz))


@functools.lru_cache(maxsize=None)
def rec_case(u, N, T):
    """inputs, the float64 reference and its float32 run, computed once and shared (never modified)"""
    g = torch.Generator().manual_seed(1000 * u + 10 * N + T)
    zin, U = torch.randn(N, T, 4 * u, generator=g), torch.randn(u, 4 * u, generator=g) / u ** 0.5
    dh = torch.randn(N, T, u, generator=g)
    return zin, U, dh, _rec_reference(zin, U, dh, torch.float64), _rec_reference(zin, U, dh, torch.float32)


def run_rec(dev, zin_cn, U, dh_cn, u, N, T, pad=0, keep=None):
    """forward (saving) and backward on CN operands with `pad` guard columns: inputs in NaN, outputs in the sentinel"""
    n = T * N
    z, zw = guarded(zin_cn.to(dev), pad, NAN, dev)
    d, dw = guarded(dh_cn.to(dev), pad, NAN, dev)
    Uv, Uw = guarded_flat(U.to(dev), NAN, dev)
    Uv = Uv.view(u, 4 * u)
    h, hw = guarded((u, n), pad, SENTINEL, dev)
    gates, gw = guarded((4 * u, n), pad, SENTINEL, dev)
    c, cw = guarded((u, n), pad, SENTINEL, dev)
    dz, dzw = guarded((4 * u, n), pad, SENTINEL, dev)
    ops.lstm_fwd(z, Uv, h, u, N, T, gates, c)
    ops.lstm_bwd(d, gates, c, Uv, dz, u, N, T)
    torch.cuda.synchronize()
    if keep is not None:
        keep.update(hw=hw, gw=gw, cw=cw, dzw=dzw)
    return h, gates, c, dz


@pytest.mark.parametrize("u,N,T", REC_CASES)
def test_recurrent_kernels_against_float64(dev, u, N, T):
    zin, U, dh, ref, ref32 = rec_case(u, N, T)
    got = run_rec(dev, tm(zin), U, tm(dh), u, N, T)
    for name, a, b, b32 in zip(("h", "gates", "c", "dz"), got, ref, ref32):
        within("(u %d, N %d, T %d) %s" % (u, N, T, name), a, b, b32)


def test_inference_form_writes_the_same_h(dev):
    u, N, T = 20, 17, 9
    zin, U, dh, _, _ = rec_case(u, N, T)
    h = run_rec(dev, tm(zin), U, tm(dh), u, N, T)[0]
    h2 = torch.full((u, T * N), SENTINEL, device=dev)
    ops.lstm_fwd(tm(zin).to(dev), U.to(dev), h2, u, N, T)            # NULL save pointers
    assert torch.equal(h2, h)


def test_too_wide_is_rejected_and_nothing_is_written(dev):
    u, N, T = 129, 2, 3
    full = lambda rows: torch.full((rows, T * N), SENTINEL, device=dev)
    zin, U = torch.zeros(4 * u, T * N, device=dev), torch.zeros(u, 4 * u, device=dev)
    h, gates, c, dz = full(u), full(4 * u), full(u), full(4 * u)
    with pytest.raises(_lib.SarError, match=r"rc=-2.*sar_lstm_fwd_f32"):
        ops.lstm_fwd(zin, U, h, u, N, T, gates, c)
    with pytest.raises(_lib.SarError, match=r"rc=-2.*sar_lstm_bwd_f32"):
        ops.lstm_bwd(torch.zeros(u, T * N, device=dev), torch.zeros(4 * u, T * N, device=dev), torch.zeros(u, T * N, device=dev), U, dz,
                     u, N, T)
    torch.cuda.synchronize()
    for t in (h, gates, c, dz):
        assert bool((t == SENTINEL).all())


# ---------------------------------------------------------------------------------------------- 2. independence, bitwise
def test_a_sequence_does_not_depend_on_its_tile_or_launch(dev):
    u, N, T = 64, 19, 37
    zin, U, dh, _, _ = rec_case(u, N, T)
    zc, dc = tm(zin), tm(dh)
    full = run_rec(dev, zc, U, dc, u, N, T)
    again = run_rec(dev, zc, U, dc, u, N, T)
    for a, b in zip(full, again):
        assert torch.equal(a, b), "two launches of the same inputs differ"
    for n in (0, 15, 16, 18):
        alone = run_rec(dev, zc.view(4 * u, T, N)[:, :, n].contiguous(), U, dc.view(u, T, N)[:, :, n].contiguous(), u, 1, T)
        for name, a, b in zip(("h", "gates", "c", "dz"), full, alone):
            assert torch.equal(a.view(a.shape[0], T, N)[:, :, n], b), "sequence %d: %s differs from the launch of that sequence alone" % (n, name)
    short = run_rec(dev, zc[:, :5 * N].contiguous(), U, dc[:, :5 * N].contiguous(), u, N, 5)
    for name, a, b in zip(("h", "gates", "c"), full, short):          # (dz of a shorter clip is another quantity)
        assert torch.equal(a[:, :5 * N], b), "%s: the first 5 steps differ from a launch with T = 5" % name


# ---------------------------------------------------------------------------------------------- 3. guard bands
def test_recurrent_kernels_guard_bands(dev):
    u, N, T, pad = 5, 3, 7, 3
    zin, U, dh, ref, ref32 = rec_case(u, N, T)
    tight = run_rec(dev, tm(zin), U, tm(dh), u, N, T)
    keep = {}
    padded = run_rec(dev, tm(zin), U, tm(dh), u, N, T, pad=pad, keep=keep)
    for name, a, b, whole in zip(("h", "gates", "c", "dz"), padded, tight, (keep["hw"], keep["gw"], keep["cw"], keep["dzw"])):
        assert bool(torch.isfinite(a).all()), "%s: a NaN margin reached the result" % name
        assert torch.equal(a, b), "%s: ld = T N + %d differs from the tight launch" % (name, pad)
        assert_guards_untouched(whole, a.shape, SENTINEL, what=name)


def _gather_inputs(N, C, T, V, k, seed):
    g = torch.Generator().manual_seed(seed)
    x, dout, values = torch.randn(N, C, T, V, generator=g), torch.randn(N, C, k, V, generator=g), torch.randn(N, k, generator=g)
    idx = torch.stack([torch.randperm(T, generator=g)[:k] for _ in range(N)]).to(torch.int32)
    inv = torch.full((N, T), -1, dtype=torch.int32)
    inv.scatter_(1, idx.long(), torch.arange(k, dtype=torch.int32).expand(N, k))
    return x, dout, values, idx, inv


def run_gather(dev, x, dout, values, idx, inv, layout, want_dx=True):
    """the gather and its backward, every operand between guards (NaN / int32 max around inputs, the sentinel around outputs);
    layout: the (stride_n, stride_t) of dscores.  Returns the results after checking the guards."""
    N, C, T, V = x.shape
    k = idx.shape[1]
    fin = lambda t: guarded_flat(t.to(dev), NAN, dev)[0].view(t.shape)
    iin = lambda t: guarded_flat(t.to(dev), 0x7FFFFFFF, dev, dtype=torch.int32)[0].view(t.shape)
    out, outw = guarded_flat(N * C * k * V, SENTINEL, dev)
    dvalues, dvw = guarded_flat(N * k, SENTINEL, dev)
    dx, dxw = guarded_flat(N * C * T * V, SENTINEL, dev)
    sn, st = layout
    rows, cols = (T, N) if sn == 1 else (N, T)                         # dscores [1][T N] or [1][N T] as one guarded CN row
    ds, dsw = guarded((1, rows * cols), 5, SENTINEL, dev)
    xg, vg = fin(x), fin(values)
    ops.frame_gather(xg, iin(idx), vg, out.view(N, C, k, V))
    ops.frame_gather_bwd(xg, fin(dout), vg, iin(inv), dvalues.view(N, k), ds, sn, st, dx.view(N, C, T, V) if want_dx else None)
    torch.cuda.synchronize()
    assert_flat_guards_untouched(outw, out.numel(), SENTINEL, what="out")
    assert_flat_guards_untouched(dvw, dvalues.numel(), SENTINEL, what="dvalues")
    assert_flat_guards_untouched(dxw, dx.numel(), SENTINEL, what="dx")
    assert_guards_untouched(dsw, ds.shape, SENTINEL, what="dscores")
    if not want_dx:
        assert bool((dx == SENTINEL).all()), "dx written although none was asked for"
    dsc = ds.view(rows, cols).t() if sn == 1 else ds.view(rows, cols)   # -> (N, T)
    return out.view(N, C, k, V), dvalues.view(N, k), dsc, dx.view(N, C, T, V)


# ---------------------------------------------------------------------------------------------- 4. top-k, exact
TOPK_CASES = [(1, 1, 1), (3, 5, 5), (3, 37, 1), (2, 300, 200), (2, 2048, 2048), (2, 2048, 7)]


@functools.lru_cache(maxsize=None)
def topk_case(N, T, k):
    """small integers stored as floats (many deliberate ties) and their stable descending sort"""
    g = torch.Generator().manual_seed(100 * N + 7 * T + k)
    scores = torch.randint(-3, 4, (N, T), generator=g).float()
    order = torch.sort(scores, dim=1, descending=True, stable=True).indices[:, :k]
    return scores, torch.gather(scores, 1, order), order.to(torch.int32)


def run_topk(dev, scores, k, layout):
    N, T = scores.shape
    buf = (scores if layout == "nt" else scores.t()).contiguous().to(dev)       # (T, 1) or (1, N)
    sn, st = (T, 1) if layout == "nt" else (1, N)
    values = torch.full((N, k), SENTINEL, device=dev)
    idx = torch.full((N, k), -5, dtype=torch.int32, device=dev)
    inv = torch.full((N, T), -5, dtype=torch.int32, device=dev)
    ops.topk_desc(buf, sn, st, N, T, k, values, idx, inv)
    torch.cuda.synchronize()
    return values.cpu(), idx.cpu(), inv.cpu()


def check_inverse(idx, inv, T):
    N, k = idx.shape
    want = torch.full((N, T), -1, dtype=torch.int32)
    want.scatter_(1, idx.long(), torch.arange(k, dtype=torch.int32).expand(N, k))
    assert torch.equal(inv, want), "inv is not the inverse of idx"


@pytest.mark.parametrize("layout", ["nt", "tn"])
@pytest.mark.parametrize("N,T,k", TOPK_CASES)
def test_topk_equals_a_stable_descending_sort(dev, N, T, k, layout):
    scores, want_values, want_idx = topk_case(N, T, k)
    values, idx, inv = run_topk(dev, scores, k, layout)
    assert torch.equal(idx, want_idx) and torch.equal(values, want_values)
    check_inverse(idx, inv, T)


def test_topk_limits(dev):
    N = 2
    for T, k, rc in ((5, 6, -1), (2049, 7, -2)):
        scores = torch.zeros(N, T, device=dev)
        values, idx = torch.full((N, k), SENTINEL, device=dev), torch.full((N, k), -5, dtype=torch.int32, device=dev)
        inv = torch.full((N, T), -5, dtype=torch.int32, device=dev)
        with pytest.raises(_lib.SarError, match=r"rc=%d.*sar_topk_desc_f32" % rc):
            ops.topk_desc(scores, T, 1, N, T, k, values, idx, inv)
        torch.cuda.synchronize()
        assert bool((values == SENTINEL).all()) and bool((idx == -5).all()) and bool((inv == -5).all())


def test_topk_with_nan_stays_a_selection(dev):
    N, T, k = 3, 37, 9
    scores = topk_case(N, T, 1)[0].clone()
    scores[1, [0, 5, 6, 20]] = NAN
    scores[1, 7] = -NAN
    values, idx, inv = run_topk(dev, scores, k, "tn")
    for n in range(N):
        assert len(set(idx[n].tolist())) == k and int(idx[n].min()) >= 0 and int(idx[n].max()) < T
    check_inverse(idx, inv, T)
    want = torch.sort(scores[[0, 2]], dim=1, descending=True, stable=True).indices[:, :k].to(torch.int32)
    assert torch.equal(idx[[0, 2]], want), "a row without NaN is disturbed by a row with"


# ---------------------------------------------------------------------------------------------- 5. gather and its backward
@pytest.mark.parametrize("time_major", [True, False])
@pytest.mark.parametrize("N,C,T,V,k", [(3, 3, 7, 25, 4), (2, 2, 5, 5, 5)])
def test_gather_and_its_backward(dev, N, C, T, V, k, time_major):
    x, dout, values, idx, inv = _gather_inputs(N, C, T, V, k, 31 * N + T)
    layout = (1, N) if time_major else (T, 1)                  # (stride_n, stride_t) of dscores
    out, dvalues, dscores, dx = (t.cpu() for t in run_gather(dev, x, dout, values, idx, inv, layout))
    pick = idx.long().view(N, 1, k, 1).expand(N, C, k, V)
    assert torch.equal(out, torch.gather(x, 2, pick) * values.view(N, 1, k, 1)), "out is not x[n, :, idx] * values bit for bit"
    ref = (dout.double() * torch.gather(x, 2, pick).double()).sum(dim=(1, 3))
    e = rel_err(dvalues, ref)
    print("dvalues: %.2e" % e)
    assert e < BAR
    want_dx = torch.zeros_like(x).scatter_(2, pick, dout * values.view(N, 1, k, 1))
    assert torch.equal(dx, want_dx), "dx is not dout * values at the chosen frames and 0 elsewhere, bit for bit"
    want_ds = torch.zeros(N, T).scatter_(1, idx.long(), dvalues)
    assert torch.equal(dscores, want_ds), "dscores is not dvalues scattered through idx"
    run_gather(dev, x, dout, values, idx, inv, layout, want_dx=False)


# ---------------------------------------------------------------------------------------------- 6. / 7. the module, end to end
def _reference_run(x, params, top_k, idx, dout, dtype):
    xd = x.to(dtype).requires_grad_(True)
    pd = [tuple(p.to(dtype).requires_grad_(True) for p in layer) for layer in params]
    out, scores, _ = R.temporal_sampler(xd, pd, top_k, indices=idx)
    grads = torch.autograd.grad(out, [xd] + [p for layer in pd for p in layer], dout.to(dtype))
    return scores.detach(), out.detach(), grads


def module_against_reference(dev, num_hidden, shape, top_k, seed):
    N, C, T, V = shape
    torch.manual_seed(seed)
    g = torch.Generator().manual_seed(seed)
    x, dout = torch.randn(N, C, T, V, generator=g), torch.randn(N, C, top_k, V, generator=g)
    m = TemporalSampler(num_hidden, top_k=top_k)
    xg = x.to(dev).requires_grad_(True)
    out = m(xg, True)
    assert out.shape == (N, C, top_k, V)
    names = [n for n, _ in m.named_parameters()]
    widths, F = list(num_hidden) + [1], V * C
    for i, u in enumerate(widths):
        assert names[3 * i:3 * i + 3] == ["lstm_model.%d.%s" % (i, s) for s in ("kernel", "recurrent_kernel", "bias")]
        layer = m.lstm_model[i]
        assert tuple(layer.kernel.shape) == (F, 4 * u) and tuple(layer.recurrent_kernel.shape) == (u, 4 * u) and tuple(layer.bias.shape) == (4 * u,)
        assert torch.equal(layer.bias.detach().cpu(), torch.cat([torch.zeros(u), torch.ones(u), torch.zeros(2 * u)]))
        F = u
    out.backward(dout.to(dev))
    torch.cuda.synchronize()
    idx, scores = m.last_indices.cpu(), m.last_scores.cpu()
    # (b) the selection is the stable descending top-k of the device's own scores
    assert torch.equal(idx.long(), R.stable_topk(scores, top_k)[1]), "idx is not the stable top-k of the device's scores"
    params = [tuple(p.detach().cpu() for p in (l.kernel, l.recurrent_kernel, l.bias)) for l in m.lstm_model]
    s64, o64, g64 = _reference_run(x, params, top_k, idx, dout, torch.float64)
    s32, o32, g32 = _reference_run(x, params, top_k, idx, dout, torch.float32)
    tag = "%s %s" % (num_hidden, shape)
    within(tag + " scores", scores, s64, s32)                             # (a)
    within(tag + " out", out, o64, o32)                                   # (c)
    got = [xg.grad] + [p.grad for p in m.parameters()]                    # (d)
    for name, a, b, b32 in zip(["dx"] + names, got, g64, g32):
        assert a is not None and a.shape == b.shape, name
        within(tag + " grad " + name, a, b, b32)
    return m, xg, out


@pytest.mark.parametrize("num_hidden,shape,top_k", [([5], (3, 2, 9, 5), 4), ([64, 20], (5, 3, 37, 25), 20)])
def test_module_end_to_end(dev, num_hidden, shape, top_k):
    m, xg, out = module_against_reference(dev, num_hidden, shape, top_k, seed=5)
    # a state_dict round trip reproduces the output bitwise; so does the inference form (nothing saved)
    m2 = TemporalSampler(num_hidden, top_k=top_k)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2(xg.detach(), False), out)
    with torch.no_grad():
        assert torch.equal(m(xg, True), out)


def test_module_at_the_reference_shape(dev):
    module_against_reference(dev, [64], (2, 3, 300, 25), 200, seed=6)


# ---------------------------------------------------------------------------------------------- 8. argument errors
def test_argument_errors_raise_before_any_launch(dev):
    m = TemporalSampler([5], top_k=4)
    good = torch.randn(2, 3, 9, 5)
    for bad in (good, good.double().to(dev), good.to(dev).transpose(2, 3), good.to(dev)[0], good.to(dev)[:, :, :3]):
        with pytest.raises(ValueError):
            m(bad, True)
    with pytest.raises(ValueError):
        m(torch.randn(2, 3, 3, 5, device=dev), True)            # top_k > T
    with pytest.raises(ValueError):
        m(torch.randn(1, 1, 2049, 1, device=dev), True)
    assert m.lstm_model[0].kernel is None, "a rejected call built the parameters"
    with pytest.raises(ValueError):
        TemporalSampler([129])
    with pytest.raises(ValueError):
        TemporalSampler([64, 200], top_k=3)
