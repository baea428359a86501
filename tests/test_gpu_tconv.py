"""GPU: TemporalConv (csrc/tconv.hip through the C ABI, sar_amd.ops, and models.tcn.TemporalConv) against the float64 restatement
tests/tconv_reference.py over the cases of tests/tconv_cases.py.

Each of the three kernels runs on its own on outputs pre-filled with NaN (every element has to be written), then the wrappers of
sar_amd.ops, then the module under autograd (out, x.grad, kernel.grad, bias.grad).  ST-GCN's own shapes are also compared with the in-tree
9-tap kernels (ops.conv_gemm / ops.conv_wgrad) on the same tensors, k = 1 with ops.conv1x1_fwd on the even frames.

Tolerance (the rule of tests/test_gpu_tattn.py): norm-wise relative error (tests/util.rel_err) below TOL = 2e-5; a quantity that misses TOL
is judged against 8x the distance of the float32 run of the SAME restatement (CPU) from float64, which tests/test_tconv_reference.py
keeps below TOL for every case.  Both numbers are printed.

Worst errors observed on MI355X per quantity: profiles/tconv.txt."""
import pytest
import torch

import tconv_cases as K
import tconv_reference as R
from util import from_cn, rel_err, to_cn

pytestmark = pytest.mark.gpu

TOL = 2e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def judge(name, got, ref64, ref32):
    e, band = rel_err(got, ref64), rel_err(ref32, ref64)
    print("%-6s engine %.3e, float32 restatement %.3e from float64" % (name, e, band))
    return None if (e < TOL or e <= 8 * band) else (e, band)


def assert_all(pairs):
    bad = {k: v for k, v in pairs.items() if v is not None}
    assert not bad, "(engine error, float32 band) beyond TOL and 8x the band: %s" % bad


def judge_case(case, got):
    _, r64, r32 = K.reference(case)
    for q in K.QUANTITIES:
        assert bool(torch.isfinite(got[q]).all()), "%s: an element was not written" % q
    assert_all({q: judge(q, got[q].reshape(r64[q].shape), r64[q], r32[q]) for q in K.QUANTITIES})


def f32(t, dev):
    return t.to(torch.float32).to(dev).contiguous()


def geometry(case):
    N, C, M, T, V, k, d, s, padding = case
    return R.geometry(T, k, s, d, padding)


def nan(dev, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=dev)


def cn_view(X, N, T, V):
    """the (N, C, T, V) view of the live columns of a CN matrix [C][ld]: s_n = T V, s_c = ld"""
    return X[:, :N * T * V].view(X.shape[0], N, T, V).permute(1, 0, 2, 3)


def kernels(dev, case, x=None, W=None, bias=None, dout=None, views=None):
    """the three entry points one at a time through the C ABI on NaN-filled outputs -> dict of out, dx, dW, dbias (and the slabs).
    views = (x, dout, out, dx) replaces the NCHW tensors by strided views (out and dx NaN-filled by the caller)."""
    from sar_amd import _lib as L
    from sar_amd._lib import check, ptr, stream_ptr
    N, C, M, T, V, k, d, s, _ = case
    T_out, pad = geometry(case)
    inputs = K.reference(case)[0]
    x, W, b, dout = (f32(t, dev) if g is None else g for t, g in zip(inputs, (x, W, bias, dout)))
    lib, st = L.load(), stream_ptr()
    out, dx = nan(dev, N, M, T_out, V), nan(dev, N, C, T, V)
    if views is not None:
        x, dout, out, dx = views
    st4 = lambda t: (t.stride(0), t.stride(1))
    Wt = nan(dev, k, M, C)
    check(lib.sar_transpose_f32(ptr(W), ptr(Wt), k, C, M, st), "transpose")
    size, nslab = k * C * M + M, lib.sar_tconv_wgrad_slabs(N, C, M, T_out, V)
    slab, flat = nan(dev, nslab, size), nan(dev, size)
    check(lib.sar_tconv_fwd_f32(ptr(x), *st4(x), ptr(W), ptr(b), N, C, M, T, T_out, V, k, d, s, pad, ptr(out), *st4(out), st), "fwd")
    check(lib.sar_tconv_bwd_data_f32(ptr(dout), *st4(dout), ptr(Wt), N, C, M, T, T_out, V, k, d, s, pad, ptr(dx), *st4(dx), st), "bwd_data")
    check(lib.sar_tconv_wgrad_f32(ptr(x), *st4(x), ptr(dout), *st4(dout), N, C, M, T, T_out, V, k, d, s, pad, ptr(slab), nslab, st), "wgrad")
    check(lib.sar_slab_reduce_f32(ptr(slab), nslab, size, size, ptr(flat), st), "slab_reduce")
    torch.cuda.synchronize()
    return dict(out=out, dx=dx, dW=flat[:k * C * M].view(k, 1, C, M), dbias=flat[k * C * M:], slab=slab, nslab=nslab)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_each_kernel_matches_the_float64_restatement(dev, case):
    got = kernels(dev, case)
    assert bool(torch.isfinite(got["slab"]).all()), "an element of a slab was not written"
    judge_case(case, got)


def test_the_slab_case_has_two_slabs(dev):
    assert kernels(dev, K.TWO_SLABS)["nslab"] == 2 and kernels(dev, K.PLAIN)["nslab"] == 1


def run_ops(dev, case, bias=True):
    from sar_amd import ops
    N, C, M, T, V, k, d, s, _ = case
    T_out, pad = geometry(case)
    x, W, b, dout = (f32(t, dev) for t in K.reference(case)[0])
    out = ops.tconv_forward(x, W, b if bias else None, s, d, pad, T_out)
    dx = ops.tconv_backward_data(dout, W, T, s, d, pad)
    dW, db = ops.tconv_wgrad(x, dout, k, s, d, pad)
    torch.cuda.synchronize()
    return dict(out=out, dx=dx, dW=dW, dbias=db)


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_ops_match_the_float64_restatement(dev, case):
    got = run_ops(dev, case)
    judge_case(case, got)
    raw = kernels(dev, case)
    for q in K.QUANTITIES:
        assert torch.equal(got[q], raw[q]), "%s: the wrapper is not the kernel" % q


def module(dev, case, use_bias=True):
    from models.tcn import TemporalConv
    N, C, M, T, V, k, d, s, padding = case
    _, W, b, _ = K.reference(case)[0]
    m = TemporalConv(M, k, stride=s, dilation=d, padding=padding, use_bias=use_bias)
    m.build(C, dev)
    with torch.no_grad():
        m.kernel.copy_(f32(W, dev))
        if use_bias:
            m.bias.copy_(f32(b, dev))
    return m


@pytest.mark.parametrize("case", K.CASES, ids=K.case_id)
def test_module_matches_the_float64_restatement(dev, case):
    x, _, _, dout = (f32(t, dev) for t in K.reference(case)[0])
    m = module(dev, case)
    x.requires_grad_(True)
    out = m(x)
    out.backward(dout)
    torch.cuda.synchronize()
    assert set(n for n, _ in m.named_parameters()) == {"kernel", "bias"} and m.kernel.shape == (case[5], 1, case[1], case[2])
    judge_case(case, dict(out=out.detach(), dx=x.grad, dW=m.kernel.grad, dbias=m.bias.grad))


def test_fresh_module_initialises_like_the_other_layers(dev):
    from models.tcn import TemporalConv
    torch.manual_seed(0)
    m = TemporalConv(64, 5, dilation=2)
    out = m(torch.randn(2, 32, 20, 25, device=dev))
    assert out.shape == (2, 64, 20, 25) and bool((m.bias == 0).all())
    std = (2.0 / (5 * 64)) ** 0.5          # VarianceScaling(2, fan_out): the receptive field times the filters
    assert abs(m.kernel.std().item() - std) < 0.1 * std and m.kernel.abs().max().item() <= 2 * std / .87962566103423978 + 1e-6
    m2 = TemporalConv(64, 5, dilation=2)
    m2.load_state_dict(m.state_dict())
    assert torch.equal(m2.kernel, m.kernel) and torch.equal(m2(torch.ones(1, 32, 7, 3, device=dev)), m(torch.ones(1, 32, 7, 3, device=dev)))


# ---- the in-tree kernels on the same tensors

@pytest.mark.parametrize("case", [K.STGCN_S1, K.STGCN_S2], ids=K.case_id)
def test_nine_taps_agree_with_the_specialised_kernels(dev, case):
    from sar_amd import _lib as L
    from sar_amd import ops
    N, C, M, T, V, k, d, s, _ = case
    T_out, pad = geometry(case)
    x, W, b, dout = (f32(t, dev) for t in K.reference(case)[0])
    got = run_ops(dev, case)
    X, D = to_cn(x), to_cn(dout)
    geo = dict(B=N, V=V, T_src=T, T_out=T_out, Kc=C, M=M, taps=9, stride=s, pad=pad)
    out = torch.empty((M, N * T_out * V), device=dev)
    ops.conv_gemm(L.SAR_CONV_TEMPORAL, X, out, W, C * M, M, bias=b, split=None, **geo)
    Wt = torch.empty((9, M, C), device=dev)
    ops.transpose(W, Wt, 9, C, M)
    dx = torch.empty((C, N * T * V), device=dev)
    ops.conv_gemm(L.SAR_CONV_TEMPORAL, D, dx, Wt, M * C, C, B=N, V=V, T_src=T_out, T_out=T, Kc=M, M=C, taps=9, stride=s, pad=pad, transposed=True,
                  split=None)
    flat = torch.empty(9 * C * M + M, device=dev)
    ops.conv_wgrad(L.SAR_CONV_TEMPORAL, X, D, flat, w_stride_tap=C * M, w_stride_c=M, wsize=9 * C * M, bsize=M, split=None, **geo)
    torch.cuda.synchronize()
    for name, mine, theirs in (("out", got["out"], from_cn(out, N, T_out, V)), ("dx", got["dx"], from_cn(dx, N, T, V)),
                               ("dW", got["dW"], flat[:9 * C * M].view(9, 1, C, M)), ("dbias", got["dbias"], flat[9 * C * M:])):
        e = rel_err(mine, theirs)
        print("%-6s %.3e from the 9-tap kernel" % (name, e))
        assert e < TOL, (name, e)


def test_one_tap_at_stride_two_agrees_with_the_1x1_product(dev):
    from sar_amd import ops
    case = K.K1_S2
    N, C, M, T, V, k, d, s, _ = case
    T_out, pad = geometry(case)
    x, W, b, _ = (f32(t, dev) for t in K.reference(case)[0])
    assert (T_out, pad) == (5, 0)
    want = ops.conv1x1_fwd(to_cn(x[:, :, ::2].contiguous()), W[0, 0].contiguous(), b, dict(B=N, V=V, T_src=T_out, T_out=T_out))
    got = run_ops(dev, case)["out"]
    e = rel_err(got, from_cn(want, N, T_out, V))
    print("out    %.3e from conv1x1_fwd on the even frames" % e)
    assert e < TOL


# ---- what is launched and what is kept

def count_entry_points(monkeypatch):
    from sar_amd import _lib as L
    lib, seen = L.load(), {}
    for name in ("sar_tconv_fwd_f32", "sar_tconv_bwd_data_f32", "sar_tconv_wgrad_f32"):
        real = getattr(lib, name)

        def counted(*a, _real=real, _name=name):
            seen[_name] = seen.get(_name, 0) + 1
            return _real(*a)
        monkeypatch.setattr(lib, name, counted)
    return seen


def test_no_bias(dev):
    case = K.STRIDE2
    x, _, _, dout = (f32(t, dev) for t in K.reference(case)[0])
    _, r64, r32 = K.reference(case)
    bias64 = K.reference(case)[0][2].view(1, -1, 1, 1)
    m = module(dev, case, use_bias=False)
    assert [n for n, _ in m.named_parameters()] == ["kernel"]
    x.requires_grad_(True)
    out = m(x)
    out.backward(dout)
    got = dict(out=out.detach(), dx=x.grad, dW=m.kernel.grad)
    assert_all({q: judge(q, got[q], r64[q] - (bias64 if q == "out" else 0), r32[q] - (bias64.float() if q == "out" else 0)) for q in got})
    assert torch.equal(run_ops(dev, case, bias=False)["out"], out.detach())


def test_backward_launches_only_what_is_asked_for(dev, monkeypatch):
    case = K.PLAIN
    x, _, _, dout = (f32(t, dev) for t in K.reference(case)[0])
    m = module(dev, case)
    seen = count_entry_points(monkeypatch)
    m(x).backward(dout)                                  # x needs no gradient
    assert seen == {"sar_tconv_fwd_f32": 1, "sar_tconv_wgrad_f32": 1} and x.grad is None and m.kernel.grad is not None
    seen.clear()
    m.kernel.requires_grad_(False)
    m.bias.requires_grad_(False)
    xg = x.clone().requires_grad_(True)
    m(xg).backward(dout)                                 # only x does
    assert seen == {"sar_tconv_fwd_f32": 1, "sar_tconv_bwd_data_f32": 1}
    assert torch.equal(xg.grad, run_ops(dev, case)["dx"])


def test_nothing_is_saved_without_a_gradient(dev):
    case = K.PLAIN
    x = f32(K.reference(case)[0][0], dev)
    m = module(dev, case)
    packed = []

    def pack(t):
        packed.append(t)
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        with torch.no_grad():
            out = m(x)
        assert out.grad_fn is None and not out.requires_grad and packed == []
        m.kernel.requires_grad_(False)
        m.bias.requires_grad_(False)
        out = m(x)                                       # grad mode, but nothing requires a gradient
        assert not out.requires_grad and packed == []
        m.kernel.requires_grad_(True)
        out2 = m(x)
        assert out2.requires_grad and len(packed) == 2   # x and the kernel
    assert torch.equal(out, out2)


# ---- determinism, batch independence, CN views

@pytest.mark.parametrize("case", [K.STRIDE2, K.STGCN_S2, K.TWO_SLABS], ids=K.case_id)
def test_two_runs_are_bitwise_equal(dev, case):
    a, b = kernels(dev, case), kernels(dev, case)
    for q in K.QUANTITIES + ("slab",):
        assert torch.equal(a[q], b[q]), q


def test_a_sample_does_not_depend_on_its_batch(dev):
    """every 4-sample slice of out and dx of the 16-sample run is bitwise the N = 4 run on that slice, the slice a view of the batch"""
    case = K.SLICE
    n = K.SLICE_N
    x, W, b, dout = (f32(t, dev) for t in K.reference(case)[0])
    whole = kernels(dev, case)
    small = (n,) + case[1:]
    T_out, _ = geometry(case)
    for i in range(0, case[0], n):
        xs, ds = x[i:i + n], dout[i:i + n]
        assert xs.data_ptr() == x.data_ptr() + 4 * i * x.stride(0)
        got = kernels(dev, small, views=(xs, ds, nan(dev, n, case[2], T_out, case[4]), nan(dev, n, case[1], case[3], case[4])), W=W, bias=b)
        assert torch.equal(got["out"], whole["out"][i:i + n]) and torch.equal(got["dx"], whole["dx"][i:i + n]), "samples %d.." % i


@pytest.mark.parametrize("case", K.GUARDED + [K.STGCN_S2], ids=K.case_id)
def test_a_cn_view_gives_the_bits_of_the_nchw_run(dev, case):
    """x, dout, out and dx as views of CN matrices [C][ld] with ld > N T V (s_n = T V, s_c = ld): all three kernels, bit for bit"""
    N, C, M, T, V, k, d, s, _ = case
    T_out, _ = geometry(case)
    x, W, b, dout = (f32(t, dev) for t in K.reference(case)[0])
    want = kernels(dev, case)
    X, D = nan(dev, C, N * T * V + 7), nan(dev, M, N * T_out * V + 3)
    X[:, :N * T * V], D[:, :N * T_out * V] = to_cn(x), to_cn(dout)
    O_, G = nan(dev, M, N * T_out * V + 5), nan(dev, C, N * T * V + 1)
    views = tuple(cn_view(t, N, tt, V) for t, tt in ((X, T), (D, T_out), (O_, T_out), (G, T)))
    assert (views[0].stride(0), views[0].stride(1)) == (T * V, N * T * V + 7)
    got = kernels(dev, case, views=views)
    for q in K.QUANTITIES:
        assert torch.equal(got[q], want[q]), q
    assert bool(torch.isnan(O_[:, N * T_out * V:]).all()) and bool(torch.isnan(G[:, N * T * V:]).all()), "the margin of a CN matrix was written"
    # and through the wrappers, which take the same views
    from sar_amd import ops
    _, pad = geometry(case)
    assert torch.equal(ops.tconv_forward(views[0], W, b, s, d, pad, T_out), want["out"])
    assert torch.equal(ops.tconv_backward_data(views[1], W, T, s, d, pad), want["dx"])
    assert torch.equal(ops.tconv_wgrad(views[0], views[1], k, s, d, pad)[0], want["dW"])
