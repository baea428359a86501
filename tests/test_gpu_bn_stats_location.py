"""GPU: BatchNorm batch statistics of data that is NOT centred -- the LOCATION of the data, where every other parity test draws zero-mean
inputs.  data_bn normalises the raw coordinates per (joint, coordinate) channel; a depth channel of a still subject sits tens of
standard deviations from 0, where var = S2/n - mean^2 from float32 sums loses 2^-24 (mean/std)^2 of the variance.  The engines
therefore run sar_data_bn_stats_pivot_f32 (two passes; a channel within 2 standard deviations of 0 keeps pivot 0 and its first-pass sums,
bit for bit the one-pass statistics: the last test) and sar_bn_finalize_pivot_f32; tests/bn_stats_reference.py restates both
orders in numpy float32 and tests/test_bn_stats_reference.py validates every 2e-5 bar below at half its value.

The error of a channel is max |y - y64| / max |y64| over its samples, y64 the float64 normalised output of the same float32 clip.

data_bn, joint / bone / joint_motion / bone_motion with the NTU bone pairs, (N, C, T, V, M) = (8, 3, 300, 25, 1) and (4, 3, 300, 25, 2)
(the loss grows with the length of the sums, so T stays 300), ONE clip per shape carrying every case in its 75 channels:
joints 0..19 cycle mean/std 0, 8, 64, 256 over their coordinates (white noise and trajectories, z-scored in float64); joints 22..24
are constant (3.2, -0.7, 0.05 in the three coordinates, times 1, 2, 3); joint 21 is exactly zero; joint 20 has a second body that is zero
in every clip.  Every channel is judged by the ratio its STREAM reaches (a bone or motion stream differences the offset away):
    reached mean/std <= 64    2e-5, the project's per-kernel bar; the CN8 apply by util.assert_bf16_close
    above (up to 256)         4 x the worst error of the two-pass-plus-apply restatement over the same channels; value printed
                              (measured on an MI355X, joint stream: 7.4e-6 at M = 1, 3.9e-6 at M = 2, bit for bit the
                              restatement's figures; it is the float32 rounding of `shift`)
    mean                      within 2e-5 std of float64; rstd within 2e-5 of float64; moving statistics at 1e-5
    zero channel              mean, moving mean and variance exactly 0, scale = gamma / sqrt(eps) to one float32 rounding
    constant channel          finite, var >= 0 (rstd <= 1/sqrt(eps)), rstd within 2e-5 of 1/sqrt(eps), y within 2e-5 * max |beta| of beta
                              (the values are small because y = x * scale + shift rounds shift = beta - 31.6 gamma x to float32:
                              2^-24 * 31.6 * 3 * 3.2 = 1.8e-5 of a max |beta| of at least 1 is what the apply pass alone may cost)
Backward (sar_data_bn_bwd_reduce_f32 / _cn8, sar_bn_bwd_finalize_f32, sar_data_bn_bwd_apply_f32 / _cn8) on the same clips against
float64 autograd at 1e-4 (tests/test_gpu_input_grad.py), per channel.  The bone and motion streams must not notice 2^k added to a
coordinate whose values stay exactly representable: bitwise.

With the one-pass order forced back (measured): 2.0e-4 / 3.2e-4 at mean/std 64, 2.0e-3 / 3.8e-3 at 256, rstd of a constant channel off
by up to 1.5 %, and the backward and engine cases below fail; mean/std 0 and 8 pass either way.

The BatchNorm-backward apply passes sar_affine2_f32, sar_bn_add_relu_bwd_apply_f32 and sar_gin_bwd_apply_f32 form k2 * u + k3, a difference of terms `ratio`
times larger than the result; three roundings (k2, k3 and the fma) bound the error by 4 * 2^-24 * (1 + ratio) of max |result|
(asserted at ratios 0, 16 and 64; sar_gin_bwd_apply_f32 too).

The convolution epilogues (SAR_EPI_STATS; fp32, split and CN8), conv2d_gemm, the dense-adjacency contractions, gin_sum_fwd and the
CN8 backward apply passes are further down, with their own notes.  pgc.hip, gpool.hip and pgpool.hip leave no (sum, sum of squares)
partials.

Engine level: the three-block STGCN at T = 40 on single-body and two-body clips with 3.3 added to the depth coordinate and 0.3 to the
height (mean/std about 27): fp32 and f32_split against the mask-conditioned float64 oracle exactly as
tests/test_gpu_stgcn_model.py::_compare, at its TOL; bf16 by the cosine of the logits against fp32."""
import functools

import numpy as np
import pytest
import torch

import bn_stats_reference as R
import data_bn_dx_reference as DX
from util import assert_bf16_close, cn8_units, cn8_values

pytestmark = pytest.mark.gpu
BAR = R.BAR
EPS = float(np.float32(1e-3))
MOMENTUM = float(np.float32(0.99))
SHAPES = [(8, 3, 300, 25, 1), (4, 3, 300, 25, 2)]
STREAMS = list(DX.STREAMS)
CONST_JOINTS, ZERO_JOINT, BODY_JOINT = (22, 23, 24), 21, 20
CONST_VALUES = (3.2, -0.7, 0.05)
RATIOS = (0, 8, 64, 256)
GROUPS = ["ratio0", "ratio8", "ratio64", "ratio256", "constant", "zero", "second_body_zero"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need a MI355X"
    from sar_amd import _lib
    _lib.load()
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _clip(shape):
    """the clip of one shape (float32, never modified), gamma, beta, and the group of every JOINT-stream channel"""
    N, C, T, V, M = shape
    x = np.zeros(shape, np.float32)
    group = {}
    for v in range(20):
        for c in range(C):
            ratio = RATIOS[(v + c) % 4]
            build = R.white if (v // 4) % 2 == 0 else R.trajectory
            x[:, c, :, v, :] = build(1000 + v * C + c, 1, N, T, M, float(ratio))[0]
            group[v * C + c] = "ratio%d" % ratio
    for i, v in enumerate(CONST_JOINTS):
        for c in range(C):
            x[:, c, :, v, :] = np.float32(CONST_VALUES[c] * (i + 1))
            group[v * C + c] = "constant"
    for c in range(C):
        group[ZERO_JOINT * C + c] = "zero"
        if M >= 2:
            x[:, c, :, BODY_JOINT, :] = R.second_body_zero(2000 + c, 1, N, T, M, 8.0)[0]
            group[BODY_JOINT * C + c] = "second_body_zero"
        else:
            x[:, c, :, BODY_JOINT, :] = R.white(2000 + c, 1, N, T, M, 8.0)[0]
            group[BODY_JOINT * C + c] = "ratio8"
    rng = np.random.default_rng(11)
    gamma = (0.5 + rng.random(V * C)).astype(np.float32)
    beta = rng.standard_normal(V * C).astype(np.float32)
    return torch.from_numpy(x), torch.from_numpy(gamma), torch.from_numpy(beta), group


def _channels(val):
    """(N, C, T, V, M) -> (V*C, N*T*M) numpy, channel ch = v*C + c"""
    N, C, T, V, M = val.shape
    return val.permute(3, 1, 0, 2, 4).reshape(V * C, N * T * M).numpy()


def _out_channels(out, shape):
    """CN rows [C][((n*M+m)*T+t)*V+v] -> (V*C, N*T*M) in the sample order of _channels"""
    N, C, T, V, M = shape
    return DX.cn_to_clip(out.double(), N, C, T, V, M).permute(3, 1, 0, 2, 4).reshape(V * C, N * T * M).numpy()


@functools.lru_cache(maxsize=None)
def _reference(shape, stream):
    """float64 statistics and output of the stream's channels, the ratio each reaches, and the restatement's error per channel"""
    x, gamma, beta, _ = _clip(shape)
    N, C, T, V, M = shape
    bone, motion = DX.STREAMS[stream]
    parent = DX.ntu_parent() if bone else None
    val32 = DX.stream_values(x, parent, motion)                      # float32 operations, as the kernel forms them
    flat = _channels(val32).astype(np.float64)
    st = R.stats64(flat, EPS, gamma.double().numpy(), beta.double().numpy())
    y64 = R.normalised64(flat, st)
    std = np.sqrt(st["var"])
    reached = np.abs(st["mean"]) / np.where(std > 0, std, 1.0)          # (meaningless for a constant channel: never read there)
    const = (flat == flat[:, :1]).all(axis=1)
    # the restatement of what the GPU runs: two passes over each clip's (T, M) samples, then the fma apply
    per_clip = val32.permute(3, 1, 0, 2, 4).reshape(V * C, N, T, M).numpy()
    rst = R.data_bn_two_pass(per_clip, V, eps=EPS, gamma=gamma.double().numpy(), beta=beta.double().numpy())
    yr = R.apply_fma(per_clip.reshape(V * C, -1), rst["scale"], rst["shift"])
    with np.errstate(invalid="ignore", divide="ignore"):
        restated = np.abs(yr - y64).max(axis=1) / np.abs(y64).max(axis=1)
    return dict(parent=parent, motion=motion, flat=flat, st=st, y64=y64, std=std, reached=reached, const=const,
                zero=(flat == 0).all(axis=1), restated=restated)


@functools.lru_cache(maxsize=None)
def _forward(shape, stream):
    """the GPU pipeline of one (shape, stream), once: stats (two passes) -> finalize -> apply (float32 and CN8)"""
    from sar_amd import ops, ops8
    dev = torch.device("cuda:0")
    x, gamma, beta, _ = _clip(shape)
    N, C, T, V, M = shape
    ref = _reference(shape, stream)
    parent = None if ref["parent"] is None else torch.from_numpy(ref["parent"]).to(dev)
    xg = x.to(dev)
    z = lambda: torch.zeros(V * C, device=dev)
    part, pivot = torch.empty((V * C, N, 2), device=dev), z()
    mean, rstd, scale, shift, rm, rv = z(), z(), z(), z(), z(), torch.ones(V * C, device=dev)
    ops.data_bn_stats(xg, parent, part, ref["motion"], pivot=pivot)
    ops.bn_finalize(part, N, V * C, N * M * T, EPS, MOMENTUM, False, gamma.to(dev), beta.to(dev), rm, rv, mean, rstd, scale, shift,
                    pivot=pivot)
    n = N * M * T * V
    out = torch.empty((C, n), device=dev)
    ops.data_bn_apply(xg, parent, scale, shift, out, ref["motion"])
    h8 = ops8.empty(C, n, dev)
    ops8.data_bn_apply(xg, parent, scale, shift, h8, ref["motion"])
    torch.cuda.synchronize()
    y = _out_channels(out.cpu(), shape)
    y8 = _out_channels(cn8_values(h8.cpu(), C), shape)
    with np.errstate(invalid="ignore", divide="ignore"):
        err = np.abs(y - ref["y64"]).max(axis=1) / np.abs(ref["y64"]).max(axis=1)
    c = lambda t: t.cpu().double().numpy()
    return dict(y=y, y8=y8, err=err, mean=c(mean), rstd=c(rstd), scale=c(scale), shift=c(shift), rm=c(rm), rv=c(rv),
                dev=dict(x=xg, parent=parent, mean=mean, rstd=rstd, gamma=gamma.to(dev)))


def _worst(what, chans, values, bars):
    i = int(np.argmax(values / bars))
    return "%s: worst channel %d (joint %d, coordinate %d): %.3e against %.3e" % (what, chans[i], chans[i] // 3, chans[i] % 3,
                                                                                 values[i], bars[i])


def _judge(shape, stream, chans, what):
    """every check of the channels `chans` of one forward run, each by the ratio its stream reaches"""
    ref, got = _reference(shape, stream), _forward(shape, stream)
    x, gamma, beta, _ = _clip(shape)
    st, g64, b64 = ref["st"], gamma.double().numpy(), beta.double().numpy()
    chans = np.asarray(chans)
    rs_eps = 1.0 / np.sqrt(EPS)
    for k in ("y", "y8", "mean", "rstd", "scale", "shift", "rm", "rv"):
        assert np.isfinite(got[k][chans]).all(), "%s %s: %s is not finite" % (what, stream, k)
    assert (got["rstd"][chans] <= rs_eps * (1 + 2.0 ** -23)).all(), "%s: var < 0" % what
    zero, const = chans[ref["zero"][chans]], chans[ref["const"][chans] & ~ref["zero"][chans]]
    live = chans[~ref["const"][chans]]
    # ---- zero channels: exact
    if len(zero):
        assert (got["mean"][zero] == 0).all() and (got["rm"][zero] == 0).all(), "%s: the mean of a zero channel" % what
        assert (got["rv"][zero] == float(np.float32(MOMENTUM))).all(), "%s: the variance of a zero channel is not exactly 0" % what
        want = g64[zero] * rs_eps
        assert (np.abs(got["scale"][zero] - want) <= 2.0 ** -24 * np.abs(want)).all(), "%s: scale of a zero channel" % what
        assert (np.abs(got["y"][zero] - b64[zero][:, None]) <= 2.0 ** -24 * np.abs(b64[zero][:, None])).all()
    # ---- constant channels
    if len(const):
        rel = np.abs(got["rstd"][const] / rs_eps - 1.0)
        print(_worst("%s %s rstd of a constant channel" % (what, stream), const, rel, np.full(len(const), BAR)))
        assert (rel <= BAR).all(), _worst("rstd of a constant channel", const, rel, np.full(len(const), BAR))
        dev_ = np.abs(got["y"][const] - b64[const][:, None]).max(axis=1)
        bar = np.full(len(const), BAR * np.abs(b64).max())
        print(_worst("%s %s constant channel, |y - beta|" % (what, stream), const, dev_, bar))
        assert (dev_ <= bar).all(), _worst("constant channel, |y - beta|", const, dev_, bar)
    # ---- channels with a variance: the normalised output by the ratio reached
    if len(live):
        reached, err = ref["reached"][live], got["err"][live]
        far = reached > 64.01
        bars = np.full(len(live), BAR)
        if far.any():
            bars[far] = 4.0 * ref["restated"][live][far].max()
            print("%s %s: mean/std %.0f..%.0f: GPU %.3e, restatement %.3e (bar 4 x)" % (
                what, stream, reached[far].min(), reached[far].max(), err[far].max(), ref["restated"][live][far].max()))
        print("%s %s: mean/std reached %.1f..%.1f; " % (what, stream, reached.min(), reached.max()) +
              _worst("output", live, err, bars) + "; restatement %.3e" % ref["restated"][live].max())
        assert (err <= bars).all(), _worst("%s %s output" % (what, stream), live, err, bars)
        near = live[~far]
        if len(near):
            assert_bf16_close(torch.from_numpy(got["y8"][near]), torch.from_numpy(ref["y64"][near]), "%s %s CN8 apply" % (what, stream))
        merr = np.abs(got["mean"][live] - st["mean"][live]) / ref["std"][live]
        assert (merr <= BAR).all(), _worst("%s %s mean, in std" % (what, stream), live, merr, np.full(len(live), BAR))
        rerr = np.abs(got["rstd"][live] / st["rstd"][live] - 1.0)
        assert (rerr <= BAR).all(), _worst("%s %s rstd" % (what, stream), live, rerr, np.full(len(live), BAR))
    # ---- moving statistics (data_bn: the biased variance) at the existing 1e-5, PER CHANNEL: a channel far from 0 sets no bar for one
    # near it.  A mean is known to a fraction of its channel's std (a z-scored channel has a mean of 1e-11), so the scale of a
    # channel's moving mean is what the update adds for a mean of one std beside the mean itself; a zero or constant channel (std 0,
    # variance 0) has the first term alone, and its moving variance is 0.99 exactly up to the rounding of var ~ 0
    mm, mv = R.moving_update64(0.0, 1.0, st["mean"][chans], st["var"][chans], x[:, 0, :, 0, :].numel(), MOMENTUM, unbiased=False)
    mscale = np.abs(mm) + (1.0 - MOMENTUM) * ref["std"][chans]
    merr = np.abs(got["rm"][chans] - mm)
    assert (merr <= 1e-5 * mscale + 1e-30).all(), _worst("%s %s moving mean" % (what, stream), chans, merr, 1e-5 * mscale + 1e-30)
    verr = np.abs(got["rv"][chans] - mv)
    assert (verr <= 1e-5 * np.abs(mv)).all(), _worst("%s %s moving variance" % (what, stream), chans, verr, 1e-5 * np.abs(mv))


# a single body has no second body to zero: joint 20 is one more channel at mean/std 8 there
@pytest.mark.parametrize("shape,group", [(s, g) for s in SHAPES for g in GROUPS if not (g == "second_body_zero" and s[4] == 1)],
                         ids=lambda v: v if isinstance(v, str) else "M%d" % v[4])
def test_data_bn_joint_stream(dev, shape, group):
    chans = [ch for ch, g in _clip(shape)[3].items() if g == group]
    assert chans
    if group.startswith("ratio"):
        reached = _reference(shape, "joint")["reached"][chans]
        assert np.abs(reached - int(group[5:])).max() < 1e-3, "the float64 ratio reached: %s" % reached
    _judge(shape, "joint", chans, group)


@pytest.mark.parametrize("stream", STREAMS[1:])
@pytest.mark.parametrize("shape", SHAPES, ids=["M1", "M2"])
def test_data_bn_bone_and_motion_streams(dev, shape, stream):
    _judge(shape, stream, list(range(75)), "all channels")


@pytest.mark.parametrize("variant", ["f32", "cn8"])
@pytest.mark.parametrize("stream", STREAMS)
@pytest.mark.parametrize("shape", SHAPES, ids=["M1", "M2"])
def test_data_bn_backward_against_float64_autograd(dev, shape, stream, variant):
    from sar_amd import ops, ops8
    N, C, T, V, M = shape
    x, gamma, beta, _ = _clip(shape)
    ref, fw = _reference(shape, stream), _forward(shape, stream)
    n = N * M * T * V
    dh = torch.randn(C, n, generator=torch.Generator().manual_seed(5))
    if variant == "cn8":
        dh = dh.bfloat16().float()
    # float64 autograd through the stream transform and the batch statistics
    x64 = x.double().requires_grad_(True)
    g64, b64 = gamma.double().requires_grad_(True), beta.double().requires_grad_(True)
    val = DX.stream_values(x64, ref["parent"], ref["motion"])
    mean = val.mean(dim=(0, 2, 4), keepdim=True)
    var = val.var(dim=(0, 2, 4), unbiased=False, keepdim=True)
    per = lambda p: p.reshape(V, C).t().reshape(1, C, 1, V, 1)
    y = (val - mean) * torch.rsqrt(var + EPS) * per(g64) + per(b64)
    dx_ref, dg_ref, db_ref = torch.autograd.grad(y, (x64, g64, b64), DX.cn_to_clip(dh.double(), N, C, T, V, M))
    d = fw["dev"]
    part = torch.empty((V * C, N, 2), device=dev)
    z = lambda: torch.zeros(V * C, device=dev)
    dgam, dbet, k1, k2, k3 = z(), z(), z(), z(), z()
    if variant == "cn8":
        dy = cn8_units(dh).to(dev)
        ops8.data_bn_bwd_reduce(d["x"], d["parent"], dy, d["mean"], part, ref["motion"])
    else:
        dy = dh.to(dev)
        ops.data_bn_bwd_reduce(d["x"], d["parent"], dy, d["mean"], part, ref["motion"])
    ops.bn_bwd_finalize(part, N, N * 2, 2, 0, 1, V * C, N * M * T, d["gamma"], d["mean"], d["rstd"], dgam, dbet, k1, k2, k3)
    dx = (ops8 if variant == "cn8" else ops).data_bn_bwd_apply(d["x"], d["parent"], dy, (k1, k2, k3), motion=ref["motion"])
    torch.cuda.synchronize()
    assert torch.isfinite(dx).all()
    got, want = _channels(dx.cpu().double()), _channels(dx_ref)
    scale = np.abs(want).max(axis=1)
    err = np.abs(got - want).max(axis=1) / np.where(scale > 0, scale, 1.0)
    chans = np.arange(V * C)
    print(_worst("%s %s dx" % (stream, variant), chans, err, np.full(V * C, 1e-4)))
    assert (err <= 1e-4).all(), _worst("%s %s dx" % (stream, variant), chans, err, np.full(V * C, 1e-4))
    for name, a, b in (("dgamma", dgam, dg_ref), ("dbeta", dbet, db_ref)):
        a, b = a.cpu().double().numpy(), b.numpy()
        # a constant channel's dgamma is 0 in float64 and a sum of roundings here: judged against the tensor's scale
        assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max(), "%s %s %s: %.3e of %.3e" % (stream, variant, name, np.abs(a - b).max(),
                                                                                         np.abs(b).max())


@pytest.mark.parametrize("stream", STREAMS[1:])
def test_differencing_streams_do_not_see_an_exact_offset(dev, stream):
    """values on a 2^-10 grid below 4 plus 64 stay exactly representable, and every NTU bone has a parent (joint 21 its own)"""
    from sar_amd import ops, ops8
    N, C, T, V, M = 2, 3, 37, 25, 2
    bone, motion = DX.STREAMS[stream]
    parent = torch.from_numpy(DX.ntu_parent()).to(dev) if bone else None
    x = (torch.randn(N, C, T, V, M, generator=torch.Generator().manual_seed(9)).clamp(-3.9, 3.9) * 1024).round() / 1024
    moved = x.clone()
    moved[:, 2] += 64.0
    assert torch.equal((moved[:, 2] - 64.0), x[:, 2])
    gamma, beta = torch.rand(V * C) + 0.5, torch.randn(V * C)
    outs = []
    for clip in (x, moved):
        xg = clip.to(dev)
        z = lambda: torch.zeros(V * C, device=dev)
        part, pivot, mean, rstd, scale, shift = torch.empty((V * C, N, 2), device=dev), z(), z(), z(), z(), z()
        ops.data_bn_stats(xg, parent, part, motion, pivot=pivot)
        ops.bn_finalize(part, N, V * C, N * M * T, EPS, MOMENTUM, False, gamma.to(dev), beta.to(dev), None, None, mean, rstd, scale,
                        shift, pivot=pivot)
        out, h8 = torch.empty((C, N * M * T * V), device=dev), ops8.empty(C, N * M * T * V, dev)
        ops.data_bn_apply(xg, parent, scale, shift, out, motion)
        ops8.data_bn_apply(xg, parent, scale, shift, h8, motion)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (part, pivot, mean, rstd, scale, shift, out, h8.view(torch.int16))])
    for name, a, b in zip(("partials", "pivot", "mean", "rstd", "scale", "shift", "out", "cn8"), *outs):
        same = torch.equal(a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else torch.equal(a, b)
        assert same, "%s: %s changed with the offset" % (stream, name)


# ------------------------------------------------------------------------------------------------ backward apply passes at un-centred u
@pytest.mark.parametrize("n", [2000, 1999], ids=["vec4", "scalar"])
@pytest.mark.parametrize("ratio", [0, 16, 64])
def test_bn_backward_apply_passes_at_uncentred_u(dev, ratio, n):
    """du = k1 dz + k2 u + k3 with k3 = -k2 mean - k1 a: two terms `ratio` times the size of their difference.  The coefficients are
    float64 here and rounded to float32 for the kernel, as sar_bn_bwd_finalize_f32 stores them: the roundings of k2 and k3 and the
    fma bound the error by 4 * 2^-24 * (1 + ratio) of max |result| per channel.  sar_affine2_f32 and both outputs of
    sar_bn_add_relu_bwd_apply_f32 (conv residual)."""
    from sar_amd import ops
    C = 16
    g = torch.Generator().manual_seed(40 + ratio)
    u = torch.randn(C, n, generator=g) + float(ratio)
    r = torch.randn(C, n, generator=g) - float(ratio)
    dy, y = torch.randn(C, n, generator=g), torch.randn(C, n, generator=g)
    k1, k2 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5 for _ in range(2))   # k2 (u - mean) is a full share of the result
    k3 = -k2 * ratio + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    q1, q2 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5 for _ in range(2))
    q3 = q2 * ratio + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    col = lambda t: t.view(-1, 1)
    bound = 4 * 2.0 ** -24 * (1 + ratio)
    d = lambda t: t.float().to(dev)
    k, q = tuple(d(t) for t in (k1, k2, k3)), tuple(d(t) for t in (q1, q2, q3))

    def judge(what, got, want):
        err = ((got.cpu().double() - want).abs().amax(dim=1) / want.abs().amax(dim=1)).numpy()
        print("%s at mean/std %d: %.3e of a bound of %.3e" % (what, ratio, err.max(), bound))
        assert (err <= bound).all(), _worst(what, np.arange(C), err, np.full(C, bound))

    out = torch.empty((C, n), device=dev)
    ops.affine2(d(dy), d(u), k, out)
    torch.cuda.synchronize()
    judge("affine2", out, col(k1) * dy.double() + col(k2) * u.double() + col(k3))
    du, dr, dz = (torch.empty((C, n), device=dev) for _ in range(3))
    ops.bn_add_relu_bwd_apply(d(dy), d(y), d(u), d(r), k, q, du, dr, dz)
    torch.cuda.synchronize()
    dz64 = dy.double() * (y > 0)
    assert torch.equal(dz.cpu().double(), dz64)
    judge("bn_add_relu_bwd_apply du", du, col(k1) * dz64 + col(k2) * u.double() + col(k3))
    judge("bn_add_relu_bwd_apply dr", dr, col(q1) * dz64 + col(q2) * r.double() + col(q3))
    # sar_gin_bwd_apply_f32: K = 1 branch, da = k1 dz + k2 a + k3 with dz = ds where a * scale + shift > 0 (include/sar_hip.h)
    # the gate's scale is a power of two: a * scale is exact, the fma rounds the exact sum, and a rounded non-zero sum keeps its sign,
    # so the float64 gate below is the kernel's gate element for element (no ties to condition on)
    sc = 2.0 ** torch.randint(-1, 2, (C,), generator=g).float()
    sh = (torch.randn(C, generator=g) - float(ratio)) * sc
    da = torch.empty((C, n), device=dev)
    ops.gin_bwd_apply(d(dy), d(u), d(sc), d(sh), k, 1, da)
    torch.cuda.synchronize()
    pre64 = u.double() * col(sc.double()) + col(sh.double())
    assert (pre64 != 0).all() and 0.2 < (pre64 > 0).double().mean() < 0.8
    judge("gin_bwd_apply", da, col(k1) * (dy.double() * (pre64 > 0)) + col(k2) * u.double() + col(k3))


# ------------------------------------------------------------------------------------------------ engine level
ENGINE_BLOCKS = [(64, 1, False), (64, 1, True), (128, 2, True)]


def _offset_clips(M, seed):
    """synthetic clips with every body present, 3.3 added to the depth and 0.3 to the height coordinate: mean/std about 27"""
    from oracle import stgcn as O
    x, y = O.synthetic_batch(4, seed=seed, T=40, M=M, num_classes=10, single_body_frac=0.0)
    x = x.clone()
    x[:, 2] += 3.3
    x[:, 1] += 0.3
    flat = x[:, 2].double()
    print("depth coordinate: mean/std %.1f" % (flat.mean() / flat.std()).item())
    return x, y


@pytest.mark.parametrize("M", [1, 2])
@pytest.mark.parametrize("mode", ["fp32", "f32_split"])
def test_engine_on_uncentred_clips_against_the_float64_oracle(dev, monkeypatch, mode, M):
    """logits, loss, every gradient, the moving statistics and the unconditioned envelope exactly as
    tests/test_gpu_stgcn_model.py::_compare judges them, at its TOL and with its defaults"""
    import sar_amd.stgcn as S
    from test_gpu_stgcn_model import TOL, _compare
    monkeypatch.setattr(S, "DEFAULT_MFMA", mode)         # _compare builds the engine without naming an arithmetic
    x, y = _offset_clips(M, seed=20 + M)
    _, eng, _ = _compare(dev, ENGINE_BLOCKS, N=4, T=40, classes=10, seed=3, tol=TOL, x=x, y=y)
    assert eng.mfma == mode


@pytest.mark.parametrize("M", [1, 2])
def test_bf16_engine_on_uncentred_clips_against_fp32(dev, M):
    """the bounds tests/test_gpu_bf16.py::test_train_step_bf16_close_to_fp32 asserts for centred clips: logits within 2e-2 of the
    fp32 engine's, cosine at least its 0.98"""
    from oracle import stgcn as O
    from sar_amd.stgcn import STGCN
    from util import rel_err
    p = O.randomize_affine(O.init_params(10, seed=0, dtype=torch.float64, blocks=ENGINE_BLOCKS))
    x, y = _offset_clips(M, seed=20 + M)
    out = {}
    for mode in ("fp32", "bf16"):
        eng = STGCN(num_classes=10, device=dev, blocks=ENGINE_BLOCKS, mfma=mode)
        eng.load_params(p)
        logits, _ = eng.loss_and_grad(x.to(dev), y.to(dev))
        torch.cuda.synchronize()
        out[mode] = logits.cpu().double()
    cos = ((out["fp32"] * out["bf16"]).sum() / (out["fp32"].norm() * out["bf16"].norm())).item()
    print("bf16 against fp32 on un-centred clips (M = %d): logits %.3e, cosine %.5f" % (M, rel_err(out["bf16"], out["fp32"]), cos))
    assert cos >= 0.98 and rel_err(out["bf16"], out["fp32"]) < 2e-2


# ------------------------------------------------------------------------------------------------ the convolution epilogues (SAR_EPI_STATS)
# Graph, 9-tap temporal and 1-tap residual forward at their smallest parity shapes widened to 2 050 columns, fp32 and both split
# arithmetics.  The offset is a per-row bias ratio * sigma64(row), sigma64 from a first launch without bias.  The statistics are judged on
# the kernel's OWN output u: y = u * scale + shift formed in float64 against the float64 normalisation of the same u, so the figure is
# the loss of the (sum, sum of squares) partials and of the finalisation alone.  R.CONV_RATIOS (0, 4, 8) are asserted at 2e-5; 16 and 64
# are held to 4 x the restatement (a float32 chain inside each partial of ceil(columns / nparts) columns) and printed.
CONV_CASES = {"graph": dict(B=2, cin=64, f=64, T=41, s=1), "temporal9": dict(B=2, cin=64, f=64, T=41, s=1),
              "residual1": dict(B=2, cin=64, f=128, T=82, s=2)}


def _conv_bias(kind, offset):
    """the operator's bias vector that adds offset[m] to every column of output row m.  The graph operator has 3 f entries, entry
    k f + m weighted by the column sums of adjacency slice k; slice 0 is the identity (column sums 1), so it carries the offset"""
    return torch.cat([offset, torch.zeros(2 * offset.numel())]) if kind == "graph" else offset


def _conv_launcher(dev, kind, arith):
    """(launch(bias) -> (u float32 on the host, partials, nparts), rows, columns) of one producer"""
    from oracle import stgcn as O
    from sar_amd import ops, _lib as L
    from test_gpu_stgcn_kernels import _tables
    from util import to_cn
    c = CONV_CASES[kind]
    B, cin, f, T, s = c["B"], c["cin"], c["f"], c["T"], c["s"]
    g = torch.Generator().manual_seed(len(kind) + 17)
    x = to_cn(torch.randn(B, cin, T, 25, generator=g)).to(dev)
    if kind == "graph":
        W, tables = (torch.randn(1, 1, cin, 3 * f, generator=g) * 0.1).to(dev), _tables(dev)
        To, geo = T, dict(B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f, taps=3, tables=tables)
        mode, strides = L.SAR_CONV_GRAPH, (f, 3 * f)
        ok = ops.split_applicable(mode, 25, cin, f, 3, 1, tables, None, False, 0)
    elif kind == "temporal9":
        W = (torch.randn(9, 1, cin, f, generator=g) * 0.05).to(dev)
        pro = ((1 + 0.2 * torch.randn(cin, generator=g)).to(dev), (0.3 * torch.randn(cin, generator=g)).to(dev))
        To, pad, _ = O.same_pad(T, 9, s)
        geo = dict(B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=9, stride=s, pad=pad, pro=pro, pro_relu=True)
        mode, strides = L.SAR_CONV_TEMPORAL, (cin * f, f)
        ok = ops.split_applicable(mode, 25, cin, f, 9, s, None, pro, False, pad)
    else:
        W = (torch.randn(1, 1, cin, f, generator=g) * 0.1).to(dev)
        To = -(-T // s)
        geo = dict(B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s, pad=0)
        mode, strides = L.SAR_CONV_TEMPORAL, (0, f)
        ok = ops.split_applicable(mode, 25, cin, f, 1, s, None, None, False, 0)
    assert arith is None or ok, "%s: the %s kernel does not take this shape" % (kind, arith)
    n = B * To * 25

    def launch(bias):
        out = torch.empty((f, n), device=dev)
        r = ops.conv_gemm(mode, x, out, W, strides[0], strides[1], bias=_conv_bias(kind, bias).to(dev), epi=L.SAR_EPI_STATS,
                          split=arith, **geo)
        torch.cuda.synchronize()
        return out.cpu(), r[0], r[1]
    return launch, f, n


def _judge_producer(dev, name, launch, f, n, case, ratios, calibrate=None, max_length=None):
    """launch(offset (f,) float32) -> (u on the host, partials, nparts).  case "asserted": the rows cycle `ratios`, 2e-5;
    "ratioN": every row at N, within 4 x the restatement, printed.  calibrate(want (f,) float64) -> (the per-row parameter of
    `launch` that brings row i to mean/std want[i], the ratios it can really reach) for a producer without an additive bias;
    max_length: the partial length up to which tests/test_bn_stats_reference.py validated `ratios`"""
    from sar_amd import ops
    want = torch.tensor([ratios[i % len(ratios)] if case == "asserted" else int(case[5:]) for i in range(f)], dtype=torch.float64)
    if calibrate is None:
        u0, _, _ = launch(torch.zeros(f))
        sigma = u0.double().std(dim=1, unbiased=False)
        param = (want * sigma - u0.double().mean(dim=1)).float()                   # the row's mean lands on ratio * sigma64(row)
    else:
        param, want = calibrate(want)
    u, part, nparts = launch(param)
    assert max_length is None or -(-n // nparts) <= max_length, "partials of %d columns: not validated on the CPU" % -(-n // nparts)
    g = torch.Generator().manual_seed(3)
    gamma, beta = (torch.rand(f, generator=g) + 0.5), torch.randn(f, generator=g)
    z = lambda: torch.zeros(f, device=dev)
    mean, rstd, scale, shift = z(), z(), z(), z()
    ops.bn_finalize(part, nparts, f, n, EPS, MOMENTUM, True, gamma.to(dev), beta.to(dev), None, None, mean, rstd, scale, shift)
    torch.cuda.synchronize()
    for t in (u, mean, rstd, scale, shift):
        assert torch.isfinite(t.cpu()).all()
    u64 = u.double().numpy()
    st = R.stats64(u64, EPS, gamma.double().numpy(), beta.double().numpy())
    y64 = R.normalised64(u64, st)
    reached = np.abs(st["mean"]) / np.sqrt(st["var"])
    err = R.channel_error(u64 * scale.cpu().double().numpy()[:, None] + shift.cpu().double().numpy()[:, None], y64)
    length = -(-n // nparts)
    rs = R.block_stats(u.numpy(), length, eps=EPS, gamma=gamma.double().numpy(), beta=beta.double().numpy())
    restated = R.channel_error(u64 * rs["scale"].astype(np.float64)[:, None] + rs["shift"].astype(np.float64)[:, None], y64)
    for ratio in sorted(set(want.round().tolist())):
        sel = want.round().numpy() == ratio
        print("%s mean/std %d (reached %.2f..%.2f), %d partials of %d columns: GPU %.3e, restatement %.3e" % (
            name, ratio, reached[sel].min(), reached[sel].max(), nparts, length, err[sel].max(), restated[sel].max()))
    assert np.abs(reached - want.numpy()).max() < 0.05, "the float64 ratio reached: %s" % reached
    bars = np.full(f, BAR) if case == "asserted" else np.full(f, 4.0 * restated.max())
    assert (err <= bars).all(), _worst(name, np.arange(f), err, bars)


@pytest.mark.parametrize("case", ["asserted", "ratio16", "ratio64"])
@pytest.mark.parametrize("arith", [None, "f16x3a", "bf16x6"], ids=["fp32", "f16x3a", "bf16x6"])
@pytest.mark.parametrize("kind", list(CONV_CASES))
def test_conv_epilogue_statistics_at_a_location(dev, kind, arith, case):
    launch, f, n = _conv_launcher(dev, kind, arith)
    assert n >= 2000
    _judge_producer(dev, "%s %s" % (kind, arith or "fp32"), launch, f, n, case, R.CONV_RATIOS, max_length=R.CONV_MAX_LENGTH)


# The dense-adjacency contractions leave one partial per row and tile (sar_graph_dense_nparts, sar_graph_dense_t_nparts): 187 and 94
# columns at 82 frames.  The offset comes in through `add`, constant along each row.  The chain restatement holds half the bar up to
# mean/std 4 (187 columns; 8 leaves 1.06e-5) and 8 (94 columns): R.DENSE_RATIOS, R.DENSE_T_RATIOS; 16 and 64 are recorded.
@pytest.mark.parametrize("case", ["asserted", "ratio16", "ratio64"])
@pytest.mark.parametrize("per_frame", [False, True], ids=["graph_dense_fwd", "graph_dense_t_fwd"])
def test_dense_adjacency_statistics_at_a_location(dev, per_frame, case):
    from sar_amd import ops
    from util import to_cn
    B, K, F, T, V = 2, 3, 64, 41, 25
    n = B * T * V
    g = torch.Generator().manual_seed(23 + per_frame)
    y = to_cn(torch.randn(B, K * F, T, V, generator=g)).to(dev)
    A = (torch.randn(*((K, T, V, V) if per_frame else (K, V, V)), generator=g) * 0.3).to(dev).contiguous()

    def launch(offset):
        out = torch.empty((F, n), device=dev)
        add = offset.view(-1, 1).expand(F, n).contiguous().to(dev)
        if per_frame:
            part, nparts = ops.graph_dense_t_fwd(y, A, out, K, F, V, B, T, stats=True, add=add)
        else:
            part, nparts = ops.graph_dense_fwd(y, A, out, K, F, V, B * T, stats=True, add=add)
        torch.cuda.synchronize()
        return out.cpu(), part, nparts
    _judge_producer(dev, "graph_dense_t_fwd" if per_frame else "graph_dense_fwd", launch, F, n, case,
                    R.DENSE_T_RATIOS if per_frame else R.DENSE_RATIOS)


@pytest.mark.parametrize("stream", ["joint", "bone"])
@pytest.mark.parametrize("shape", SHAPES, ids=["M1", "M2"])
def test_a_channel_near_zero_keeps_its_one_pass_statistics_bitwise(dev, shape, stream):
    """the pivot is the mean where the channel lies more than 2 standard deviations from 0 and 0 elsewhere; with pivot 0 the second
    pass leaves the first-pass sums alone, so such a channel's partials and statistics are those of sar_data_bn_stats_f32 +
    sar_bn_finalize_f32, bit for bit (centred training data computes what it computed with one pass)"""
    from sar_amd import ops
    x, gamma, beta, _ = _clip(shape)
    N, C, T, V, M = shape
    ref = _reference(shape, stream)
    parent = None if ref["parent"] is None else torch.from_numpy(ref["parent"]).to(dev)
    xg = x.to(dev)
    z = lambda: torch.zeros(V * C, device=dev)
    outs = []
    for pivot in (None, z()):
        part = torch.empty((V * C, N, 2), device=dev)
        mean, rstd, scale, shift = z(), z(), z(), z()
        ops.data_bn_stats(xg, parent, part, ref["motion"], pivot=pivot)
        ops.bn_finalize(part, N, V * C, N * M * T, EPS, MOMENTUM, False, gamma.to(dev), beta.to(dev), None, None, mean, rstd, scale,
                        shift, pivot=pivot)
        torch.cuda.synchronize()
        outs.append([t.cpu() for t in (part, mean, rstd, scale, shift)])
    p = pivot.cpu().numpy()
    live = ~ref["const"]
    assert (p[live & (ref["reached"] > 2.05)] != 0).all() and (p[live & (ref["reached"] < 1.95)] == 0).all()
    assert (p[ref["zero"]] == 0).all() and (p[ref["const"] & ~ref["zero"]] != 0).all()
    near = torch.from_numpy(p == 0)
    assert near.any() and not near.all()
    for name, a, b in zip(("partials", "mean", "rstd", "scale", "shift"), *outs):
        assert torch.equal(a[near].view(torch.int32), b[near].view(torch.int32)), "%s of a channel with pivot 0 differs" % name


# ------------------------------------------------------------------------------------------------ the CN8 (bf16) convolution epilogues
# sar_conv_gemm_cn8 reduces its statistics from the float32 ACCUMULATORS and stores the output rounded to bfloat16
# (csrc/conv_gemm_cn8.hip, csrc/conv_cn8_common.h), so the statistics are not those of the stored tensor: at mean/std r the rounding of
# 2 050 stored values moves their mean by about r * 2^-9 / sqrt(3 * 2050) std, 3e-4 std at 8.  They are therefore judged on the
# accumulators: the fp32 kernel's output for the SAME bf16-representable operands (no folded prologue, whose result the CN8 kernel
# rounds to bfloat16 once more; the graph operator, whose gathered operand it rounds too, by util.graph_ref in float64), which differs
# from the CN8 accumulators by the order of a float32 sum.  The stored output is held to
# util.assert_bf16_close of that tensor.  Same cases, ratios and bars as the fp32 epilogues.
def _conv_launcher_cn8(dev, kind):
    from oracle import stgcn as O
    from sar_amd import ops, ops8, _lib as L
    from test_gpu_cn8 import _pack
    from test_gpu_stgcn_kernels import _A, _tables
    from util import graph_ref, to_cn
    c = CONV_CASES[kind]
    B, cin, f, T, s = c["B"], c["cin"], c["f"], c["T"], c["s"]
    g = torch.Generator().manual_seed(len(kind) + 29)
    x4 = torch.randn(B, cin, T, 25, generator=g).bfloat16().float()
    xc = to_cn(x4).to(dev)
    x8 = ops8.from_cn(xc)
    bfw = lambda *shape, k: (torch.randn(*shape, generator=g) * k).bfloat16().float()
    if kind == "graph":
        W, tables = bfw(1, 1, cin, 3 * f, k=0.1), _tables(dev)
        To, geo, mode, strides = T, dict(B=B, V=25, T_src=T, T_out=T, Kc=cin, M=f, taps=3, tables=tables), L.SAR_CONV_GRAPH, (f, 3 * f)
    elif kind == "temporal9":
        W = bfw(9, 1, cin, f, k=0.05)
        To, pad, _ = O.same_pad(T, 9, s)
        geo, mode, strides = dict(B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=9, stride=s, pad=pad), L.SAR_CONV_TEMPORAL, (cin * f, f)
    else:
        W = bfw(1, 1, cin, f, k=0.1)
        To = -(-T // s)
        geo, mode, strides = dict(B=B, V=25, T_src=T, T_out=To, Kc=cin, M=f, taps=1, stride=s, pad=0), L.SAR_CONV_TEMPORAL, (0, f)
    packed = _pack(dev, W, strides[0], strides[1], 1, geo["taps"], cin, f)
    Wd, n = W.to(dev), B * To * 25

    def launch(bias):
        b3 = _conv_bias(kind, bias)
        out8 = ops8.empty(f, n, dev)
        r = ops8.conv_gemm(mode, x8, out8, packed, bias=b3.to(dev), epi=L.SAR_EPI_STATS, **geo)
        if kind == "graph":    # the CN8 graph kernel rounds the gathered operand to bfloat16: util.graph_ref is its exact definition
            acc = to_cn(graph_ref(x4, W, b3, _A(), tables)).float()
        else:
            out = torch.empty((f, n), device=dev)
            ops.conv_gemm(mode, xc, out, Wd, strides[0], strides[1], bias=b3.to(dev), split=None, **geo)
            acc = out
        torch.cuda.synchronize()
        assert_bf16_close(ops8.to_cn(out8, f).cpu(), acc.cpu(), "%s CN8 stored output" % kind)
        return acc.cpu(), r[0], r[1]
    return launch, f, n


@pytest.mark.parametrize("case", ["asserted", "ratio16", "ratio64"])
@pytest.mark.parametrize("kind", list(CONV_CASES))
def test_cn8_conv_epilogue_statistics_at_a_location(dev, kind, case):
    launch, f, n = _conv_launcher_cn8(dev, kind)
    assert n >= 2000
    _judge_producer(dev, "%s cn8" % kind, launch, f, n, case, R.CONV_RATIOS, max_length=R.CONV_MAX_LENGTH)


# ------------------------------------------------------------------------------------------------ conv2d_gemm with statistics
# sar_conv2d_gemm_f32 / _split have no bias.  The offset comes from an all-positive source (3x3: the folded prologue relu(0.05 x + 4);
# the 7x7 stem: a positive image 4 + 0.05 x) and a constant c[m] added to every weight of output row m: u[m] = a[m] + c[m] s, with
# a = W0 . h and s the window sum of h.  s drops at the zero-padded border, so mean/std cannot pass mean(s) / std(s) (about 7 for the
# 3x3 layer, 4 for the stem): a ratio beyond 0.9 of that is replaced by it, and the ratio reached is printed.  c solves
# (mean a + c mean s)^2 = r^2 var(a + c s) in float64.  Partials of 50 (3x3), 64 (stem) and 25 (split) columns.
CONV2D_CASES = {"3x3": dict(B=4, Kc=16, M=32, H_src=20, W_src=20, H_out=20, W_out=20, KH=3, KW=3, stride=1, pad=1),
                "stem7x7": dict(B=2, Kc=1, M=64, H_src=64, W_src=64, H_out=32, W_out=32, KH=7, KW=7, stride=2, pad=3)}


@pytest.mark.parametrize("case", ["asserted", "ratio16", "ratio64"])
@pytest.mark.parametrize("kind,arith", [("3x3", None), ("3x3", "f16x3a"), ("3x3", "bf16x6"), ("stem7x7", None)],
                         ids=["3x3-fp32", "3x3-f16x3a", "3x3-bf16x6", "stem7x7-fp32"])
def test_conv2d_statistics_at_a_location(dev, kind, arith, case):
    import torch.nn.functional as F
    from sar_amd import ops, _lib as L
    geo = CONV2D_CASES[kind]
    B, cin, cout, k, H, Ho = geo["B"], geo["Kc"], geo["M"], geo["KH"], geo["H_src"], geo["H_out"]
    taps, n = k * k, B * Ho * Ho
    assert arith is None or ops.conv2d_split_applicable(**geo)
    g = torch.Generator().manual_seed(k + 31)
    x = torch.randn(B, cin, H, H, generator=g)
    w0 = torch.randn(cout, cin, k, k, generator=g) / (cin * taps) ** 0.5
    cn = lambda t: t.permute(1, 0, 2, 3).reshape(t.shape[1], -1).contiguous()
    if cin > 1:
        src, pro = x, (torch.full((cin,), 0.05).to(dev), torch.full((cin,), 4.0).to(dev))
        h = torch.relu(x.double() * float(np.float32(0.05)) + 4.0)
    else:
        src, pro = (4.0 + 0.05 * x), None
        h = src.double()
    a = cn(F.conv2d(h, w0.double(), None, stride=geo["stride"], padding=geo["pad"])).numpy()
    s = cn(F.conv2d(h, torch.ones(1, cin, k, k, dtype=torch.float64), None, stride=geo["stride"], padding=geo["pad"])).numpy()[0]
    srcd = cn(src).to(dev)

    def calibrate(want):
        ma, va, ms, vs = a.mean(1), a.var(1), s.mean(), s.var()
        cov = ((a - ma[:, None]) * (s - ms)[None]).mean(1)
        r = np.minimum(want.numpy(), 0.9 * ms / np.sqrt(vs))
        qa, qb, qc = ms * ms - r * r * vs, 2 * (ma * ms - r * r * cov), ma * ma - r * r * va
        c = (-qb + np.sqrt(np.maximum(qb * qb - 4 * qa * qc, 0.0))) / (2 * qa)                     # the root with mean a + c mean s >= 0
        return torch.from_numpy(c).float(), torch.from_numpy(r)

    def launch(c):
        w = (w0 + c.view(-1, 1, 1, 1)).to(dev).contiguous()
        wf = torch.empty(taps * cin * cout, device=dev)
        ops.permute3(w, wf, taps, cin, cout, 1, taps, cin * taps)
        out = torch.empty((cout, n), device=dev)
        r = ops.conv2d_gemm(srcd, out, wf, cin * cout, cout, epi=L.SAR_EPI_STATS, pro=pro, pro_relu=pro is not None, split=arith, **geo)
        torch.cuda.synchronize()
        return out.cpu(), r[0], r[1]
    _judge_producer(dev, "conv2d %s %s" % (kind, arith or "fp32"), launch, cout, n, case, R.CONV_RATIOS, calibrate=calibrate,
                    max_length=R.CONV_MAX_LENGTH)


# ------------------------------------------------------------------------------------------------ gin_sum_fwd with partials
# s[c] = sum_k relu(a[k C + c] * scale + shift) has no bias and is not negative; the knob is one shift t[c] for the K branches of a
# row, found by bisection on the float64 mean/std of the row (monotone in t).  The smallest ratio a sum of three rectified normals
# reaches comfortably is 1, which stands in for 0.  n = 2 050 columns: 9 partials of 228 (n % 4 == 0 would leave 3 of 684).
@pytest.mark.parametrize("case", ["asserted", "ratio16", "ratio64"])
def test_gin_sum_statistics_at_a_location(dev, case):
    from sar_amd import ops
    K, C, n = 3, 16, R.CONV_COLUMNS
    g = torch.Generator().manual_seed(37)
    a = torch.randn(K * C, n, generator=g)
    sc = torch.rand(K * C, generator=g) + 0.5
    pre = (a.double() * sc.double()[:, None]).view(K, C, n).numpy()

    def ratio_at(t):
        s = np.maximum(pre + t[None, :, None], 0.0).sum(0)
        return s.mean(1) / np.maximum(s.std(1), 1e-300)

    def calibrate(want):
        lo, hi = np.full(C, -3.0), np.full(C, 400.0)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            below = ratio_at(mid) < want.numpy()
            lo, hi = np.where(below, mid, lo), np.where(below, hi, mid)
        return torch.from_numpy(hi).float(), want

    def launch(t):
        s_out = torch.empty((C, n), device=dev)
        part, nparts = ops.gin_sum_fwd(a.to(dev), sc.to(dev), t.repeat(K).to(dev), K, s_out, stats=True)
        torch.cuda.synchronize()
        return s_out.cpu(), part, nparts
    _judge_producer(dev, "gin_sum_fwd", launch, C, n, case, R.GIN_RATIOS, calibrate=calibrate, max_length=R.GIN_MAX_LENGTH)


# ------------------------------------------------------------------------------------------------ the CN8 backward apply passes
@pytest.mark.parametrize("ratio", [0, 16, 64])
def test_cn8_backward_apply_passes_at_uncentred_u(dev, ratio):
    """sar_affine2_cn8 and sar_bn_add_relu_bwd_apply_cn8 (both outputs): bf16 operands, float32 arithmetic, the result stored as
    bfloat16.  Per element: the one bfloat16 rounding util.assert_bf16_close allows (2^-8 of the value) plus the float32 bound of the
    fp32 passes, 4 * 2^-24 * (1 + ratio) of max |result|.  A result that lost the offset's cancellation would miss it by ratio * 2^-9."""
    from sar_amd import ops8
    C, n = 16, 2000
    g = torch.Generator().manual_seed(50 + ratio)
    bf = lambda t: t.bfloat16().float()
    u, r = bf(torch.randn(C, n, generator=g) + float(ratio)), bf(torch.randn(C, n, generator=g) - float(ratio))
    dy, y = bf(torch.randn(C, n, generator=g)), bf(torch.randn(C, n, generator=g))
    k1, k2 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5 for _ in range(2))
    k3 = -k2 * ratio + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    q1, q2 = (torch.rand(C, generator=g, dtype=torch.float64) + 0.5 for _ in range(2))
    q3 = q2 * ratio + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    col = lambda t: t.view(-1, 1)
    d8 = lambda t: ops8.from_cn(t.to(dev))
    k, q = tuple(t.float().to(dev) for t in (k1, k2, k3)), tuple(t.float().to(dev) for t in (q1, q2, q3))

    def judge(what, got8, want):
        got = ops8.to_cn(got8, C).cpu().double()
        excess = (got - want).abs() - 2.0 ** -8 * want.abs() - 4 * 2.0 ** -24 * (1 + ratio) * want.abs().amax(dim=1, keepdim=True)
        print("%s at mean/std %d: worst excess %.3e (worst error %.3e of max |result|)" % (
            what, ratio, excess.max().item(), ((got - want).abs().amax(dim=1) / want.abs().amax(dim=1)).max().item()))
        assert excess.max().item() <= 0, "%s at mean/std %d: worst excess %.3e" % (what, ratio, excess.max().item())

    out = ops8.empty(C, n, dev)
    ops8.affine2(d8(dy), d8(u), k, out, C)
    torch.cuda.synchronize()
    judge("affine2 cn8", out, col(k1) * dy.double() + col(k2) * u.double() + col(k3))
    du, dr, dz = ops8.empty(C, n, dev), ops8.empty(C, n, dev), ops8.empty(C, n, dev)
    ops8.bn_add_relu_bwd_apply(d8(dy), d8(y), d8(u), d8(r), k, q, du, dr, dz, C)
    torch.cuda.synchronize()
    dz64 = dy.double() * (y > 0)
    assert torch.equal(ops8.to_cn(dz, C).cpu().double(), dz64)
    judge("bn_add_relu_bwd_apply cn8 du", du, col(k1) * dz64 + col(k2) * u.double() + col(k3))
    judge("bn_add_relu_bwd_apply cn8 dr", dr, col(q1) * dz64 + col(q2) * r.double() + col(q3))
