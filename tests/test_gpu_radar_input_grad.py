"""GPU: the gradient of VirtualRadar with respect to the skeleton input -- sar_vr_signal_bwd_x_f32 (csrc/radar.hip) through
layers.virtual_radar.VirtualRadar.signal_backward_x, the layer under autograd, and x.grad through models.resnet.Model.

Truth is torch autograd of the float64 oracle (oracle.radar.signal_torch / spectrogram_torch) at the parameter values the module
holds (its float32 wavelength and radar_location, as tests/test_gpu_radar.py::test_parameter_gradients_against_reference_autograd
takes them).  Errors are norm-wise relative.  A case passes below 2e-5 (the project's per-kernel fp32 tolerance) or within
3 x the band, the band being the distance of the SAME oracle run in float32 on the CPU from its float64 run: at lambda = 5e-4 the
phase is ~1e5 rad and float32 itself is 1e-4 away.  Every case first asserts that the float64 gradient is finite: the synthetic
clips put every body everywhere (tests/golden/make_golden_radar_grad.py's recipe); on real NTU clips the reference is NaN.
Degenerate inputs are checked against the hand-written adjoint tests/radar_dx_reference.py (zero subgradient)."""
import functools

import numpy as np
import pytest
import torch

import radar_dx_reference as X
from oracle import radar as R

pytestmark = pytest.mark.gpu

CASES = [(10.0, (0.5, -1.0, 2.0)), (0.1, (0.5, -1.0, 2.0)), (1e-2, (0.3, 0.2, -1.5)), (5e-4, (0.0, 0.0, 0.0))]
SHAPES = [(1, 5, 1), (2, 64, 2), (3, 65, 2), (2, 130, 3)]      # (B, T, M): a tail wave, an exact wave, one frame over, three bodies
HUB_EDGES = [(0, 1), (1, 2), (1, 3), (1, 4), (4, 5)]           # joint 1 collects four edges, joint 6 is in none
NAN_BITS = 0x7FC00ABC                                           # a quiet NaN with a payload: the guard-band fill


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _f32(v):
    """the value a float32 Parameter holds, as float64"""
    return np.asarray(v, dtype=np.float32).astype(np.float64)


def _radar(dev, lam, loc, edges=R.EDGES, **kw):
    from layers.virtual_radar import VirtualRadar
    return VirtualRadar(edges=edges, wavelength=lam, radar_location=list(loc), device=dev, **kw)


@functools.lru_cache(maxsize=None)
def _signal_truth(lam, loc, B, T, V, M, edges):
    """(x, dz_re, dz_im, float64 autograd, band) of the signal stage; computed once per case"""
    x = X.synthetic_clip(B, T, V, M)
    ur, ui = X.cotangent(B, T)
    t64 = X.autograd_dx(x, _f32(loc), _f32(lam), ur, ui, list(edges))
    t32 = X.autograd_dx(x, _f32(loc), _f32(lam), ur, ui, list(edges), dtype=torch.float32)
    return x, ur, ui, t64, X.rel_err(t32, t64)


def _run(vr, dev, x, ur, ui):
    dx = vr.signal_backward_x(torch.from_numpy(x).to(dev), torch.from_numpy(ur).to(dev), torch.from_numpy(ui).to(dev))
    torch.cuda.synchronize()
    return dx


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "B%dT%dM%d" % s)
@pytest.mark.parametrize("lam,loc", CASES, ids=lambda v: ("lam%g" % v) if isinstance(v, float) else "")
def test_signal_stage_against_float64(dev, lam, loc, shape):
    """All terms: at lambda = 10 dropping the coupling through c moves dx by 0.1 and dropping the amplitude path by 1.0 (relative),
    at 5e-4 the phase term dominates and they move it by 3e-5 / 1e-3."""
    B, T, M = shape
    x, ur, ui, truth, band = _signal_truth(lam, loc, B, T, 25, M, tuple(R.EDGES))
    assert np.isfinite(truth).all()
    dx = _run(_radar(dev, lam, loc), dev, x, ur, ui)
    assert dx.shape == x.shape and dx.dtype == torch.float32 and dx.is_contiguous()
    err = X.rel_err(dx.cpu().numpy(), truth)
    print("signal dx lambda %g B %d T %d M %d: err %.2e  band %.2e" % (lam, B, T, M, err, band))
    assert X.within_band(err, band), (err, band)


def test_custom_graph_with_a_hub_and_an_unused_joint(dev):
    lam, loc = 0.1, (0.5, -1.0, 2.0)
    x, ur, ui, truth, band = _signal_truth(lam, loc, 2, 9, 7, 4, tuple(HUB_EDGES))
    assert np.isfinite(truth).all()
    dx = _run(_radar(dev, lam, loc, edges=HUB_EDGES), dev, x, ur, ui).cpu().numpy()
    assert (dx[:, :, :, 6] == 0).all() and not np.signbit(dx[:, :, :, 6]).any()
    err = X.rel_err(dx, truth)
    hub = X.rel_err(dx[:, :, :, 1], truth[:, :, :, 1])
    print("custom graph: err %.2e (hub joint %.2e)  band %.2e" % (err, hub, band))
    assert X.within_band(err, band) and X.within_band(hub, band), (err, hub, band)


def test_an_absent_body_gets_exactly_zero(dev):
    lam, loc = 0.1, (0.5, -1.0, 2.0)
    x = X.synthetic_clip(2, 9).copy()
    x[:, :, :, :, 1] = 0
    ur, ui = X.cotangent(2, 9)
    want = X.signal_dx(x, _f32(loc), _f32(lam), ur, ui, R.EDGES)
    one = np.ascontiguousarray(x[..., :1])
    band = X.rel_err(X.autograd_dx(one, _f32(loc), _f32(lam), ur, ui, R.EDGES, dtype=torch.float32),
                     X.autograd_dx(one, _f32(loc), _f32(lam), ur, ui, R.EDGES))
    assert np.isfinite(want).all() and (want[..., 1] == 0).all()
    dx = _run(_radar(dev, lam, loc), dev, x, ur, ui).cpu().numpy()
    assert np.isfinite(dx).all()
    assert (dx[..., 1] == 0).all()
    err = X.rel_err(dx[..., 0], want[..., 0])
    print("absent body: body 0 err %.2e  band %.2e" % (err, band))
    assert X.within_band(err, band), (err, band)


def test_a_joint_at_the_radar_and_a_zero_length_edge_stay_finite(dev):
    lam, loc = 0.1, (0.5, -1.0, 2.0)
    x = X.synthetic_clip(2, 9).copy()
    x[0, :, 2, 20, 0] = np.asarray(loc, dtype=np.float32)
    x[1, :, 4, 5, 1] = x[1, :, 4, 4, 1]
    ur, ui = X.cotangent(2, 9)
    want = X.signal_dx(x, _f32(loc), _f32(lam), ur, ui, R.EDGES)
    dx = _run(_radar(dev, lam, loc), dev, x, ur, ui).cpu().numpy()
    assert np.isfinite(want).all() and np.isfinite(dx).all()
    # the frames without a degenerate point agree with the reference (the float32 value of u next to |u| = 1 differs at the others)
    keep = np.ones(9, dtype=bool)
    keep[[2, 4]] = False
    assert X.rel_err(dx[:, :, keep], want[:, :, keep]) < 1e-4


@pytest.mark.parametrize("shape", [(1, 5, 1), (3, 65, 2)], ids=lambda s: "B%dT%dM%d" % s)
def test_nothing_outside_dx_is_written_and_all_of_dx_is(dev, shape):
    from sar_amd._lib import check, load, ptr, stream_ptr
    B, T, M = shape
    V, margin = 25, 4096
    vr = _radar(dev, 0.1, (0.5, -1.0, 2.0))
    x = torch.from_numpy(X.synthetic_clip(B, T, V, M)).to(dev)
    ur, ui = (torch.from_numpy(a).to(dev) for a in X.cotangent(B, T))
    n = x.numel()
    buf = torch.full((n + 2 * margin,), NAN_BITS, dtype=torch.int32, device=dev)
    inner = buf[margin:margin + n].view(torch.float32)
    assert torch.isnan(inner).all()
    check(load().sar_vr_signal_bwd_x_f32(ptr(x), B, T, V, M, ptr(vr._src), ptr(vr._dst), len(vr.src), ptr(vr.radar_location.data),
                                         ptr(vr.wavelength.data.reshape(1)), ptr(ur), ptr(ui), ptr(inner), stream_ptr()))
    torch.cuda.synchronize()
    assert (buf[:margin] == NAN_BITS).all() and (buf[margin + n:] == NAN_BITS).all()
    assert not torch.isnan(inner).any()
    assert torch.equal(inner.view(x.shape), vr.signal_backward_x(x, ur, ui))


def test_bitwise_reproducible_and_independent_of_the_batch(dev):
    vr = _radar(dev, 5e-4, (0.0, 0.0, 0.0))
    x = torch.from_numpy(X.synthetic_clip(3, 65, 25, 2)).to(dev)
    ur, ui = (torch.from_numpy(a).to(dev) for a in X.cotangent(3, 65))
    a, b = vr.signal_backward_x(x, ur, ui), vr.signal_backward_x(x, ur, ui)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    for i in range(3):
        one = vr.signal_backward_x(x[i:i + 1].contiguous(), ur[i:i + 1].contiguous(), ui[i:i + 1].contiguous())
        assert torch.equal(one.view(torch.int32), a[i:i + 1].view(torch.int32)), i


# ---- the layer under autograd, end to end against oracle.radar.spectrogram_torch at n_fft = 32, hop = 4, T = 70
N_FFT, HOP, T_E2E = 32, 4, 70


@functools.lru_cache(maxsize=None)
def _e2e_truth(lam, out_cols):
    loc = (0.5, -1.0, 2.0)
    x = X.synthetic_clip(2, T_E2E)
    F_ = T_E2E // HOP + 1
    w = np.random.default_rng(7).standard_normal((2, N_FFT, out_cols or F_)).astype(np.float32)
    grads = []
    for dt in (torch.float64, torch.float32):
        xt = torch.from_numpy(x).to(dt).requires_grad_(True)
        out = R.spectrogram_torch(xt, torch.from_numpy(_f32(loc)).to(dt), torch.tensor(float(_f32(lam)), dtype=dt),
                                  n_fft=N_FFT, hop=HOP, out_cols=out_cols, dtype=dt)
        (out * torch.from_numpy(w).to(dt)).sum().backward()
        grads.append(xt.grad.double().numpy())
    return loc, x, w, grads[0], X.rel_err(grads[1], grads[0])


@pytest.mark.parametrize("out_cols", [0, 32])
@pytest.mark.parametrize("lam", [0.1, 5e-4])
def test_module_gives_x_a_gradient(dev, lam, out_cols):
    """(a) only x requires a gradient"""
    loc, x, w, truth, band = _e2e_truth(lam, out_cols)
    assert np.isfinite(truth).all()
    vr = _radar(dev, lam, loc, n_fft=N_FFT, hop_length=HOP)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    out = vr(xg, out_cols=out_cols)
    assert out.requires_grad
    (out * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    assert vr.radar_location.grad is None and vr.wavelength.grad is None
    with torch.no_grad():
        assert torch.equal(out.detach(), vr(xg, out_cols=out_cols))      # the forward through the node is the plain forward
    err = X.rel_err(xg.grad.cpu().numpy(), truth)
    print("module dx lambda %g out_cols %d: err %.2e  band %.2e" % (lam, out_cols, err, band))
    assert X.within_band(err, band), (err, band)


def test_parameter_gradients_do_not_change_when_x_wants_one_too(dev):
    """(b) train_radar_location / train_wavelength with and without x.requires_grad: dloc / dlam bitwise equal, x.grad as in (a)"""
    lam, out_cols = 0.1, 0
    loc, x, w, truth, band = _e2e_truth(lam, out_cols)
    res = []
    for want_x in (False, True):
        vr = _radar(dev, lam, loc, n_fft=N_FFT, hop_length=HOP, train_radar_location=True, train_wavelength=True)
        xg = torch.from_numpy(x).to(dev).requires_grad_(want_x)
        (vr(xg, out_cols=out_cols) * torch.from_numpy(w).to(dev)).sum().backward()
        torch.cuda.synchronize()
        res.append((vr.radar_location.grad.clone(), vr.wavelength.grad.clone(), xg.grad))
    assert res[0][2] is None
    assert torch.equal(res[0][0].view(torch.int32), res[1][0].view(torch.int32))
    assert torch.equal(res[0][1].view(torch.int32), res[1][1].view(torch.int32))
    assert X.within_band(X.rel_err(res[1][2].cpu().numpy(), truth), band)
    # ... and x.grad does not depend on what else trains
    vr = _radar(dev, lam, loc, n_fft=N_FFT, hop_length=HOP)
    xg = torch.from_numpy(x).to(dev).requires_grad_(True)
    (vr(xg, out_cols=out_cols) * torch.from_numpy(w).to(dev)).sum().backward()
    assert torch.equal(xg.grad.view(torch.int32), res[1][2].view(torch.int32))


@pytest.mark.parametrize("train_kernels", [True, False], ids=["kernels_train", "kernels_frozen"])
def test_trainable_fourier_kernels_pass_the_gradient_on(dev, train_kernels):
    """(c) train_stft_kernel=True: the signal cotangent is produced for x alone; the kernel gradients are bitwise those of a run
    whose x does not require a gradient"""
    lam, out_cols = 0.1, 32
    loc, x, w, truth, band = _e2e_truth(lam, out_cols)
    res = []
    for want_x in (False, True):
        vr = _radar(dev, lam, loc, n_fft=N_FFT, hop_length=HOP, train_stft_kernel=True)
        vr.stft.wcos.requires_grad_(train_kernels)
        vr.stft.wsin.requires_grad_(train_kernels)
        if not (want_x or train_kernels):
            res.append((None, None, None))
            continue
        xg = torch.from_numpy(x).to(dev).requires_grad_(want_x)
        (vr(xg, out_cols=out_cols) * torch.from_numpy(w).to(dev)).sum().backward()
        torch.cuda.synchronize()
        res.append((vr.stft.wcos.grad, vr.stft.wsin.grad, xg.grad))
    if train_kernels:
        assert res[0][2] is None
        for a, b in zip(res[0][:2], res[1][:2]):
            assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    else:
        assert res[1][0] is None and res[1][1] is None
    err = X.rel_err(res[1][2].cpu().numpy(), truth)      # the kernels hold float32 of the analytic ones
    print("trainable kernels (%s): dx err %.2e  band %.2e" % (train_kernels, err, band))
    assert X.within_band(err, band), (err, band)


def test_nothing_changes_when_x_does_not_require_a_gradient(dev):
    lam, loc = 5e-4, (0.0, 0.0, 0.0)
    vr = _radar(dev, lam, loc, n_fft=N_FFT, hop_length=HOP)
    x = torch.from_numpy(X.synthetic_clip(2, T_E2E)).to(dev)
    out = vr(x)
    assert not out.requires_grad and out.grad_fn is None and x.grad is None
    assert torch.equal(out, vr._stft(*vr.signal(x)))
    xg = x.clone().requires_grad_(True)
    assert torch.equal(vr(xg).detach(), out)
    with torch.no_grad():
        assert vr(xg).grad_fn is None


def test_the_upsampling_path_refuses_a_gradient_for_x(dev):
    vr = _radar(dev, 5e-4, (0.0, 0.0, 0.0), n_fft=N_FFT, hop_length=HOP)
    x = torch.from_numpy(X.synthetic_clip(1, 12)).to(dev)
    with pytest.raises(ValueError, match="num_pad_frames"):
        vr(x.clone().requires_grad_(True), num_pad_frames=4)
    out = vr(x, num_pad_frames=4)                                  # data: as before
    assert out.shape == (1, N_FFT, 48 // HOP + 1)
    with torch.no_grad():
        assert torch.equal(vr(x.clone().requires_grad_(True), num_pad_frames=4), out)


def test_model_fills_x_grad(dev):
    """models.resnet.Model at the smallest configuration of tests/test_gpu_resnet.py: x.grad is the signal adjoint of the STFT adjoint
    of the engine's own d loss / d image, bit for bit"""
    from models.resnet import Model
    from sar_amd._lib import check, load, ptr, stream_ptr
    model = Model(num_classes=10, num_filters=8, device=dev)
    model.train()
    vr = model.virtual_radar
    x = torch.from_numpy(X.synthetic_clip(2, 300, seed=1)).to(dev)
    y = torch.tensor([3, 7], device=dev)
    xg = x.clone().requires_grad_(True)
    torch.nn.functional.cross_entropy(model(xg), y).backward()
    torch.cuda.synchronize()
    assert xg.grad.shape == x.shape and torch.isfinite(xg.grad).all() and xg.grad.abs().max() > 0
    # the same step with the image as the leaf: the engine's d loss / d image
    img = model.spectrogram(x).detach().requires_grad_(True)
    torch.nn.functional.cross_entropy(model.base_model(img), y).backward()
    dimg = img.grad[:, 0].contiguous()
    zr, zi = vr.signal(x)
    lib = load()
    ws = torch.empty(lib.sar_stft_logmag_bwd_workspace_floats(2, 300, vr.n_fft, vr.hop_length), dtype=torch.float32, device=dev)
    dzr, dzi = torch.empty_like(zr), torch.empty_like(zi)
    check(lib.sar_stft_logmag_bwd_f32(ptr(zr), ptr(zi), 2, 300, vr.n_fft, vr.hop_length, ptr(vr.window), model.image_size, ptr(dimg),
                                      ptr(ws), ptr(dzr), ptr(dzi), stream_ptr()))
    want = vr.signal_backward_x(x, dzr, dzi)
    torch.cuda.synchronize()
    assert torch.equal(want.view(torch.int32), xg.grad.view(torch.int32))
