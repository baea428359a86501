"""The radar oracle (oracle/radar.py) at the edge shapes of tests/test_gpu_radar_edges.py, on the CPU: a GPU failure at one of these
shapes then means the kernel is wrong, not the yardstick.  Every statement is checked against something that is NOT the oracle's own
code: numpy's reflect padding and FFT, torch's nearest interpolation, central differences, scipy called directly."""
import numpy as np
import pytest
import torch

from oracle import radar as R
from radar_edges import (KERNEL_SHAPES, LAM, LOC, MODULE_CLIP, SIGNAL_SHAPES, STFT_SHAPES, clip, edge_list, explicit_log_spectrogram,
                         normal, signal_edge_kinds)

ALL_STFT = sorted({s[:4] for s in STFT_SHAPES + KERNEL_SHAPES})
IDS = ["T%d-n%d-h%d-c%d" % s for s in ALL_STFT]


@pytest.mark.parametrize("T,n_fft,hop,out_cols", ALL_STFT, ids=IDS)
def test_stft_oracles_equal_an_explicit_float64_dft(T, n_fft, hop, out_cols):
    """stft_torch in float64 (the truth of the GPU tests) to 1e-12 of the peak, its column select included; the float32 numpy
    stft_complex / log_spectrogram to 1e-5 of the peak (their float32 einsum over n_fft terms)."""
    zr, zi = normal((2, T), 11).astype(np.float32), normal((2, T), 12).astype(np.float32)
    logm, mag = explicit_log_spectrogram(zr, zi, n_fft, hop)
    F_ = T // hop + 1
    assert mag.shape == (2, n_fft, F_)
    t = R.stft_torch(torch.from_numpy(zr), torch.from_numpy(zi), n_fft, hop, out_cols).numpy()
    want = logm if out_cols == 0 else logm[:, :, R.nearest_columns(F_, out_cols)]
    assert t.shape == want.shape and t.dtype == np.float64
    assert np.abs((np.exp(t) - 1e-6) - (np.exp(want) - 1e-6)).max() <= 1e-12 * mag.max()
    # the complex transform of one real signal: (real, -imag) = (Re, Im) of the FFT
    re, im = R.stft_complex(zr, n_fft, hop)
    half = n_fft // 2
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)
    up = np.pad(zr.astype(np.float64), ((0, 0), (half, half)), mode="reflect")
    Z = np.stack([np.fft.fft(up[:, f * hop:f * hop + n_fft] * w, axis=1) for f in range(F_)], axis=2)
    scale = np.abs(Z).max()
    assert re.shape == (2, n_fft, F_) and np.abs(re - Z.real).max() <= 1e-5 * scale and np.abs(im - Z.imag).max() <= 1e-5 * scale
    l32, m32 = R.log_spectrogram(zr, zi, n_fft, hop)
    assert np.abs(m32 - mag).max() <= 1e-5 * mag.max()
    assert np.abs((np.exp(l32.astype(np.float64)) - 1e-6) - (np.exp(logm) - 1e-6)).max() <= 1e-5 * mag.max()


@pytest.mark.parametrize("T,n_fft,hop,out_cols", [s for s in ALL_STFT if s[3] > 0], ids=[i for i, s in zip(IDS, ALL_STFT) if s[3] > 0])
def test_nearest_columns_are_torchs_nearest_interpolation(T, n_fft, hop, out_cols):
    F_ = T // hop + 1
    src = torch.arange(F_, dtype=torch.float32).view(1, 1, F_)
    want = torch.nn.functional.interpolate(src, out_cols, mode="nearest")[0, 0].long().numpy()
    got = R.nearest_columns(F_, out_cols)
    assert np.array_equal(got, want)
    assert got.min() >= 0 and got.max() <= F_ - 1
    if out_cols < F_:
        assert len(set(range(F_)) - set(got.tolist())) > 0        # the case is there for frames nobody reads
    if out_cols > F_:
        assert len(set(got.tolist())) < out_cols                  # ... and for frames read more than once


def _edge_clips():
    yield MODULE_CLIP, edge_list(7, 5, "shared"), 30, 7, 0
    yield MODULE_CLIP, edge_list(7, 5, "degenerate"), 30, 7, 9
    yield (2, 3, 23, 7, 3), edge_list(7, 5, "shared"), 18, 5, 0
    yield (2, 3, 40, 6, 4), edge_list(6, 5, "degenerate"), 16, 23, 0
    yield (1, 3, 70, 21, 4), edge_list(21, 32, "both"), 44, 3, 0


@pytest.mark.parametrize("shape,edges,n_fft,hop,out_cols", list(_edge_clips()), ids=["shared", "degenerate-select", "n18", "hop23", "E32"])
def test_spectrogram_torch_is_signal_then_log_spectrogram(shape, edges, n_fft, hop, out_cols):
    """the float64 torch restatement against the float32 numpy stages (written independently of it): signal within 2e-5 of its scale,
    magnitude within 1e-4 of the peak -- the floors of tests/test_gpu_radar.py; and it is exactly its two stages in sequence"""
    x = clip(shape, 21)
    loc, lam = torch.tensor(LOC, dtype=torch.float64), torch.tensor(LAM, dtype=torch.float64)
    out = R.spectrogram_torch(x, loc, lam, edges=edges, n_fft=n_fft, hop=hop, out_cols=out_cols)
    zr64, zi64 = R.signal_torch(x, loc, lam, edges)
    assert torch.equal(out, R.stft_torch(zr64, zi64, n_fft, hop, out_cols))
    zr, zi = R.radar_signal(x, edges, LAM, LOC)
    scale = max(zr64.abs().max().item(), zi64.abs().max().item())
    assert np.isfinite(zr).all() and np.isfinite(zi).all() and scale > 0
    assert np.abs(zr - zr64.numpy()).max() <= 2e-5 * scale and np.abs(zi - zi64.numpy()).max() <= 2e-5 * scale
    l32 = R.log_spectrogram(zr, zi, n_fft, hop)[0].astype(np.float64)
    if out_cols:
        l32 = l32[:, :, R.nearest_columns(l32.shape[2], out_cols)]
    m64 = np.exp(out.numpy()) - 1e-6
    assert l32.shape == tuple(out.shape)
    assert np.abs((np.exp(l32) - 1e-6) - m64).max() <= 1e-4 * m64.max()


@pytest.mark.parametrize("T,V,M,E,why", SIGNAL_SHAPES, ids=["T%d-V%d-M%d-E%d" % s[:4] for s in SIGNAL_SHAPES])
def test_signal_oracles_agree_at_the_signal_shapes(T, V, M, E, why):
    for kind in signal_edge_kinds(E):
        edges = edge_list(V, E, kind)
        assert len(edges) == E and max(max(e) for e in edges) < V
        x = clip((2, 3, T, V, M), 31)
        z64 = R.signal_torch(x, torch.tensor(LOC, dtype=torch.float64), torch.tensor(LAM, dtype=torch.float64), edges)
        zr, zi = R.radar_signal(x, edges, LAM, LOC)
        scale = max(z64[0].abs().max().item(), z64[1].abs().max().item())
        assert np.abs(zr - z64[0].numpy()).max() <= 2e-5 * scale and np.abs(zi - z64[1].numpy()).max() <= 2e-5 * scale
        # an all-zero clip is exact silence
        z0 = R.radar_signal(np.zeros((1, 3, T, V, M), np.float32), edges, LAM, LOC)
        assert not z0[0].any() and not z0[1].any()


def test_parameter_gradients_agree_with_central_differences():
    """radar_param_grads (autograd, float64) against central differences of the same float64 function, degenerate edge included"""
    x = clip((1, 3, 12, 6, 2), 41)
    edges = edge_list(6, 5, "degenerate")
    kw = dict(edges=edges, n_fft=8, hop=3, out_cols=7)
    w = normal((1, 8, 7), 42).astype(np.float64)
    dloc, dlam = R.radar_param_grads(x, w, LOC, LAM, **kw)

    def f(loc, lam):
        out = R.spectrogram_torch(x, torch.tensor(loc, dtype=torch.float64), torch.tensor(lam, dtype=torch.float64), **kw)
        return float((out * torch.from_numpy(w)).sum())
    eps = 1e-6
    for p in range(3):
        lp, lm = list(LOC), list(LOC)
        lp[p] += eps
        lm[p] -= eps
        fd = (f(lp, LAM) - f(lm, LAM)) / (2 * eps)
        assert abs(fd - dloc[p]) <= 1e-5 * np.abs(dloc).max(), (p, fd, dloc)
    eps = 1e-8
    fd = (f(list(LOC), LAM + eps) - f(list(LOC), LAM - eps)) / (2 * eps)
    assert abs(fd - dlam) <= 1e-5 * abs(dlam), (fd, dlam)


@pytest.mark.parametrize("sigma", [3, 0.1])
@pytest.mark.parametrize("T", [5, 6, 9])
def test_pad_frames_at_short_clips(T, sigma):
    from scipy.interpolate import interp1d
    from scipy.ndimage import gaussian_filter1d
    x = clip((3, T, 7, 3), 50 + T)
    sm = gaussian_filter1d(x, sigma, axis=-3)
    assert sm.dtype == np.float32
    knots = np.linspace(0, 1, T)
    direct = interp1d(knots, sm, kind="cubic", axis=-3)
    # scipy's own spline, finely sampled: its overshoot beyond the knots' range.  Between two samples (spacing h = 1 / (400 T)) the
    # spline rises above them by at most h^2 / 8 max |f''|, and |f''| <= 6 (T-1)^2 x 4 max |y| for a cubic through these knots'
    # second differences: under 2e-5 of the clip's scale.
    dense = direct(np.linspace(0, 1, 400 * T + 1))
    slack = 2e-5 * np.abs(sm).max()
    for P in (1, 7, 13):
        up = R.pad_frames(x, P, sigma)
        assert up.shape == (3, P * T, 7, 3) and up.dtype == np.float32
        assert np.array_equal(up, direct(np.linspace(0, 1, P * T)).astype(np.float32))
        sm2, up64 = R.pad_frames_parts(x, P, sigma)
        assert np.array_equal(sm2, sm) and up64.dtype == np.float64 and np.array_equal(up64.astype(np.float32), up)
        # the end points are knots; every coordinate stays inside the range of scipy's spline through the smoothed clip
        tiny = 1e-6 * np.abs(sm).max()
        assert np.abs(up[:, 0] - sm[:, 0]).max() <= tiny and np.abs(up[:, -1] - sm[:, -1]).max() <= tiny
        assert (up <= dense.max(axis=-3, keepdims=True) + slack).all() and (up >= dense.min(axis=-3, keepdims=True) - slack).all()
        if P == 1:
            assert np.abs(up - sm).max() <= tiny                     # the smoothed clip itself
    if sigma == 0.1:
        assert np.array_equal(sm, x)                                 # radius 0: the filter is the identity
    # float64 end to end (the truth of the up-sampled GPU cases) stays close to the float32-smoothed pipeline
    sm64, up64 = R.pad_frames_parts(x.astype(np.float64), 7, sigma)
    assert sm64.dtype == np.float64 and np.abs(up64 - R.pad_frames(x, 7, sigma)).max() <= 1e-5 * np.abs(sm64).max() + 1e-7
