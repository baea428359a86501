"""The edge shapes of the VirtualRadar kernels (csrc/radar.hip) and their inputs, shared by tests/test_radar_edge_reference.py (pins
the oracle at these shapes on the CPU) and tests/test_gpu_radar_edges.py (runs the HIP kernels at them).  Each shape names the path
it is there for; all are tiny."""
import numpy as np
import torch

from oracle import radar as R

# (T, n_fft, hop, out_cols, batch sizes, what it is for) -- sar_stft_logmag_f32 / sar_stft_logmag_bwd_f32
STFT_SHAPES = [
    (2, 2, 1, 0, (1, 3), "smallest accepted"),
    (10, 18, 4, 0, (1, 3), "T == half + 1, non-power-of-two, hop does not divide T"),
    (23, 30, 7, 9, (1, 3), "select, out_cols > F = 4"),
    (23, 30, 7, 3, (1, 3), "select, frames not consumed"),
    (23, 30, 7, 1, (1, 3), "select, one column"),
    (40, 16, 16, 0, (1, 3), "hop == n_fft"),
    (40, 16, 23, 0, (1, 3), "hop > n_fft: unread samples"),
    (300, 260, 16, 0, (1, 3), "second trip of the 256-strided loops"),
    (300, 260, 16, 7, (1, 3), "second trip of the 256-strided loops, with select"),
    (1025, 2048, 512, 0, (1,), "largest accepted n_fft"),
]

# sar_stft_kernels_fwd_f32 / sar_stft_kernels_bwd_f32
KERNEL_SHAPES = [
    (10, 18, 4, 0, (1, 3), "T == half + 1"),
    (23, 30, 7, 9, (1, 3), "select, out_cols > F"),
    (23, 30, 7, 3, (1, 3), "select, frames not consumed"),
    (40, 16, 23, 0, (1, 3), "hop > n_fft"),
    (300, 260, 16, 6, (1, 3), "partial last wave and partial KWB block in the wgrad, ncols % KF != 0"),
    (513, 1024, 256, 0, (1,), "largest accepted"),
]

# (T, V, M, E, what it is for) -- sar_vr_signal_f32 / sar_vr_signal_bwd_f32
SIGNAL_SHAPES = [
    (1, 2, 1, 1, "smallest"),
    (63, 7, 3, 5, "below the FRAMES boundary"),
    (65, 7, 3, 5, "above the FRAMES boundary"),
    (64, 6, 4, 5, "even V*M"),
    (70, 21, 4, 32, "exactly 64 KiB of LDS"),
]

# (B, T, V, M, P, sigma, what it is for) -- sar_upsample_prepare_f64 / sar_vr_signal_upsampled_f32 / ..._bwd_f32
UPSAMPLE_SHAPES = [
    (1, 5, 7, 3, 7, 3, "63 series, radius 12 > 2 T"),
    (3, 5, 7, 3, 1, 3, "P = 1"),
    (1, 9, 11, 2, 13, 0.1, "radius 0, 66 series"),
    (1, 304, 2, 1, 2, 3, "PREP_TMAX: the LDS solve"),
    (1, 305, 2, 1, 2, 3, "PREP_TMAX + 1: the global-scratch solve"),
]

LAM, LOC = 0.1, (0.4, -0.3, 1.0)          # the project's well-conditioned regime
MODULE_CLIP = (2, 3, 23, 7, 3)            # the module-level clip
LOG_EPS = float(np.float32(np.log(np.float32(1e-6))))


def edge_list(V, E, kind):
    """E edges on V joints.  "shared": joint 1 is used by several edges; "degenerate": one edge has src == dst.  E = 1 is the single
    bone (0, 1); the long lists (E > 5) hold both features."""
    if E == 1:
        return [(0, 1)]
    if E == 5:
        assert V >= 6
        return [(0, 1), (1, 2), (1, 3), (3, 4), (4, 5)] if kind == "shared" else [(0, 1), (1, 2), (2, 3), (4, 4), (3, 5)]
    chain = [(i, i + 1) for i in range(V - 1)]
    star = [(1, j) for j in range(3, V)]
    edges = (chain + [(7 % V, 7 % V)] + star)[:E]
    assert len(edges) == E, "V = %d has no %d edges" % (V, E)
    return edges


def signal_edge_kinds(E):
    return ("shared", "degenerate") if E == 5 else ("both",)


def clip(shape, seed):
    """clamp(0.12 * randn, -1.1, 0.75) like tests/test_gpu_radar.py, float32 numpy"""
    g = torch.Generator().manual_seed(seed)
    return (0.12 * torch.randn(shape, generator=g)).clamp_(-1.1, 0.75).numpy()


def normal(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).numpy()


def fourier_kernels(n_fft, variant):
    """(wcos, wsin) [k][n] float32: the analytic kernels of oracle.radar.stft_kernels, or those perturbed by 0.05 N(0, 1)"""
    wcos, wsin = R.stft_kernels(n_fft)
    if variant == "perturbed":
        rng = np.random.default_rng(100 + n_fft)
        wsin = wsin + (0.05 * rng.standard_normal((n_fft, n_fft))).astype(np.float32)
        wcos = wcos + (0.05 * rng.standard_normal((n_fft, n_fft))).astype(np.float32)
    return np.ascontiguousarray(wcos), np.ascontiguousarray(wsin)


def explicit_log_spectrogram(zr, zi, n_fft, hop):
    """The stage written out with numpy's own reflect padding and FFT in float64: (log(|Z| + 1e-6) rolled by n_fft/2, |Z|),
    each (B, n_fft, F)."""
    u = np.asarray(zr, dtype=np.float64) + 1j * np.asarray(zi, dtype=np.float64)
    half = n_fft // 2
    up = np.pad(u, ((0, 0), (half, half)), mode="reflect")
    F_ = u.shape[1] // hop + 1
    w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(n_fft) / n_fft)                      # periodic Hann
    Z = np.stack([np.fft.fft(up[:, f * hop:f * hop + n_fft] * w, axis=1) for f in range(F_)], axis=2)   # (B, k, F)
    mag = np.abs(Z)
    return np.roll(np.log(mag + 1e-6), half, axis=1), mag


def eval_pieces(coef, B, T, P, V, M):
    """the cubic pieces [B][T-1][3][V*M][4] of sar_upsample_prepare_f64 evaluated at np.linspace(0, 1, P*T) the way the signal
    kernels do (interval floor(x (T-1)), local dx in units of x) -> (B, 3, P*T, V, M) float64"""
    Tup = P * T
    xn = np.arange(Tup, dtype=np.float64) / float(Tup - 1)
    i = np.minimum(np.floor(xn * (T - 1)).astype(np.int64), T - 2)
    dx = (xn - i / float(T - 1))[None, :, None, None]
    c = np.asarray(coef, dtype=np.float64).reshape(B, T - 1, 3, V * M, 4)[:, i]         # (B, Tup, 3, VM, 4)
    val = c[..., 0] + dx * (c[..., 1] + dx * (c[..., 2] + dx * c[..., 3]))
    return np.ascontiguousarray(val.transpose(0, 2, 1, 3)).reshape(B, 3, Tup, V, M)
