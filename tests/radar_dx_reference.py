"""CPU float64 reference for the gradient of the VirtualRadar signal stage with respect to the skeleton
(sar_vr_signal_bwd_x_f32, layers.virtual_radar.VirtualRadar.signal_backward_x):

    dx = d/dx sum_{b,t} (dz_re * z_re + dz_im * z_im),      (z_re, z_im) = oracle.radar.signal_torch(x, loc, lam)

`signal_dx` is a HAND-WRITTEN reverse mode in numpy, not autograd: it is defined at the degenerate points where autograd is NaN
(conventions below) and shares no code with the kernel.  `autograd_dx` is torch autograd through the oracle (the truth at generic
points, and the float32 run that gives the tolerance band); `synthetic_clip` / `cotangent` are the seeded inputs of the tests.

Per (frame, body), edge (s, d), e = s - loc, A = loc - (s + d)/2, B = d - s, u = <A,B> / (|A||B| + 1e-6) = cos(theta),
c = (mean_e |B_e|)^2:
    den = sin^2(theta) (cos^2(phi) + sin^2(phi)) + c cos^2(theta) = (1 - u)(1 + u) + c u^2       (phi cancels: d den / d phi = 0)
    amp = sqrt(pi c) / |den|,   psi = 4 pi |e| / lam
    P = dz_re cos(psi) + dz_im sin(psi) = dL/d amp,     amp Q = amp (dz_im cos(psi) - dz_re sin(psi)) = dL/d psi
    phase:      ds += amp Q (4 pi / lam) e / |e|
    amplitude:  g_den = -P amp / den,  g_u = g_den * 2 u (c - 1),  u -> (s, d) through <A,B>, |A|, |B|
    coupling:   g_c = sum_e (P amp / (2 c) + g_den u^2),  c -> every edge of the body: +-g_c (2 sqrt(c) / E) (s - d) / |s - d|

Zero-subgradient conventions (the reference's autograd is NaN at each of them):
    |e| = 0 (a joint at the radar position)     the phase term of that edge is 0
    |A| = 0, |B| = 0 (a zero-length edge)       d|A|, d|B| = 0
    |u| = 1                                     g_u = 0
    c = 0 (an absent, all-zero body; amp = 0)   every coordinate of that body gets exactly 0
A joint that belongs to no edge gets exactly 0."""
import numpy as np

FLOOR = 2e-5        # the project's per-kernel fp32 tolerance
BAND_FACTOR = 3     # ... or this many times the float32 oracle's own distance from float64


def synthetic_clip(B, T, V=25, M=2, seed=11):
    """tests/golden/make_golden_radar_grad.py's recipe: 0.12 * standard_normal clipped to [-1.1, 0.75], every body present"""
    return np.clip(0.12 * np.random.default_rng(seed).standard_normal((B, 3, T, V, M)), -1.1, 0.75).astype(np.float32)


def cotangent(B, T, seed=5):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, T)).astype(np.float32), g.standard_normal((B, T)).astype(np.float32)


def signal_dx(x, loc, lam, dz_re, dz_im, edges):
    """the hand-written adjoint, float64: x (B,3,T,V,M), loc (3,), lam scalar, dz_re / dz_im (B,T) -> dx (B,3,T,V,M)"""
    x = np.asarray(x, dtype=np.float64)
    loc = np.asarray(loc, dtype=np.float64)
    lam = float(lam)
    src, dst = map(list, zip(*edges))
    E = len(src)
    S, D = x[:, :, :, src], x[:, :, :, dst]                       # (B,3,T,E,M)
    Lc = loc[None, :, None, None, None]
    ur = np.asarray(dz_re, dtype=np.float64)[:, :, None, None]    # (B,T,1,1)
    ui = np.asarray(dz_im, dtype=np.float64)[:, :, None, None]

    def norm(v):
        return np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])

    def edge_sum(v):                                              # over the edge axis in the edges' order, whatever the memory layout
        acc = np.zeros_like(v[:, :, :1])
        for i in range(E):
            acc = acc + v[:, :, i:i + 1]
        return acc

    def safe_div(a, b):
        return np.divide(a, b, out=np.zeros(np.broadcast(a, b).shape), where=(b != 0))

    e = S - Lc
    A = Lc - (S + D) / 2
    Bv = D - S
    dist, nA, nB = norm(e), norm(A), norm(Bv)                     # (B,T,E,M)
    den_u = nA * nB + 1e-6
    u = ((A[:, 0] * Bv[:, 0] + A[:, 1] * Bv[:, 1]) + A[:, 2] * Bv[:, 2]) / den_u
    cbar = edge_sum(nB) / E                                       # (B,T,1,M)
    c = cbar * cbar
    live = c > 0
    su2 = (1 - u) * (1 + u)
    den = su2 + c * u * u
    amp = np.where(live, safe_div(np.sqrt(np.pi * c), np.abs(den)), 0.0)
    psi = 4 * np.pi * dist / lam
    cs, sn = np.cos(psi), np.sin(psi)
    P, Q = ur * cs + ui * sn, ui * cs - ur * sn
    # phase
    gS = (safe_div(amp * Q * (4 * np.pi / lam), dist))[:, None] * e
    # amplitude through u
    gden = -safe_div(P * amp, den)
    gc = edge_sum(safe_div(P * amp, 2 * c) + gden * u * u)
    gu = np.where(su2 > 0, gden * 2 * u * (c - 1), 0.0)
    k0 = (gu / den_u)[:, None]
    ka = (0.5 * u * safe_div(nB, nA))[:, None]
    kb = (u * safe_div(nA, nB))[:, None]
    gS = gS + k0 * (-0.5 * Bv - A + ka * A + kb * Bv)
    gD = k0 * (-0.5 * Bv + A + ka * A - kb * Bv)
    # coupling through c
    k = safe_div(gc * 2 * cbar / E, nB)[:, None]
    gS = gS - k * Bv
    gD = gD + k * Bv
    mask = live[:, None]
    gS, gD = np.where(mask, gS, 0.0), np.where(mask, gD, 0.0)
    dx = np.zeros_like(x)
    for i in range(E):                                            # fixed edge order
        dx[:, :, :, src[i]] += gS[:, :, :, i]
        dx[:, :, :, dst[i]] += gD[:, :, :, i]
    return dx


def autograd_dx(x, loc, lam, dz_re, dz_im, edges, dtype=None):
    """torch autograd through oracle.radar.signal_torch in `dtype` (float64 by default) -> dx as a float64 numpy array"""
    import torch
    from oracle import radar as R
    dtype = dtype or torch.float64
    xt = torch.as_tensor(np.asarray(x)).to(dtype).requires_grad_(True)
    loc_t = torch.as_tensor(np.asarray(loc, dtype=np.float64)).to(dtype)
    lam_t = torch.tensor(float(lam), dtype=dtype)
    zr, zi = R.signal_torch(xt, loc_t, lam_t, edges, dtype)
    (zr * torch.as_tensor(np.asarray(dz_re)).to(dtype) + zi * torch.as_tensor(np.asarray(dz_im)).to(dtype)).sum().backward()
    return xt.grad.double().numpy()


def rel_err(a, ref):
    """norm-wise relative error"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.linalg.norm((a - ref).ravel()) / np.linalg.norm(ref.ravel()))


def within_band(err, band, factor=BAND_FACTOR):
    """the rule of tests/test_gpu_radar.py::test_parameter_gradients_against_reference_autograd with the per-kernel floor"""
    return err < FLOOR or err <= factor * band
