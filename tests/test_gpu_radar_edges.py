"""The VirtualRadar kernels (csrc/radar.hip) through the C ABI at the shapes where their index arithmetic can go wrong -- strided
loops past one trip, launch widths that are no multiple of a wave or of a row block, both reflections in one frame, hops past the
frame, column selects that repeat or drop frames, tile tails, the LDS limit, smoothing radii past the clip -- each against the float64
oracle (oracle/radar.py, pinned at these shapes by tests/test_radar_edge_reference.py), with every buffer between poisoned margins.

Criterion (tests/test_gpu_radar.py's): truth = the oracle in float64; band = distance of the oracle's own float32 run from it at the
same shape and input; every quantity must satisfy err <= max(3 band, floor), err = max |a - truth| / max |truth|, on magnitudes
exp(out) - 1e-6 for spectrograms.  Floors: 1e-5 magnitude from a given z, 1e-4 magnitude through the signal stage, 2e-5 of scale for z,
2e-3 for every gradient.

Guard bands: every output / workspace is a guarded_flat range (tests/util.py), every input sits between NaN (edge lists: out-of-range)
margins.  Each case runs once with NaN-filled and once with sentinel-filled outputs: margins bit-unchanged, no live output element
still holds the fill, results finite, and the two runs bitwise equal (launch-to-launch determinism)."""
import numpy as np
import pytest
import torch

from oracle import radar as R
from radar_edges import (KERNEL_SHAPES, LAM, LOC, LOG_EPS, MODULE_CLIP, SIGNAL_SHAPES, STFT_SHAPES, UPSAMPLE_SHAPES, clip, edge_list,
                         eval_pieces, fourier_kernels, normal, signal_edge_kinds)
from util import NAN, SENTINEL, _bits, assert_flat_guards_untouched, guarded_flat

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
EDGE_SENTINEL = 1 << 30          # margins of the int32 edge lists: a joint index far outside any clip
FLOOR_MAG, FLOOR_MAG_SIGNAL, FLOOR_Z, FLOOR_GRAD = 1e-5, 1e-4, 2e-5, 2e-3

# The spline pieces are float64 work: evaluated at np.linspace(0, 1, P*T) against scipy.interpolate.interp1d('cubic') on scipy's own
# float32-smoothed series, error = max |difference| / max |scipy's value|.  Measured on the MI355X over UPSAMPLE_SHAPES (all three
# modes): 1.9e-16 .. 2.9e-16 at T = 5, 1.4e-15 at T = 9, 7.9e-15 at T = 304 (LDS solve), 9.13e-15 at T = 305 (global-scratch solve) --
# the worst is COEF_MEASURED; the bound is 4x that (the input-dependent rounding of a T-step Thomas recurrence).
COEF_MEASURED = 9.13e-15
COEF_BOUND = 4 * COEF_MEASURED


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def lib():
    from sar_amd._lib import load
    return load()


def ok(rc, what):
    from sar_amd._lib import check
    check(rc, what)


def sp():
    from sar_amd._lib import stream_ptr
    return stream_ptr()


def p(t):
    return None if t is None else t.data_ptr()


class Guarded:
    """the buffers of one run: inputs between NaN margins, outputs and workspaces between margins of `fill` and filled with it"""

    def __init__(self, dev, fill):
        self.dev, self.fill, self.outs, self.wss, self.full, self.inputs = dev, fill, {}, {}, {}, []

    def inp(self, a, dtype=F32):
        t = torch.from_numpy(np.ascontiguousarray(a)).to(dtype)
        view, whole = guarded_flat(t, NAN if dtype.is_floating_point else EDGE_SENTINEL, self.dev, dtype=dtype)
        self.inputs.append(whole)          # (an input built inside a call's argument list lives as long as the run)
        return view

    def out(self, name, n, dtype=F32):
        self.outs[name] = guarded_flat(int(n), self.fill, self.dev, dtype=dtype)
        return self.outs[name][0]

    def ws(self, name, n, written=False):
        """a workspace of exactly its advertised size (in floats); written: every element of it is an output of the call"""
        (self.full if written else self.wss)[name] = guarded_flat(int(n), self.fill, self.dev)
        return (self.full if written else self.wss)[name][0]

    def holds_fill(self, t):
        return _bits(t) == _bits(torch.full((1,), self.fill, dtype=t.dtype, device=t.device))

    def check(self):
        for name, (view, whole) in list(self.outs.items()) + list(self.wss.items()) + list(self.full.items()):
            assert_flat_guards_untouched(whole, view.numel(), self.fill, what="%s (fill %r)" % (name, self.fill))
        for name, (view, _) in list(self.outs.items()) + list(self.full.items()):
            assert not bool(self.holds_fill(view).any()), "%s: %d live elements still hold the fill %r" % (
                name, int(self.holds_fill(view).sum()), self.fill)
            assert bool(torch.isfinite(view).all()), "%s (fill %r): not finite" % (name, self.fill)

    def check_nothing_written(self):
        for name, (view, whole) in list(self.outs.items()) + list(self.wss.items()) + list(self.full.items()):
            assert bool(self.holds_fill(whole).all()), "%s: written by a rejected call" % name

    def results(self):
        return {name: view.cpu().numpy().copy() for name, (view, _) in self.outs.items()}


def drive(dev, fn):
    """fn(g) launches on the buffers of g: once with NaN-filled, once with sentinel-filled outputs -> the (bitwise equal) results"""
    runs = []
    for fill in (NAN, SENTINEL):
        g = Guarded(dev, fill)
        fn(g)
        torch.cuda.synchronize()
        g.check()
        runs.append(g.results())
    assert set(runs[0]) == set(runs[1])
    for name in runs[0]:
        assert np.array_equal(runs[0][name], runs[1][name]), "%s: the NaN-filled and the sentinel-filled run differ" % name
    return runs[0]


def dist(a, t):
    a, t = np.asarray(a, dtype=np.float64), np.asarray(t, dtype=np.float64)
    s = np.abs(t).max()
    return np.abs(a - t).max() / (s if s > 0 else 1.0)


def mag(logspec):
    return np.exp(np.asarray(logspec, dtype=np.float64)) - 1e-6


def judge(case, name, hip, f32, f64, floor, magnitude=False):
    if magnitude:
        hip, f32, f64 = mag(hip), mag(f32), mag(f64)
    err, band = dist(hip, f64), dist(f32, f64)
    print("radar-edges %s %-7s: HIP %.2e from the float64 oracle (oracle float32: %.2e, floor %.0e)" % (case, name, err, band, floor))
    assert np.shape(hip) == np.shape(f64), (case, name)
    assert err <= max(3 * band, floor), "%s %s: %.3e > max(3 x %.3e, %.0e)" % (case, name, err, band, floor)


def window32(n_fft):
    return R.hann_periodic(n_fft).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- STFT stages

def stft_ref(zr, zi, n_fft, hop, out_cols, dout, wcos=None, wsin=None):
    """{dtype: out, dz (2,B,T), dw (2,n_fft,n_fft) or None} from autograd through oracle.radar.stft_torch"""
    res = {}
    for dt in (F64, F32):
        a, b = torch.from_numpy(zr).to(dt).requires_grad_(), torch.from_numpy(zi).to(dt).requires_grad_()
        wc = ws = None
        if wcos is not None:
            wc, ws = torch.from_numpy(wcos).to(dt).requires_grad_(), torch.from_numpy(wsin).to(dt).requires_grad_()
        out = R.stft_torch(a, b, n_fft, hop, out_cols, dt, wc, ws)
        (out * torch.from_numpy(dout).to(dt)).sum().backward()
        res[dt] = dict(out=out.detach().numpy(), dz=np.stack([a.grad.numpy(), b.grad.numpy()]),
                       dw=None if wc is None else np.stack([wc.grad.numpy(), ws.grad.numpy()]))
    return res


def read_samples(T, n_fft, hop, out_cols):
    """(T,) bool: the samples some CONSUMED frame reads, directly or through the reflect padding"""
    half, F_ = n_fft // 2, T // hop + 1
    idx = np.pad(np.arange(T), (half, half), mode="reflect")
    frames = range(F_) if out_cols == 0 else sorted(set(R.nearest_columns(F_, out_cols).tolist()))
    read = np.zeros(T, dtype=bool)
    for f in frames:
        read[idx[f * hop:f * hop + n_fft]] = True
    return read


def run_stft(dev, lib, zr, zi, n_fft, hop, out_cols, dout):
    B, T = zr.shape
    nc = out_cols if out_cols > 0 else T // hop + 1

    def fn(g):
        a, b, w = g.inp(zr), g.inp(zi), g.inp(window32(n_fft))
        out = g.out("out", B * n_fft * nc)
        ok(lib.sar_stft_logmag_f32(p(a), p(b), B, T, n_fft, hop, p(w), out_cols, p(out), sp()), "sar_stft_logmag_f32")
        nws = lib.sar_stft_logmag_bwd_workspace_floats(B, T, n_fft, hop)
        assert nws == B * (T // hop + 1) * n_fft * 2
        ws = g.ws("workspace", nws, written=True)
        dzr, dzi = g.out("dz_re", B * T), g.out("dz_im", B * T)
        ok(lib.sar_stft_logmag_bwd_f32(p(a), p(b), B, T, n_fft, hop, p(w), out_cols, p(g.inp(dout)), p(ws), p(dzr), p(dzi), sp()),
           "sar_stft_logmag_bwd_f32")
    r = drive(dev, fn)
    return dict(out=r["out"].reshape(B, n_fft, nc), dz=np.stack([r["dz_re"], r["dz_im"]]).reshape(2, B, T))


STFT_CASES = [(T, n, h, c, B) for T, n, h, c, Bs, _ in STFT_SHAPES for B in Bs]


@pytest.mark.parametrize("T,n_fft,hop,out_cols,B", STFT_CASES, ids=["T%d-n%d-h%d-c%d-B%d" % c for c in STFT_CASES])
def test_closed_form_stft_forward_and_backward(dev, lib, T, n_fft, hop, out_cols, B):
    """sar_stft_logmag_f32 / sar_stft_logmag_bwd_f32: output and dz against autograd through the float64 oracle; samples that no
    consumed frame reads get exactly zero gradient; clip b of a batch is bitwise the clip alone; silence is exactly log(1e-6)"""
    case = "stft T%d n%d h%d c%d B%d" % (T, n_fft, hop, out_cols, B)
    zr, zi = normal((B, T), 100 + T).astype(np.float32), normal((B, T), 200 + T).astype(np.float32)
    nc = out_cols if out_cols > 0 else T // hop + 1
    dout = normal((B, n_fft, nc), 300 + T).astype(np.float32)
    got = run_stft(dev, lib, zr, zi, n_fft, hop, out_cols, dout)
    ref = stft_ref(zr, zi, n_fft, hop, out_cols, dout)
    judge(case, "|Z|", got["out"], ref[F32]["out"], ref[F64]["out"], FLOOR_MAG, magnitude=True)
    judge(case, "dz", got["dz"], ref[F32]["dz"], ref[F64]["dz"], FLOOR_GRAD)
    unread = ~read_samples(T, n_fft, hop, out_cols)
    if hop > n_fft:
        assert unread.any(), "the case is there for samples no frame reads"
    assert not got["dz"][:, :, unread].any(), "a sample no consumed frame reads has a gradient"
    assert not ref[F64]["dz"][:, :, unread].any()
    if B > 1:
        for b in range(B):
            one = run_stft(dev, lib, zr[b:b + 1], zi[b:b + 1], n_fft, hop, out_cols, dout[b:b + 1])
            assert np.array_equal(one["out"][0], got["out"][b]) and np.array_equal(one["dz"][:, 0], got["dz"][:, b]), "clip %d" % b
    else:
        zero = np.zeros((1, T), np.float32)
        sil = run_stft(dev, lib, zero, zero, n_fft, hop, out_cols, dout)
        assert (sil["out"] == np.float32(LOG_EPS)).all() and not sil["dz"].any()


def splits_of(BF):
    odd = next(n for n in range(2, BF + 3) if BF % n)
    return [1, odd, BF, BF + 3]


def run_kernels(dev, lib, zr, zi, n_fft, hop, out_cols, dout, wcos, wsin, nsplits, both_modes=True):
    """out, and per nsplit: dw (2, n_fft, n_fft) and dz -- dw once more with dz_re = dz_im = NULL, bitwise the same"""
    B, T = zr.shape
    F_ = T // hop + 1
    nc = out_cols if out_cols > 0 else F_
    wcosT, wsinT = np.ascontiguousarray(wcos.T), np.ascontiguousarray(wsin.T)

    def fwd(g):
        out = g.out("out", B * n_fft * nc)
        ok(lib.sar_stft_kernels_fwd_f32(p(g.inp(zr)), p(g.inp(zi)), B, T, n_fft, hop, p(g.inp(wcosT)), p(g.inp(wsinT)), out_cols,
                                        p(out), sp()), "sar_stft_kernels_fwd_f32")
    res = dict(out=drive(dev, fwd)["out"].reshape(B, n_fft, nc), dw={}, dz={})
    for nsplit in nsplits:
        for with_dz in ((True, False) if both_modes else (True,)):
            def bwd(g):
                nws = lib.sar_stft_kernels_bwd_workspace_floats(B, T, n_fft, hop, nsplit)
                assert nws == B * F_ * n_fft * 4 + nsplit * 2 * n_fft * n_fft
                ws = g.ws("workspace", nws, written=with_dz)      # (the frame cotangents are not computed without dz)
                dw = g.out("dw", 2 * n_fft * n_fft)
                dzr = g.out("dz_re", B * T) if with_dz else None
                dzi = g.out("dz_im", B * T) if with_dz else None
                ok(lib.sar_stft_kernels_bwd_f32(p(g.inp(zr)), p(g.inp(zi)), B, T, n_fft, hop, p(g.inp(wcos)), p(g.inp(wsin)),
                                                p(g.inp(wcosT)), p(g.inp(wsinT)), out_cols, p(g.inp(dout)), p(ws), nsplit, p(dw), p(dzr),
                                                p(dzi), sp()), "sar_stft_kernels_bwd_f32")
            r = drive(dev, bwd)
            dw = r["dw"].reshape(2, n_fft, n_fft)
            if with_dz:
                res["dw"][nsplit] = dw
                res["dz"][nsplit] = np.stack([r["dz_re"], r["dz_im"]]).reshape(2, B, T)
            else:
                assert np.array_equal(dw, res["dw"][nsplit]), "nsplit %d: dw differs between dz given and dz NULL" % nsplit
    return res


KERNEL_CASES = [(T, n, h, c, B, v) for T, n, h, c, Bs, _ in KERNEL_SHAPES for B in Bs for v in ("analytic", "perturbed")]


@pytest.mark.parametrize("T,n_fft,hop,out_cols,B,variant", KERNEL_CASES, ids=["T%d-n%d-h%d-c%d-B%d-%s" % c for c in KERNEL_CASES])
def test_trainable_kernel_stft_forward_and_backward(dev, lib, T, n_fft, hop, out_cols, B, variant):
    """sar_stft_kernels_fwd_f32 / sar_stft_kernels_bwd_f32 at nsplit in {1, one that does not divide B F, B F, B F + 3 (empty
    splits)}, with and without dz: output, dz and dw against autograd through the float64 oracle"""
    case = "kernels T%d n%d h%d c%d B%d %s" % (T, n_fft, hop, out_cols, B, variant)
    zr, zi = normal((B, T), 400 + T).astype(np.float32), normal((B, T), 500 + T).astype(np.float32)
    F_ = T // hop + 1
    nc = out_cols if out_cols > 0 else F_
    dout = normal((B, n_fft, nc), 600 + T).astype(np.float32)
    wcos, wsin = fourier_kernels(n_fft, variant)
    nsplits = splits_of(B * F_)
    assert nsplits[1] > 1 and (B * F_) % nsplits[1] != 0
    got = run_kernels(dev, lib, zr, zi, n_fft, hop, out_cols, dout, wcos, wsin, nsplits)
    ref = stft_ref(zr, zi, n_fft, hop, out_cols, dout, wcos, wsin)
    judge(case, "|Z|", got["out"], ref[F32]["out"], ref[F64]["out"], FLOOR_MAG, magnitude=True)
    for nsplit in nsplits:
        judge(case + " nsplit %d" % nsplit, "dz", got["dz"][nsplit], ref[F32]["dz"], ref[F64]["dz"], FLOOR_GRAD)
        judge(case + " nsplit %d" % nsplit, "dw", got["dw"][nsplit], ref[F32]["dw"], ref[F64]["dw"], FLOOR_GRAD)
        assert np.array_equal(got["dz"][nsplit], got["dz"][nsplits[0]])          # dz does not depend on the split
    unread = ~read_samples(T, n_fft, hop, out_cols)
    assert not got["dz"][1][:, :, unread].any()
    if variant != "analytic":
        return
    if B > 1:
        for b in range(B):
            one = run_kernels(dev, lib, zr[b:b + 1], zi[b:b + 1], n_fft, hop, out_cols, dout[b:b + 1], wcos, wsin, [1], both_modes=False)
            assert np.array_equal(one["out"][0], got["out"][b]) and np.array_equal(one["dz"][1][:, 0], got["dz"][1][:, b]), "clip %d" % b
    else:
        zero = np.zeros((1, T), np.float32)
        sil = run_kernels(dev, lib, zero, zero, n_fft, hop, out_cols, dout, wcos, wsin, [nsplits[1]], both_modes=False)
        assert (sil["out"] == np.float32(LOG_EPS)).all() and not sil["dz"][nsplits[1]].any() and not sil["dw"][nsplits[1]].any()


# ---------------------------------------------------------------------------------------------------------------- signal stage

def signal_ref(x, edges, dzr, dzi, dt):
    """z (2,B,T) and d <dz, z> / d (loc, lam) from autograd through oracle.radar.signal_torch in dtype dt; x may be float64"""
    loc, lam = torch.tensor(LOC, dtype=dt, requires_grad=True), torch.tensor(LAM, dtype=dt, requires_grad=True)
    zr, zi = R.signal_torch(torch.from_numpy(np.asarray(x)), loc, lam, edges, dt)
    ((zr * torch.from_numpy(dzr).to(dt)).sum() + (zi * torch.from_numpy(dzi).to(dt)).sum()).backward()
    return dict(z=np.stack([zr.detach().numpy(), zi.detach().numpy()]), dloc=loc.grad.numpy(), dlam=lam.grad.numpy())


def run_signal(dev, lib, x, edges, dzr, dzi):
    B, _, T, V, M = x.shape
    src, dst = (np.array(e, dtype=np.int32) for e in zip(*edges))
    E = len(edges)

    def fn(g):
        xd, es, ed = g.inp(x), g.inp(src, torch.int32), g.inp(dst, torch.int32)
        loc, lam = g.inp(np.array(LOC, np.float32)), g.inp(np.array([LAM], np.float32))
        zr, zi = g.out("z_re", B * T), g.out("z_im", B * T)
        ok(lib.sar_vr_signal_f32(p(xd), B, T, V, M, p(es), p(ed), E, p(loc), p(lam), p(zr), p(zi), sp()), "sar_vr_signal_f32")
        nparts = lib.sar_vr_signal_bwd_nparts(B, T)
        assert nparts == B * ((T + 63) // 64)
        part = g.out("partials", nparts * 4)
        ok(lib.sar_vr_signal_bwd_f32(p(xd), B, T, V, M, p(es), p(ed), E, p(loc), p(lam), p(g.inp(dzr)), p(g.inp(dzi)), p(part), sp()),
           "sar_vr_signal_bwd_f32")
    r = drive(dev, fn)
    grad = r["partials"].reshape(-1, 4).astype(np.float64).sum(0)
    return dict(z=np.stack([r["z_re"], r["z_im"]]).reshape(2, B, T), dloc=grad[:3], dlam=grad[3])


def judge_signal(case, got, x32, x64, edges, dzr, dzi):
    r32, r64 = signal_ref(x32, edges, dzr, dzi, F32), signal_ref(x64, edges, dzr, dzi, F64)
    judge(case, "z", got["z"], r32["z"], r64["z"], FLOOR_Z)
    judge(case, "dloc", got["dloc"], r32["dloc"], r64["dloc"], FLOOR_GRAD)
    judge(case, "dlam", got["dlam"], r32["dlam"], r64["dlam"], FLOOR_GRAD)


SIGNAL_CASES = [(T, V, M, E, B, fast) for T, V, M, E, _ in SIGNAL_SHAPES for B in (1, 3) for fast in ("0", "1")]


@pytest.mark.parametrize("T,V,M,E,B,fast", SIGNAL_CASES, ids=["T%d-V%d-M%d-E%d-B%d-fastplain%s" % c for c in SIGNAL_CASES])
def test_signal_forward_and_backward(dev, lib, monkeypatch, T, V, M, E, B, fast):
    """sar_vr_signal_f32 (literal and, with SAR_VR_FAST_PLAIN=1, the up-sampled path's arithmetic) / sar_vr_signal_bwd_f32"""
    monkeypatch.setenv("SAR_VR_FAST_PLAIN", fast)
    for kind in signal_edge_kinds(E):
        case = "signal T%d V%d M%d E%d B%d %s fastplain%s" % (T, V, M, E, B, kind, fast)
        edges = edge_list(V, E, kind)
        x = clip((B, 3, T, V, M), 700 + T + V)
        dzr, dzi = normal((B, T), 800 + T).astype(np.float32), normal((B, T), 900 + T).astype(np.float32)
        got = run_signal(dev, lib, x, edges, dzr, dzi)
        judge_signal(case, got, x, x, edges, dzr, dzi)
        if fast == "1" and T >= 63:      # the switch is read on every call: the other arithmetic gives other bits
            monkeypatch.setenv("SAR_VR_FAST_PLAIN", "0")
            literal = run_signal(dev, lib, x, edges, dzr, dzi)
            monkeypatch.setenv("SAR_VR_FAST_PLAIN", "1")
            assert not np.array_equal(literal["z"], got["z"]) and np.array_equal(literal["dloc"], got["dloc"])
        if B > 1:
            total = np.zeros(4)
            for b in range(B):
                one = run_signal(dev, lib, x[b:b + 1], edges, dzr[b:b + 1], dzi[b:b + 1])
                assert np.array_equal(one["z"][:, 0], got["z"][:, b]), "clip %d" % b
                total += np.append(one["dloc"], one["dlam"])
            whole = np.append(got["dloc"], got["dlam"])
            assert np.abs(total - whole).max() <= FLOOR_GRAD * np.abs(whole).max()
        else:
            sil = run_signal(dev, lib, np.zeros_like(x), edges, dzr, dzi)
            assert not sil["z"].any() and not sil["dloc"].any() and sil["dlam"] == 0


# ---------------------------------------------------------------------------------------------------------------- up-sampling

def run_upsample(dev, lib, x, P, sigma, edges, dzr, dzi):
    from layers.virtual_radar import gaussian_weights
    B, _, T, V, M = x.shape
    src, dst = (np.array(e, dtype=np.int32) for e in zip(*edges))
    E, Tup = len(edges), T * P
    w, radius = gaussian_weights(sigma)
    assert radius == int(4.0 * sigma + 0.5)
    ncoef = lib.sar_upsample_coef_doubles(B, T, V, M)
    nbytes = lib.sar_upsample_workspace_bytes(B, T, V, M)
    assert ncoef == B * (T - 1) * 3 * V * M * 4 and nbytes == B * 3 * V * M * T * 20

    def prepare(g):
        ws = g.ws("workspace", nbytes // 4)
        coef = g.out("coef", ncoef, F64)
        ok(lib.sar_upsample_prepare_f64(p(g.inp(x)), B, T, V, M, p(g.inp(w, F64)), radius, p(ws), p(coef), sp()), "sar_upsample_prepare_f64")
    coef = drive(dev, prepare)["coef"]

    def signal(g):
        cf, es, ed = g.inp(coef, F64), g.inp(src, torch.int32), g.inp(dst, torch.int32)
        loc, lam = g.inp(np.array(LOC, np.float32)), g.inp(np.array([LAM], np.float32))
        zr, zi = g.out("z_re", B * Tup), g.out("z_im", B * Tup)
        ok(lib.sar_vr_signal_upsampled_f32(p(cf), B, T, P, V, M, p(es), p(ed), E, p(loc), p(lam), p(zr), p(zi), sp()),
           "sar_vr_signal_upsampled_f32")
        part = g.out("partials", lib.sar_vr_signal_bwd_nparts(B, Tup) * 4)
        ok(lib.sar_vr_signal_upsampled_bwd_f32(p(cf), B, T, P, V, M, p(es), p(ed), E, p(loc), p(lam), p(g.inp(dzr)), p(g.inp(dzi)),
                                               p(part), sp()), "sar_vr_signal_upsampled_bwd_f32")
    r = drive(dev, signal)
    grad = r["partials"].reshape(-1, 4).astype(np.float64).sum(0)
    return dict(coef=coef, z=np.stack([r["z_re"], r["z_im"]]).reshape(2, B, Tup), dloc=grad[:3], dlam=grad[3])


UPSAMPLE_CASES = [s[:6] + (mode,) for s in UPSAMPLE_SHAPES for mode in ("default", "SAR_UPSAMPLE_LDS=0", "SAR_VR_FAST=0")
                  if mode == "default" or s[1] in (5, 9)]


@pytest.mark.parametrize("B,T,V,M,P,sigma,mode", UPSAMPLE_CASES, ids=["B%d-T%d-V%d-M%d-P%d-s%g-%s" % c for c in UPSAMPLE_CASES])
def test_upsampling_prepare_signal_and_backward(dev, lib, monkeypatch, B, T, V, M, P, sigma, mode):
    """sar_upsample_prepare_f64 (spline pieces against scipy on its own float32-smoothed series), sar_vr_signal_upsampled_f32 and
    ..._bwd_f32 (against the oracle on the scipy-up-sampled clip; truth = float64 end to end); the global-scratch solve gives
    bitwise the pieces of the LDS solve"""
    case = "upsample B%d T%d V%d M%d P%d sigma%g %s" % (B, T, V, M, P, sigma, mode)
    for name in ("SAR_UPSAMPLE_LDS", "SAR_VR_FAST"):
        monkeypatch.delenv(name, raising=False)
    edges = edge_list(V, 1 if V == 2 else 5, "shared")
    x = clip((B, 3, T, V, M), 1000 + T + P)
    Tup = T * P
    dzr, dzi = normal((B, Tup), 1100 + T).astype(np.float32), normal((B, Tup), 1200 + T).astype(np.float32)
    base = run_upsample(dev, lib, x, P, sigma, edges, dzr, dzi) if mode == "SAR_UPSAMPLE_LDS=0" else None
    if mode != "default":
        monkeypatch.setenv(*mode.split("="))
    got = run_upsample(dev, lib, x, P, sigma, edges, dzr, dzi)
    if base is not None:
        assert np.array_equal(base["coef"], got["coef"]), "the global-scratch solve differs from the LDS solve"
        assert np.array_equal(base["z"], got["z"])
    _, up = R.pad_frames_parts(x, P, sigma)                  # scipy on the float32-smoothed series, float64, not rounded
    err = dist(eval_pieces(got["coef"], B, T, P, V, M), up)
    print("radar-edges %s coef   : HIP pieces %.2e from scipy's spline of the float32-smoothed series (bound %.2e)" % (case, err, COEF_BOUND))
    up64 = R.pad_frames_parts(x.astype(np.float64), P, sigma)[1]
    judge_signal(case, got, up.astype(np.float32), up64, edges, dzr, dzi)
    if B > 1:
        total = np.zeros(4)
        for b in range(B):
            one = run_upsample(dev, lib, x[b:b + 1], P, sigma, edges, dzr[b:b + 1], dzi[b:b + 1])
            n = one["coef"].size
            assert np.array_equal(one["coef"], got["coef"][b * n:(b + 1) * n]) and np.array_equal(one["z"][:, 0], got["z"][:, b]), b
            total += np.append(one["dloc"], one["dlam"])
        whole = np.append(got["dloc"], got["dlam"])
        assert np.abs(total - whole).max() <= FLOOR_GRAD * np.abs(whole).max()
    else:
        sil = run_upsample(dev, lib, np.zeros_like(x), P, sigma, edges, dzr, dzi)
        assert not sil["coef"].any() and not sil["z"].any() and not sil["dloc"].any() and sil["dlam"] == 0
    assert err <= COEF_BOUND, "spline pieces: %.3e from scipy, bound %.3e" % (err, COEF_BOUND)


# ---------------------------------------------------------------------------------------------------------------- rejections

def _rejections():
    """name -> fn(g, lib) issuing ONE call that must be refused; every buffer is as large as an accepted call would need"""
    cases = {}
    es5, ed5 = (np.array(e, dtype=np.int32) for e in zip(*edge_list(7, 5, "shared")))
    loc, lam = np.array(LOC, np.float32), np.array([LAM], np.float32)

    def stft(T, n_fft, hop):
        def fn(g, lib):
            z = g.inp(normal((1, T), 1))
            return lib.sar_stft_logmag_f32(p(z), p(z), 1, T, n_fft, hop, p(g.inp(np.ones(n_fft, np.float32))), 0,
                                           p(g.out("out", n_fft * (T + 1))), sp())
        return fn

    def stft_bwd(T, n_fft, hop):
        def fn(g, lib):
            z, nf = g.inp(normal((1, T), 1)), T + 1
            return lib.sar_stft_logmag_bwd_f32(p(z), p(z), 1, T, n_fft, hop, p(g.inp(np.ones(n_fft, np.float32))), 0,
                                               p(g.inp(np.ones(n_fft * nf, np.float32))), p(g.ws("workspace", 2 * n_fft * nf)),
                                               p(g.out("dz_re", T)), p(g.out("dz_im", T)), sp())
        return fn

    def kern(T, n_fft, hop):
        def fn(g, lib):
            z, w = g.inp(normal((1, T), 1)), g.inp(np.ones(n_fft * n_fft, np.float32))
            return lib.sar_stft_kernels_fwd_f32(p(z), p(z), 1, T, n_fft, hop, p(w), p(w), 0, p(g.out("out", n_fft * (T + 1))), sp())
        return fn

    def kern_bwd(T, n_fft, hop, null=None):
        def fn(g, lib):
            z, w, nf = g.inp(normal((1, T), 1)), g.inp(np.ones(n_fft * n_fft, np.float32)), T + 1
            dzr = None if null == "dz_re" else g.out("dz_re", T)
            dzi = None if null == "dz_im" else g.out("dz_im", T)
            return lib.sar_stft_kernels_bwd_f32(p(z), p(z), 1, T, n_fft, hop, p(w), p(w), p(w), p(w), 0, p(g.inp(np.ones(n_fft * nf, np.float32))),
                                                p(g.ws("workspace", 4 * n_fft * nf + 2 * n_fft * n_fft)), 1,
                                                p(g.out("dw", 2 * n_fft * n_fft)), p(dzr), p(dzi), sp())
        return fn

    def signal(T, V, M, edges, E=None, bwd=False):
        def fn(g, lib):
            src, dst = (np.array(e, dtype=np.int32) for e in zip(*edges))
            n = len(edges) if E is None else E
            x = g.inp(clip((1, 3, T, V, M), 2))
            if bwd:
                dz = g.inp(normal((1, T), 3))
                return lib.sar_vr_signal_bwd_f32(p(x), 1, T, V, M, p(g.inp(src, torch.int32)), p(g.inp(dst, torch.int32)), n, p(g.inp(loc)),
                                                 p(g.inp(lam)), p(dz), p(dz), p(g.out("partials", 4 * ((T + 63) // 64))), sp())
            return lib.sar_vr_signal_f32(p(x), 1, T, V, M, p(g.inp(src, torch.int32)), p(g.inp(dst, torch.int32)), n, p(g.inp(loc)),
                                         p(g.inp(lam)), p(g.out("z_re", T)), p(g.out("z_im", T)), sp())
        return fn

    def upsampled(T, P, which):
        def fn(g, lib):
            V, M, Tup = 7, 3, T * max(P, 1)
            if which == "prepare":
                assert lib.sar_upsample_workspace_bytes(1, T, V, M) == -1 and lib.sar_upsample_coef_doubles(1, T, V, M) == -1
                return lib.sar_upsample_prepare_f64(p(g.inp(clip((1, 3, T, V, M), 2))), 1, T, V, M, p(g.inp(np.ones(1), F64)), 0,
                                                    p(g.ws("workspace", 3 * V * M * T * 5)), p(g.out("coef", T * 3 * V * M * 4, F64)), sp())
            cf = g.inp(np.zeros(T * 3 * V * M * 4), F64)
            args = (p(cf), 1, T, P, V, M, p(g.inp(es5, torch.int32)), p(g.inp(ed5, torch.int32)), 5, p(g.inp(loc)), p(g.inp(lam)))
            if which == "signal":
                return lib.sar_vr_signal_upsampled_f32(*args, p(g.out("z_re", Tup)), p(g.out("z_im", Tup)), sp())
            dz = g.inp(normal((1, Tup), 3))
            return lib.sar_vr_signal_upsampled_bwd_f32(*args, p(dz), p(dz), p(g.out("partials", 4 * ((Tup + 63) // 64))), sp())
        return fn

    cases["T == n_fft/2 (closed form)"] = stft(8, 16, 4)
    cases["T == n_fft/2 (closed form, backward)"] = stft_bwd(8, 16, 4)
    cases["T == n_fft/2 (kernels)"] = kern(8, 16, 4)
    cases["T == n_fft/2 (kernels, backward)"] = kern_bwd(8, 16, 4)
    cases["odd n_fft (closed form)"] = stft(12, 15, 4)
    cases["odd n_fft (closed form, backward)"] = stft_bwd(12, 15, 4)
    cases["odd n_fft (kernels)"] = kern(12, 17, 4)
    cases["odd n_fft (kernels, backward)"] = kern_bwd(12, 17, 4)
    cases["n_fft = 2050 (closed form)"] = stft(1100, 2050, 512)
    cases["n_fft = 2050 (closed form, backward)"] = stft_bwd(1100, 2050, 512)
    cases["n_fft = 1026 (kernels)"] = kern(600, 1026, 256)
    cases["n_fft = 1026 (kernels, backward)"] = kern_bwd(600, 1026, 256)
    cases["n_fft = 14 (kernels, backward)"] = kern_bwd(10, 14, 4)
    cases["hop = 0 (closed form)"] = stft(12, 16, 0)
    cases["hop = 0 (closed form, backward)"] = stft_bwd(12, 16, 0)
    cases["hop = 0 (kernels)"] = kern(12, 16, 0)
    cases["hop = 0 (kernels, backward)"] = kern_bwd(12, 16, 0)
    cases["M = 5"] = signal(8, 3, 5, [(0, 1), (1, 2)])
    cases["M = 5 (backward)"] = signal(8, 3, 5, [(0, 1), (1, 2)], bwd=True)
    cases["E = 0"] = signal(8, 3, 2, [(0, 1), (1, 2)], E=0)
    cases["E = 0 (backward)"] = signal(8, 3, 2, [(0, 1), (1, 2)], E=0, bwd=True)
    cases["T = 4 (prepare)"] = upsampled(4, 2, "prepare")
    cases["T = 4 (up-sampled signal)"] = upsampled(4, 2, "signal")
    cases["T = 4 (up-sampled backward)"] = upsampled(4, 2, "backward")
    cases["P = 0 (up-sampled signal)"] = upsampled(6, 0, "signal")
    cases["P = 0 (up-sampled backward)"] = upsampled(6, 0, "backward")
    cases["dz_re NULL alone"] = kern_bwd(12, 16, 4, null="dz_re")
    cases["dz_im NULL alone"] = kern_bwd(12, 16, 4, null="dz_im")
    cases["E = 33 past 64 KiB of LDS"] = signal(70, 21, 4, edge_list(21, 33, "both"))
    cases["E = 33 past 64 KiB of LDS (backward)"] = signal(70, 21, 4, edge_list(21, 33, "both"), bwd=True)
    return cases


REJECTIONS = _rejections()


@pytest.mark.parametrize("name", list(REJECTIONS))
def test_rejected_calls_launch_nothing(dev, lib, name):
    """the call returns the error code, no buffer is written, and the stream takes the next (valid) call"""
    for fill in (NAN, SENTINEL):
        g = Guarded(dev, fill)
        rc = REJECTIONS[name](g, lib)
        torch.cuda.synchronize()
        assert rc != 0 and lib.sar_last_error_string(), name
        g.check_nothing_written()
    zr, zi = normal((1, 12), 5).astype(np.float32), normal((1, 12), 6).astype(np.float32)
    dout = normal((1, 16, 4), 7).astype(np.float32)
    got = run_stft(dev, lib, zr, zi, 16, 4, 0, dout)
    ref = stft_ref(zr, zi, 16, 4, 0, dout)
    assert dist(mag(got["out"]), mag(ref[F64]["out"])) <= FLOOR_MAG


def test_the_lds_limit_is_exactly_64_kib():
    """V = 21, M = 4: 3 x 64 rows of pitch (84 | 1) floats + 2 E edge indices = 65 536 bytes at E = 32"""
    assert 4 * 3 * 64 * ((21 * 4) | 1) + 4 * 2 * 32 == 64 * 1024


# ---------------------------------------------------------------------------------------------------------------- the module

@pytest.mark.parametrize("out_cols", [0, 9])
def test_module_away_from_the_workload_shapes(dev, out_cols):
    """VirtualRadar(n_fft=30, hop_length=7, 5 edges, everything trainable): the wrapper's F, workspace sizes and nsplit"""
    from layers.virtual_radar import VirtualRadar
    edges = edge_list(7, 5, "shared")
    x = clip(MODULE_CLIP, 1300)
    vr = VirtualRadar(edges=edges, wavelength=LAM, radar_location=list(LOC), train_wavelength=True, train_radar_location=True,
                      train_stft_kernel=True, n_fft=30, hop_length=7, device=dev)
    out = vr(torch.from_numpy(x).to(dev), out_cols=out_cols)
    nc = out_cols if out_cols else 23 // 7 + 1
    assert tuple(out.shape) == (2, 30, nc)
    w = normal((2, 30, nc), 1301).astype(np.float32)
    (out * torch.from_numpy(w).to(dev)).sum().backward()
    torch.cuda.synchronize()
    got = dict(out=out.detach().cpu().numpy(), dloc=vr.radar_location.grad.cpu().numpy(), dlam=vr.wavelength.grad.cpu().numpy(),
               dwcos=vr.stft.wcos.grad.cpu().numpy()[:, 0], dwsin=vr.stft.wsin.grad.cpu().numpy()[:, 0])
    wcos0, wsin0 = vr.stft.wcos.detach().cpu().numpy()[:, 0], vr.stft.wsin.detach().cpu().numpy()[:, 0]
    ref = {}
    for dt in (F64, F32):
        loc, lam = torch.tensor(LOC, dtype=dt, requires_grad=True), torch.tensor(LAM, dtype=dt, requires_grad=True)
        wc, ws = torch.from_numpy(wcos0).to(dt).requires_grad_(), torch.from_numpy(wsin0).to(dt).requires_grad_()
        o = R.spectrogram_torch(x, loc, lam, edges=edges, n_fft=30, hop=7, out_cols=out_cols, dtype=dt, wcos=wc, wsin=ws)
        (o * torch.from_numpy(w).to(dt)).sum().backward()
        ref[dt] = dict(out=o.detach().numpy(), dloc=loc.grad.numpy(), dlam=lam.grad.numpy(), dwcos=wc.grad.numpy(), dwsin=ws.grad.numpy())
    case = "module n30 h7 c%d" % out_cols
    for name in ("out", "dloc", "dlam", "dwcos", "dwsin"):
        judge(case, name, got[name], ref[F32][name], ref[F64][name], FLOOR_MAG_SIGNAL if name == "out" else FLOOR_GRAD, magnitude=name == "out")
