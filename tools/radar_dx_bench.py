#!/usr/bin/env python3
"""Measures the skeleton gradient of VirtualRadar (sar_vr_signal_bwd_x_f32, csrc/radar.hip) and writes profiles/radar_input_grad.txt.
Both inputs are plain tensors: a batch of clips (32, 3, 300, 25, 2) and up-sampled data given directly (2, 3, 75000, 25, 2).
  * the kernel alone, warm, beside sar_vr_signal_f32 (the forward), sar_vr_signal_bwd_f32 (the gradient of radar_location /
    wavelength) and the box's float4 copy of the bytes it has to move (x read + dx written), the four launches ALTERNATING
    (A B C D A B ...), device events around each, median (min .. max) of --reps launches after warm-up rounds;
  * the Path B train step through models.resnet.Model under autograd (forward, cross entropy, backward) with and without
    x.requires_grad, blocks of --step-block steps alternating in one process, each block ended by a device synchronise;
  * the error against the float64 oracle and the float32 band of every case of tests/test_gpu_radar_input_grad.py.
--plain-steps N runs N train steps whose x does not require a gradient and nothing else: the program to put under a kernel trace
(with --root another checkout's package is imported, so one trace of each commit gives the two launch lists to compare).
Usage: python tools/radar_dx_bench.py [--reps 100] [--blocks 6] [--step-block 5] [--out profiles/radar_input_grad.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(32, 3, 300, 25, 2), (2, 3, 75000, 25, 2)]


def use_tree(root):
    for p in (os.path.join(root, "tests"), root, os.path.join(root, "skeleton-action-recognition_amd")):
        sys.path.insert(0, p)


def clip(shape, dev, seed=11):
    """tests/golden/make_golden_radar_grad.py's recipe, generated on the host in chunks of one clip"""
    g = np.random.default_rng(seed)
    return torch.stack([torch.from_numpy(np.clip(0.12 * g.standard_normal(shape[1:]), -1.1, 0.75).astype(np.float32))
                        for _ in range(shape[0])]).to(dev)


def stats(ev):
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(t)), float(t.min()), float(t.max())


def kernels(dev, shape, reps, warmup=10):
    """us per launch of (signal forward, d(loc, wavelength), dx, copy of 2 x the clip), alternating: (median, min, max) each"""
    from layers.virtual_radar import VirtualRadar
    from sar_amd import _lib
    from sar_amd._lib import check, ptr, stream_ptr
    lib = _lib.load()
    vr = VirtualRadar(wavelength=5e-4, device=dev)
    x = clip(shape, dev)
    B, _, T, V, M = shape
    g = torch.Generator().manual_seed(5)
    ur, ui = torch.randn(B, T, generator=g).to(dev), torch.randn(B, T, generator=g).to(dev)
    zr, zi = torch.empty_like(ur), torch.empty_like(ui)
    part = torch.empty((lib.sar_vr_signal_bwd_nparts(B, T), 4), device=dev)
    dx = torch.empty_like(x)
    ncopy = x.numel()
    dst = torch.empty(ncopy, device=dev)
    common = (ptr(x), B, T, V, M, ptr(vr._src), ptr(vr._dst), len(vr.src), ptr(vr.radar_location.data), ptr(vr.wavelength.data.reshape(1)))
    launches = [
        lambda: check(lib.sar_vr_signal_f32(*common, ptr(zr), ptr(zi), stream_ptr()), "sar_vr_signal_f32"),
        lambda: check(lib.sar_vr_signal_bwd_f32(*common, ptr(ur), ptr(ui), ptr(part), stream_ptr()), "sar_vr_signal_bwd_f32"),
        lambda: check(lib.sar_vr_signal_bwd_x_f32(*common, ptr(ur), ptr(ui), ptr(dx), stream_ptr()), "sar_vr_signal_bwd_x_f32"),
        lambda: check(lib.sar_box_copy_f32(ptr(x), ptr(dst), ncopy, stream_ptr()), "sar_box_copy_f32"),
    ]
    for _ in range(warmup):
        for fn in launches:
            fn()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)] for _ in launches]
    for r in range(reps):
        for i, fn in enumerate(launches):
            ev[i][r][0].record()
            fn()
            ev[i][r][1].record()
    torch.cuda.synchronize()
    return [stats(e) for e in ev]


def make_step(dev, shape):
    """one Path B train step under autograd: models.resnet.Model forward, cross entropy, backward"""
    from models.resnet import Model
    model = Model(num_classes=60, device=dev)
    model.train()
    x = clip(shape, dev, seed=3)
    y = torch.arange(shape[0], device=dev) % 60

    def run(n, want_x):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            x.requires_grad_(want_x)
            torch.nn.functional.cross_entropy(model(x), y).backward()
            model.zero_grad(set_to_none=True)
            x.grad = None
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3
    return run


def steps(dev, shape, blocks, block):
    run = make_step(dev, shape)
    run(3, False), run(3, True)
    plain, with_dx = [], []
    for _ in range(blocks):
        plain.append(run(block, False))
        with_dx.append(run(block, True))
    return np.array(plain), np.array(with_dx)


def errors(dev, say):
    """engine error and float32 band of every case of tests/test_gpu_radar_input_grad.py"""
    import radar_dx_reference as X
    import test_gpu_radar_input_grad as G
    from oracle import radar as R
    worst = 0.0
    for lam, loc in G.CASES:
        for B, T, M in G.SHAPES:
            x, ur, ui, truth, band = G._signal_truth(lam, loc, B, T, 25, M, tuple(R.EDGES))
            err = X.rel_err(G._run(G._radar(dev, lam, loc), dev, x, ur, ui).cpu().numpy(), truth)
            worst = max(worst, err / max(band, X.FLOOR / X.BAND_FACTOR))
            say("  signal  lambda %-6g (B, T, M) = (%d, %3d, %d)   err %.2e   band %.2e   err / band %.2f" % (lam, B, T, M, err, band, err / band))
    x, ur, ui, truth, band = G._signal_truth(0.1, (0.5, -1.0, 2.0), 2, 9, 7, 4, tuple(G.HUB_EDGES))
    err = X.rel_err(G._run(G._radar(dev, 0.1, (0.5, -1.0, 2.0), edges=G.HUB_EDGES), dev, x, ur, ui).cpu().numpy(), truth)
    say("  custom graph (V = 7, M = 4, hub joint)             err %.2e   band %.2e   err / band %.2f" % (err, band, err / band))
    for lam in (0.1, 5e-4):
        for cols in (0, 32):
            loc, x, w, truth, band = G._e2e_truth(lam, cols)
            vr = G._radar(dev, lam, loc, n_fft=G.N_FFT, hop_length=G.HOP)
            xg = torch.from_numpy(x).to(dev).requires_grad_(True)
            (vr(xg, out_cols=cols) * torch.from_numpy(w).to(dev)).sum().backward()
            err = X.rel_err(xg.grad.cpu().numpy(), truth)
            worst = max(worst, err / max(band, X.FLOOR / X.BAND_FACTOR))
            say("  module  lambda %-6g n_fft 32 hop 4 T 70 out_cols %-2d   err %.2e   band %.2e   err / band %.2f" % (lam, cols, err, band, err / band))
    say("  worst err / max(band, floor / %d) = %.2f (the tests allow %d)" % (X.BAND_FACTOR, worst, X.BAND_FACTOR))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--step-block", type=int, default=5)
    ap.add_argument("--plain-steps", type=int, default=0)
    ap.add_argument("--root", default=os.path.dirname(HERE))
    ap.add_argument("--out", default=os.path.join(os.path.dirname(HERE), "profiles", "radar_input_grad.txt"))
    arg = ap.parse_args()
    use_tree(os.path.abspath(arg.root))
    assert torch.cuda.is_available(), "radar_dx_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    if arg.plain_steps:
        run = make_step(dev, SHAPES[0])
        print("%d plain steps: %.3f ms per step" % (arg.plain_steps, run(arg.plain_steps, False)))
        return
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("device: %s" % torch.cuda.get_device_name(0))
    say("kernels: %d launches each after 10 warm-up rounds, the four alternating, device events, us: median (min .. max)" % arg.reps)
    for shape in SHAPES:
        nbytes = 2 * int(np.prod(shape)) * 4
        f, p, d, c = kernels(dev, shape, arg.reps)
        say("  x %s: dx moves x once in and dx once out = %.1f MB" % (shape, nbytes / 1e6))
        for name, (med, lo, hi) in (("sar_vr_signal_f32", f), ("sar_vr_signal_bwd_f32", p), ("sar_vr_signal_bwd_x_f32", d), ("copy of the same bytes", c)):
            say("    %-26s %9.1f (%.1f .. %.1f)" % (name, med, lo, hi))
        say("    dx = %.2f x forward, %.2f x d(loc, wavelength), %.2f x copy; %.0f GB/s against the copy's %.0f GB/s"
            % (d[0] / f[0], d[0] / p[0], d[0] / c[0], nbytes / d[0] / 1e3, nbytes / c[0] / 1e3))
    say("Path B train step (models.resnet.Model forward, cross entropy, backward; with x.requires_grad the backward adds the stem's data")
    say("gradient, the STFT adjoint and the dx kernel), %d alternating blocks of %d steps, ms per step: median (min .. max)" % (arg.blocks, arg.step_block))
    for shape in SHAPES:
        a, b = steps(dev, shape, arg.blocks, arg.step_block)
        say("  x %-22s without %9.3f (%.3f .. %.3f)   with x.requires_grad %9.3f (%.3f .. %.3f)   %+.3f ms (%+.2f %%)"
            % (shape, np.median(a), a.min(), a.max(), np.median(b), b.min(), b.max(), np.median(b) - np.median(a),
               100 * (np.median(b) / np.median(a) - 1)))
    say("error against the float64 oracle (norm-wise relative) and the band (the float32 oracle's own distance from float64):")
    errors(dev, say)
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
