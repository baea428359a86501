#!/usr/bin/env python3
"""Times the backward apply pass of data_bn (sar_data_bn_bwd_apply_f32 / _cn8, csrc/elementwise.hip) and prints the lines of
profiles/input_grad.txt, at the benchmark batch N = 64, C = 3, T = 300, V = 25, M = 2 and for each of the four streams:
  * the kernel alone, warm: both variants, ops.pre_normalize and ops.augment_clips on the same tensor, and the box's float4 copy
    of 1.5 x the clip (read + write = the 3 x 11.5 MB the kernel moves: x read, dh read, dx written), the five launches ALTERNATING
    (A B C D E A B ...), device events around each, the median of --reps launches each after warm-up;
  * the fp32 and the bf16 train step (loss_and_grad + sgd_step) with and without need_dx, blocks of --step-block steps alternating
    in one process, each block ended by a device synchronise, the median block of each.
Usage: python tools/input_grad_bench.py [--reps 200] [--blocks 6] [--step-block 10]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "skeleton-action-recognition_amd"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from sar_amd import _lib, ops, ops8  # noqa: E402
from sar_amd.augment import ClipAugment  # noqa: E402
from sar_amd.bone import NTU_BONE_PAIRS, bone_parent_array  # noqa: E402
from prenorm_bench import raw_clips  # noqa: E402

STREAMS = {"joint": (False, False), "bone": (True, False), "joint_motion": (False, True), "bone_motion": (True, True)}
SHAPE = (64, 3, 300, 25, 2)


def median_us(ev):
    return float(np.median([a.elapsed_time(b) * 1e3 for a, b in ev]))


def kernels(dev, stream, reps, warmup=20):
    """median launch time in us of (apply f32, apply cn8, pre_normalize, augment_clips, float4 copy), alternating"""
    bone, motion = STREAMS[stream]
    N, C, T, V, M = SHAPE
    g = torch.Generator(device="cpu").manual_seed(1)
    raw = torch.from_numpy(raw_clips(N)).to(dev)
    x = ops.pre_normalize(raw)
    parent = torch.from_numpy(bone_parent_array()).to(dev) if bone else None
    dh = torch.randn(C, N * M * T * V, generator=g).to(dev)
    dh8 = ops8.from_cn(dh)
    k = tuple(torch.randn(V * C, generator=g).to(dev) for _ in range(3))
    tab = torch.from_numpy(ClipAugment(seed=0, rot=0.3, scale=0.1, shift=0.2, crop=0.5).table(N, 0, 0)).to(dev)
    dx, dx8, out_p, out_a = (torch.empty_like(x) for _ in range(4))
    ncopy = x.numel() * 3 // 2
    src, dst = torch.ones(ncopy, device=dev), torch.empty(ncopy, device=dev)
    lib = _lib.load()
    launches = [
        lambda: ops.data_bn_bwd_apply(x, parent, dh, k, dx=dx, motion=motion),
        lambda: ops8.data_bn_bwd_apply(x, parent, dh8, k, dx=dx8, motion=motion),
        lambda: ops.pre_normalize(raw, out_p),
        lambda: ops.augment_clips(x, tab, crop=True, out=out_a),
        lambda: _lib.check(lib.sar_box_copy_f32(src.data_ptr(), dst.data_ptr(), ncopy, _lib.stream_ptr()), "sar_box_copy_f32"),
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
    return [median_us(e) for e in ev]


def steps(dev, stream, mode, blocks, block, batch=64):
    """ms per train step without / with need_dx: alternating blocks, each ended by a device synchronise"""
    from sar_amd.stgcn import STGCN
    from sar_amd.train import synthetic_clips
    bone, motion = STREAMS[stream]
    eng = STGCN(num_classes=60, device=dev, seed=0, mfma=mode, bone_pairs=NTU_BONE_PAIRS if bone else None, motion=motion)
    batches = [synthetic_clips(batch, dev, seed=i, num_classes=60) for i in range(2)]
    it = [0]

    def run(n, need_dx):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            x, y = batches[it[0] % 2]
            eng.loss_and_grad(x, y, need_dx=need_dx)
            eng.sgd_step(0.01)
            it[0] += 1
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n * 1e3

    run(10, False), run(10, True)
    plain, with_dx = [], []
    for _ in range(blocks):
        plain.append(run(block, False))
        with_dx.append(run(block, True))
    return np.array(plain), np.array(with_dx)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--step-block", type=int, default=10)
    ap.add_argument("--modes", default="fp32,bf16")
    arg = ap.parse_args()
    assert torch.cuda.is_available(), "input_grad_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    nbytes = 3 * int(np.prod(SHAPE)) * 4
    print("kernels at (N, C, T, V, M) = %s, %d launches each after 20 warm-up rounds, alternating, device events, median in us"
          % (SHAPE, arg.reps))
    print("(the apply pass moves x, dh and dx once: %.1f MB; the CN8 plane is 16 B per position, of which 6 B are read)" % (nbytes / 1e6))
    print("  %-13s %10s %10s %14s %14s %12s" % ("stream", "apply f32", "apply cn8", "pre_normalize", "augment_clips", "copy 34.6 MB"))
    for stream in STREAMS:
        f32, cn8, pre, aug, cp = kernels(dev, stream, arg.reps)
        print("  %-13s %10.1f %10.1f %14.1f %14.1f %12.1f   apply f32 = %.2f x copy, %.2f x pre_normalize, %.2f x augment; %.0f GB/s"
              % (stream, f32, cn8, pre, aug, cp, f32 / cp, f32 / pre, f32 / aug, nbytes / f32 / 1e3))
    print("train step (loss_and_grad + sgd_step) at bs = 64, %d alternating blocks of %d steps, ms per step, median (min .. max):"
          % (arg.blocks, arg.step_block))
    for mode in filter(None, arg.modes.split(",")):
        for stream in STREAMS:
            a, b = steps(dev, stream, mode, arg.blocks, arg.step_block)
            print("  %-5s %-13s without need_dx %8.3f (%.3f .. %.3f)   with need_dx %8.3f (%.3f .. %.3f)   %+.3f ms (%+.2f %%)"
                  % (mode, stream, np.median(a), a.min(), a.max(), np.median(b), b.min(), b.max(), np.median(b) - np.median(a),
                     100 * (np.median(b) / np.median(a) - 1)))


if __name__ == "__main__":
    main()
