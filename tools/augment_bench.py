#!/usr/bin/env python3
"""Times sar_augment_clips_f32 (csrc/augment.hip) and prints the lines of profiles/augment.txt:
  * the kernel on a training batch N = 64, T = 300, V = 25, M = 2 with everything on (rot, scale, shift, crop, moving key frames),
    and ops.pre_normalize on the same batch in the same run, launches ALTERNATING (A B A B ...), device events around each, the
    median of --reps launches each after warm-up.  Both read the batch once (twice counting the null-frame sweep, which hits the
    cache) and write it once; the bar is 2 x the pre_normalize time of THIS run;
  * the numpy float32 restatement tests/augment_reference.py in clips/s on one host core next to the kernel's rate;
  * the worst distance from the float64 restatement on 8 clips of that batch, in the units of tests/test_gpu_augment.py;
  * the ST-GCN bf16 train step at bs = 64 with and without ClipAugment in front of it, blocks of --step-block steps alternating in
    one process, the median block of each (reported, not gated), and what the table copy + launch take on the stream inside them.
Usage: python tools/augment_bench.py [--reps 200] [--blocks 6] [--step-block 20]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "skeleton-action-recognition_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))):
    sys.path.insert(0, p)
from sar_amd import ops  # noqa: E402
from sar_amd.augment import ClipAugment  # noqa: E402
import augment_reference as A  # noqa: E402
from prenorm_bench import raw_clips  # noqa: E402

FULL = dict(rot=0.3, scale=0.1, shift=0.2, crop=0.5)


def stats(ev):
    t = np.array([a.elapsed_time(b) * 1e3 for a, b in ev])
    return float(np.median(t)), float(t.min()), float(np.percentile(t, 90))


def time_interleaved(raw, x, tab, reps, warmup=20):
    """(augment, pre_normalize) launch times in us, the two kernels alternating"""
    out_a, out_p = torch.empty_like(x), torch.empty_like(x)
    for _ in range(warmup):
        ops.augment_clips(x, tab, crop=True, out=out_a)
        ops.pre_normalize(raw, out_p)
    ev_a = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    ev_p = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for (a0, a1), (p0, p1) in zip(ev_a, ev_p):
        a0.record()
        ops.augment_clips(x, tab, crop=True, out=out_a)
        a1.record()
        p0.record()
        ops.pre_normalize(raw, out_p)
        p1.record()
    torch.cuda.synchronize()
    return stats(ev_a), stats(ev_p)


def step_cost(dev, blocks, block, batch=64):
    """the bf16 ST-GCN step with / without augmentation: per-step ms of alternating blocks, each ended by a device synchronise"""
    from sar_amd.stgcn import STGCN
    from sar_amd.train import Trainer, synthetic_clips
    eng = STGCN(num_classes=60, device=dev, seed=0, mfma="bf16")
    trainer = Trainer(eng, batch_size=batch, world_size=1)
    batches = [synthetic_clips(batch, dev, seed=i, num_classes=60) for i in range(4)]
    aug = ClipAugment(seed=0, **FULL)
    it, on_stream, on_host = [0], [], []

    def run(n, augment, keep=False):
        torch.cuda.synchronize()
        ev = []
        t0 = time.perf_counter()
        for _ in range(n):
            x, y = batches[it[0] % 4]
            if augment:                                       # events around (table copy + launch) as the stream sees them
                ev.append((torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)))
                h0 = time.perf_counter()
                ev[-1][0].record()
                x = aug(x, 0, it[0])
                ev[-1][1].record()
                if keep:
                    on_host.append((time.perf_counter() - h0) * 1e6)
            trainer.step(x, y)
            it[0] += 1
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t0) / n * 1e3
        if keep:
            on_stream.extend(a.elapsed_time(b) * 1e3 for a, b in ev)
        return dt

    run(30, False), run(30, True)
    plain, with_aug = [], []
    for _ in range(blocks):
        plain.append(run(block, False))
        with_aug.append(run(block, True, keep=True))
    return np.array(plain), np.array(with_aug), float(np.median(on_stream)), float(np.median(on_host))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--step-block", type=int, default=20)
    arg = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench.py measures on the GPU"
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(0))
    N = 64
    raw = torch.from_numpy(raw_clips(N)).to(dev)
    x = ops.pre_normalize(raw)                                # what the augmentation sees in training: padded, centred clips
    tabh = ClipAugment(seed=0, **FULL).table(N, 0, 0)
    tab = torch.from_numpy(tabh).to(dev)
    (med, lo, p90), (pmed, plo, pp90) = time_interleaved(raw, x, tab, arg.reps)
    nbytes = 2 * x.numel() * 4
    print("N = %d T = 300 V = 25 M = 2, %d launches each, alternating, device events:" % (N, arg.reps))
    print("  augment_clips (rot, scale, shift, crop, moving): median %.1f us (min %.1f, p90 %.1f), %.1f MB moved, %.0f GB/s"
          % (med, lo, p90, nbytes / 1e6, nbytes / med / 1e3))
    print("  pre_normalize:                                   median %.1f us (min %.1f, p90 %.1f)" % (pmed, plo, pp90))
    print("  bar: at most 2 x pre_normalize of this run = %.1f us -> %s (%.2f x)" % (2 * pmed, "met" if med <= 2 * pmed else "MISSED", med / pmed))
    (rmed, _, _), _ = time_interleaved(raw, raw, tab, arg.reps)
    print("  augment_clips on the RAW batch (trailing null frames, L < T): median %.1f us" % rmed)
    xh = x.cpu().numpy()
    k = 8
    t0 = time.perf_counter()
    f32 = A.augment(xh[:k], tabh[:k], True, "float32")
    cpu = k / (time.perf_counter() - t0)
    print("  numpy float32 restatement, one host core: %.0f clips/s; the kernel: %.0f clips/s (%.0f x)" % (cpu, N / med * 1e6, N / med * 1e6 / cpu))
    ref, bar = A.bound(xh[:k], tabh[:k], True)
    got = ops.augment_clips(x[:k].contiguous(), tab[:k].contiguous(), crop=True).cpu().numpy()
    live = ref != 0
    print("  worst distance from the float64 restatement (%d clips): kernel %.2f, numpy float32 %.2f units of 2^-24 (|joint| s_max + d_max); bar 8"
          % (k, (np.abs(got - ref)[live] / bar[live]).max() * 8, (np.abs(f32 - ref)[live] / bar[live]).max() * 8))
    plain, with_aug, on_stream, on_host = step_cost(dev, arg.blocks, arg.step_block)
    print("ST-GCN bf16 step, bs = 64, %d alternating blocks of %d steps (ms per step):" % (arg.blocks, arg.step_block))
    print("  without augmentation: median %.3f (min %.3f, max %.3f)" % (np.median(plain), plain.min(), plain.max()))
    print("  with ClipAugment:     median %.3f (min %.3f, max %.3f)  -> %+.3f ms per step (%+.2f %%)"
          % (np.median(with_aug), with_aug.min(), with_aug.max(), np.median(with_aug) - np.median(plain),
             100 * (np.median(with_aug) / np.median(plain) - 1)))
    print("  inside those steps, table copy + launch between two events on the stream: median %.1f us; the host's share of a step "
          "(Philox draw, pinned staging, two enqueues): median %.1f us" % (on_stream, on_host))


if __name__ == "__main__":
    main()
