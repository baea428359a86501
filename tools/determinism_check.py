#!/usr/bin/env python3
"""Run-to-run determinism of the whole train step at the bench size: the kernels use no atomics and every reduction has
a fixed order, so logits, loss and every gradient must be BITWISE identical between repetitions -- a mismatch means a
race (LDS hazard, missing barrier).  Usage: python tools/determinism_check.py [--reps 5] [--batch 64]

--digest prints, per mode, the SHA-256 of logits, loss, grad and flat after each of two loss_and_grad + sgd_step rounds and of
predict(x): two commits that print the same lines on the same machine and library compute the same steps.  The modes resnet,
resnet_f32_split and resnet_f32_split_bf16x6 digest Path B's classifier (num_filters 64, a fixed (4, 1, 64, 64) input: the smallest
at which all four stages, the down-sampling branches, the K-split of the small feature maps and the stride-2 parity classes run):
loss_and_grad(need_dx=True) + adam_step, dx as well, and the logits of forward(training=False).  For these and for fp32 / bf16 a
second pass on a fresh engine hands its gradient buckets to a callback that records (bucket, lo, hi): the hand-over order is
printed and the digests once more ("<mode>+buckets")."""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402

from sar_amd.stgcn import STGCN  # noqa: E402
from sar_amd.train import synthetic_clips  # noqa: E402


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def digest(mode, eng, x, y, record_buckets=False):
    resnet, kw, order = mode.startswith("resnet"), {}, []
    if record_buckets:
        mode += "+buckets"
        kw["bucket_cb"] = lambda bi, flat, events: order.append(
            (bi, (flat.data_ptr() - eng.grad.data_ptr()) // 4, (flat.data_ptr() - eng.grad.data_ptr()) // 4 + flat.numel()))
    for step in range(2):
        out = eng.loss_and_grad(x, y, need_dx=True, **kw) if resnet else eng.loss_and_grad(x, y, **kw)
        eng.adam_step(1e-3) if resnet else eng.sgd_step(0.1)
        torch.cuda.synchronize()
        for name, t in (("logits", out[0]), ("loss", out[1])) + ((("dx", out[2]),) if resnet else ()) + (("grad", eng.grad), ("flat", eng.flat)):
            print("%s step%d %s %s" % (mode, step, name, sha(t)))
    probs = eng.forward(x, training=False) if resnet else eng.predict(x)
    torch.cuda.synchronize()
    print("%s predict %s" % (mode, sha(probs)))
    if record_buckets:
        print("%s order %s" % (mode, ";".join("%d:%d-%d" % o for o in order)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--modes", default="fp32,bf16")
    ap.add_argument("--digest", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    total_bad = 0
    modes = a.modes.split(",")
    if a.digest:
        modes += [m + "+buckets" for m in modes if m in ("fp32", "bf16") or m.startswith("resnet")]
    for mode in modes:
        mode, buckets = mode.split("+")[0], mode.endswith("+buckets")
        bad = 0
        if mode.startswith("resnet"):      # Path B's classifier at its bench shape (bs 32, 256 x 256 spectrograms; --digest: see above)
            from sar_amd.resnet import ResNet18
            eng = ResNet18(num_classes=60, num_filters=64, device=dev, seed=0, mfma=mode[7:] or None)
            g = torch.Generator(device=dev).manual_seed(5)
            n, hw = (4, 64) if a.digest else (32, 256)
            x, y = torch.randn((n, 1, hw, hw), generator=g, device=dev), torch.randint(0, 60, (n,), generator=g, device=dev)
        elif mode == "stgin":
            from sar_amd.stgin import STGIN
            eng = STGIN(num_classes=60, device=dev, seed=0)
            x, y = synthetic_clips(a.batch, dev, seed=3, num_classes=60)
        elif mode in ("stpgcn", "stgcn_ta"):      # the sibling engines (fp32): the layer between two blocks / per-frame adjacencies
            from sar_amd.stgcn_ta import STGCNTA
            from sar_amd.stpgcn import STPGCN
            eng = (STPGCN if mode == "stpgcn" else STGCNTA)(num_classes=60, device=dev, seed=0)
            x, y = synthetic_clips(a.batch, dev, seed=3, num_classes=60)
        elif mode in ("dense", "bone_motion"):     # trainable adjacency (dense contraction kernels) / bone + motion input streams
            from sar_amd.bone import NTU_BONE_PAIRS
            kw = dict(trainable_adjacency=True) if mode == "dense" else dict(bone_pairs=NTU_BONE_PAIRS, motion=True)
            eng = STGCN(num_classes=60, device=dev, seed=0, mfma="fp32", **kw)
            x, y = synthetic_clips(a.batch, dev, seed=3, num_classes=60)
        else:
            eng = STGCN(num_classes=60, device=dev, seed=0, mfma=mode)
            x, y = synthetic_clips(a.batch, dev, seed=3, num_classes=60)
        if a.digest:
            digest(mode, eng, x, y, buckets)
            continue
        state = {k: v.clone() for k, v in eng.state_dict().items()}
        ref = None
        for r in range(a.reps):
            eng.load_params(state)
            logits, loss = eng.loss_and_grad(x, y)[:2]
            torch.cuda.synchronize()
            cur = (logits.clone(), loss.clone(), eng.grad.clone())
            if ref is None:
                ref = cur
            else:
                same = all(torch.equal(p, q) for p, q in zip(ref, cur))
                if not same:
                    bad += 1
                    d = (ref[2] - cur[2]).abs().max().item()
                    names = []
                    for k in eng.shapes:      # which tensors differ
                        o, n = eng.offsets[k], 1
                        for v in eng.shapes[k]:
                            n *= v
                        dk = (ref[2][o:o + n] - cur[2][o:o + n]).abs().max().item()
                        if dk > 0:
                            names.append("%s %.2e" % (k, dk))
                    print("%s rep %d: MISMATCH (max |grad diff| %.3e; logits equal %s) %s" %
                          (mode, r, d, torch.equal(ref[0], cur[0]), ", ".join(names[:12]) + (" ... %d tensors" % len(names) if len(names) > 12 else "")))
        print("%s: %d repetitions, loss %.6f, %s" % (mode, a.reps, ref[1].item(), "bitwise identical" if bad == 0 else "NOT deterministic (%d)" % bad))
        total_bad += bad
    sys.exit(1 if total_bad else 0)


if __name__ == "__main__":
    main()
