"""Per-frame trainable adjacency (sar_amd/stgcn_ta.py, csrc/graph_dense_t.hip) against its siblings at bs = 64 (N = 64 clips, M = 2,
T = 300), four fp32 train steps timed round-robin in ONE process:

  (a) STGCN()                              the fp32 headline (fixed adjacency, gather lists)
  (b) STGCN(trainable_adjacency=True)      one shared (K, V, V) adjacency, csrc/graph_dense.hip
  (c) STGCNTA(), train_adjacency = True    one (K, T_i, V, V) table per block, csrc/graph_dense_t.hip
  (d) STGCNTA(), train_adjacency = False   the same, frozen (no dadj launch)

then every new kernel alone, per layer shape, next to the graph_dense_* kernel it stands in for.

  python tools/stgcn_ta_step.py [--rounds 5] [--steps 5]      (output: profiles/stgcn_ta_step.txt)

Bar: median (c) <= median (b) + twice the spread (max - min) of (b)'s own rounds.  (c) / (a) is reported only."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402


def timed(fn, n):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n


def median(v):
    return sorted(v)[len(v) // 2]


def main():
    from sar_amd import ops
    from sar_amd.stgcn import STGCN, KS
    from sar_amd.stgcn_ta import STGCNTA
    from sar_amd.train import synthetic_clips
    argv = sys.argv[1:]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 5
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 5
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    x, y = synthetic_clips(64, dev, seed=0, num_classes=60)
    ta = STGCNTA(num_classes=60, device=dev)
    engines = {"a stgcn": (STGCN(num_classes=60, device=dev, mfma="fp32"), True),
               "b shared-A": (STGCN(num_classes=60, device=dev, trainable_adjacency=True), True),
               "c per-frame": (ta, True), "d frozen": (ta, False)}

    def step(e, train_adj):
        e.train_adjacency = train_adj
        e.loss_and_grad(x, y)
        e.sgd_step(0.01)

    for e, adj in engines.values():
        for _ in range(2):
            step(e, adj)
    torch.cuda.synchronize()
    res = {k: [] for k in engines}
    for r in range(rounds):
        for k, (e, adj) in engines.items():
            res[k].append(timed(lambda: step(e, adj), steps))
    print("train step, bs = 64, fp32, %d rounds x %d steps, interleaved (ms per step):" % (rounds, steps))
    for k, v in res.items():
        print("  %-12s %s   median %.3f  spread %.3f" % (k, " ".join("%.3f" % t for t in v), median(v), max(v) - min(v)))
    mb, mc = median(res["b shared-A"]), median(res["c per-frame"])
    margin = 2 * (max(res["b shared-A"]) - min(res["b shared-A"]))
    print("  bar: (c) %.3f <= (b) %.3f + 2 x spread of (b) %.3f = %.3f : %s" % (mc, mb, margin, mb + margin,
                                                                               "MET" if mc <= mb + margin else "MISSED"))
    print("  ratio (c) / (a) (medians): %.4f   (d) / (c): %.4f" % (mc / median(res["a stgcn"]), median(res["d frozen"]) / mc))
    del engines, ta
    torch.cuda.empty_cache()

    # ---- the kernels alone, B = 128, per layer shape (F, T)
    B, V = 128, 25
    print("\nkernels alone, B = 128, V = 25 (ms per launch, median of 5 x 5 launches): per-frame table | shared table it stands in for")
    g = torch.Generator(device=dev).manual_seed(1)
    tot = {"t": 0.0, "s": 0.0}
    for F, T, count in ((64, 300, 4), (128, 300, 1), (128, 150, 2), (256, 150, 1), (256, 75, 2)):
        n = B * T * V
        y3 = torch.randn((KS * F, n), generator=g, device=dev)
        dout = torch.randn((F, n), generator=g, device=dev)
        out, dy = torch.empty((F, n), device=dev), torch.empty((KS * F, n), device=dev)
        At = torch.randn((KS, T, V, V), generator=g, device=dev) * 0.3
        A = At[:, 0].contiguous()
        dAt, dA = torch.empty_like(At), torch.empty_like(A)
        pairs = {
            "fwd": (lambda: ops.graph_dense_t_fwd(y3, At, out, KS, F, V, B, T, stats=True),
                    lambda: ops.graph_dense_fwd(y3, A, out, KS, F, V, B * T, stats=True)),
            "bwd_data": (lambda: ops.graph_dense_t_bwd_data(dout, At, dy, KS, F, V, B, T),
                         lambda: ops.graph_dense_bwd_data(dout, A, dy, KS, F, V, B * T)),
            "dadj": (lambda: ops.graph_dense_t_dA(y3, dout, dAt, KS, F, V, B, T),
                     lambda: ops.graph_dense_dA(y3, dout, dA, KS, F, V, B * T)),
        }
        gb = {"fwd": 4 * n * (KS * F + F) / 1e9, "bwd_data": 4 * n * (KS * F + F) / 1e9, "dadj": 4 * n * (KS * F + F) / 1e9}
        for name, (ft, fs) in pairs.items():
            ft(), fs()
            torch.cuda.synchronize()
            tt, ts = [], []
            for _ in range(5):
                tt.append(timed(ft, 5))
                ts.append(timed(fs, 5))
            mt, ms = median(tt), median(ts)
            tot["t"] += count * mt
            tot["s"] += count * ms
            print("  F = %3d T = %3d (x%d) %-8s  %.3f  | %.3f   ratio %.2f   activations %.2f GB -> %.2f TB/s"
                  % (F, T, count, name, mt, ms, mt / ms, gb[name], gb[name] / mt))
        del y3, dout, out, dy
        torch.cuda.empty_cache()
    print("  summed over the 10 blocks of a step (block 0 counted at F = 64): per-frame %.3f ms | shared %.3f ms" % (tot["t"], tot["s"]))


if __name__ == "__main__":
    main()
