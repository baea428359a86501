"""ST-PGCN vs ST-GCN fp32 train step at bs = 64 (N = 64 clips, M = 2, T = 300), the two engines timed round-robin in ONE process,
then the projection graph convolution's kernels alone (csrc/pgc.hip) at the same size:

  python tools/stpgcn_step.py [--rounds 4] [--steps 10]      (output: profiles/stpgcn_step.txt)

Layer floor: x (245.8 MB) and q (122.9 MB) -- forward: read x, write q; read x and q, write out; backward: read dout and q; read x,
dout and q, write dx -- about 2.3 GB per step, 0.3 ms at ~8 TB/s."""
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


def main():
    from sar_amd import _lib as L, ops
    from sar_amd.stgcn import STGCN
    from sar_amd.stpgcn import STPGCN
    from sar_amd.train import synthetic_clips
    argv = sys.argv[1:]
    rounds = int(argv[argv.index("--rounds") + 1]) if "--rounds" in argv else 4
    steps = int(argv[argv.index("--steps") + 1]) if "--steps" in argv else 10
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    x, y = synthetic_clips(64, dev, seed=0, num_classes=60)
    engines = {"stgcn": STGCN(num_classes=60, device=dev, mfma="fp32"), "stpgcn": STPGCN(num_classes=60, device=dev)}

    def step(e):
        e.loss_and_grad(x, y)
        e.sgd_step(0.01)

    for e in engines.values():
        for _ in range(3):
            step(e)
    torch.cuda.synchronize()
    res = {k: [] for k in engines}
    for r in range(rounds):
        for k, e in engines.items():
            res[k].append(timed(lambda: step(e), steps))
    print("train step, bs = 64, fp32, %d rounds x %d steps, interleaved (ms per step):" % (rounds, steps))
    for k, v in res.items():
        print("  %-7s %s   median %.3f" % (k, " ".join("%.3f" % t for t in v), sorted(v)[len(v) // 2]))
    ratio = sorted(res["stpgcn"])[rounds // 2] / sorted(res["stgcn"])[rounds // 2]
    print("  ratio stpgcn / stgcn (medians): %.4f" % ratio)
    del engines
    torch.cuda.empty_cache()

    # ---- the layer alone, B = 128, P = 7 500
    lib = L.load()
    B, P = 128, 300 * 25
    g = torch.Generator(device=dev).manual_seed(1)
    xc = torch.relu(torch.randn((64, B * P), generator=g, device=dev))
    dout = torch.randn((64, B * P), generator=g, device=dev)
    cen = 0.5 * torch.randn((1, 64, 1, 32), generator=g, device=dev)
    var = 0.5 * torch.randn((1, 64, 1, 32), generator=g, device=dev)
    W = 0.2 * torch.randn((1, 64, 64), generator=g, device=dev)
    bias = torch.zeros(64, device=dev)
    out, dx = torch.empty_like(xc), torch.empty_like(xc)
    gc, gv, gwb = torch.empty_like(cen), torch.empty_like(var), torch.empty(64 * 64 + 64, device=dev)
    G = lib.sar_pgc_nparts(P)
    q = torch.empty((32, B * P), device=dev)
    fpart = torch.empty((B, G, ops.PGC_FWD_PART), device=dev)
    saved = torch.empty((B, ops.PGC_SAVED), device=dev)
    dpart = torch.empty((B, G, ops.PGC_DH_PART), device=dev)
    dsaved = torch.empty((B, ops.PGC_DSAVED), device=dev)
    slab = torch.empty((B, ops.PGC_SLAB), device=dev)
    cpart = torch.empty((B, G, ops.PGC_BWD_PART), device=dev)
    sp = L.stream_ptr()
    p_ = L.ptr
    kernels = {
        "assign": lambda: lib.sar_pgc_assign_f32(p_(xc), B * P, B, P, p_(cen), p_(var), p_(q), p_(fpart), sp),
        "small_fwd": lambda: lib.sar_pgc_small_fwd_f32(p_(fpart), B, G, p_(cen), p_(var), p_(W), p_(bias), p_(saved), sp),
        "project": lambda: lib.sar_pgc_project_f32(p_(xc), B * P, p_(q), p_(saved), B, P, p_(out), B * P, sp),
        "bwd_reduce": lambda: lib.sar_pgc_bwd_reduce_f32(p_(dout), B * P, p_(q), B, P, p_(dpart), sp),
        "small_bwd": lambda: lib.sar_pgc_small_bwd_f32(p_(dpart), B, G, p_(var), p_(W), p_(saved), p_(dsaved), p_(slab), sp),
        "bwd_column": lambda: lib.sar_pgc_bwd_column_f32(p_(xc), B * P, p_(dout), B * P, p_(q), p_(saved), p_(dsaved), p_(cen), p_(var),
                                                         B, P, p_(dx), B * P, p_(cpart), sp),
    }
    for fn in kernels.values():      # in order once: every input of the next kernel exists
        L.check(fn())
    torch.cuda.synchronize()
    print("\nProjectionGraphConv(64, 32) alone, B = 128, P = 7 500 (ms per launch, 20 launches each):")
    tot = 0.0
    for k, fn in kernels.items():
        t = timed(fn, 20)
        tot += t
        print("  %-11s %.3f" % (k, t))
    fwd = timed(lambda: ops.pgc_forward(xc, B, P, cen, var, W, bias, out), 20)
    q2, sv2 = ops.pgc_forward(xc, B, P, cen, var, W, bias, out)
    bwd = timed(lambda: ops.pgc_backward(xc, dout, q2, sv2, B, P, cen, var, W, dx, gc, gv, gwb), 20)
    print("  kernels summed %.3f ms; ops.pgc_forward %.3f ms, ops.pgc_backward %.3f ms (incl. slab reductions), layer %.3f ms"
          % (tot, fwd, bwd, fwd + bwd))
    print("  HBM floor of the layer ~0.3 ms (2.3 GB at ~8 TB/s)")


if __name__ == "__main__":
    main()
