"""ProjectionGraphPool alone (csrc/pgpool.hip through sar_amd.ops), forward + backward, at the two pools of ST-PGCNP at the benchmark
batch -- (B, C, P, J) = (128, 256, 950, 512) and (128, 256, 512, 256) -- timed warm and interleaved with a PyTorch-on-GPU
restatement that does not materialise z either: the same arithmetic from torch ops, the (B, C, P, j) tensor formed for `--chunk`
vertices at a time (float32).

  python tools/pgpool_bench.py [--runs 12] [--chunk 8] [--batch 128]      (output: profiles/pgpool.txt)

Reported: min and median of the runs, the ratio of the medians, the forward / backward split of the kernels."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402

EPS = 1e-12


def torch_pool(x, cen, s, dz, dA, chunk):
    """forward + backward of the layer from torch ops, x (B, C, P), cen / s (C, J); vertices in chunks -> (zn, A, dx, dcen, dvar)"""
    B, C, P = x.shape
    J = cen.shape[1]
    r = 1.0 / s
    d = torch.empty((B, P, J), dtype=x.dtype, device=x.device)
    for j0 in range(0, J, chunk):
        z = (x[..., None] - cen[None, :, None, j0:j0 + chunk]) * r[None, :, None, j0:j0 + chunk]
        d[..., j0:j0 + chunk] = (z * z).sum(1)
    q = torch.softmax(torch.clamp(d, min=EPS) * -0.5, -1)
    S = torch.einsum("bcp,bpj->bcj", x, q)
    qs = q.sum(1)[:, None, :]
    zp = (S - cen * qs) / (s * qs)
    n2 = (zp * zp).sum(-1)
    n = torch.sqrt(torch.clamp(n2, min=EPS))
    zn = zp / n[..., None]
    A = torch.einsum("bci,bcj->bij", zn, zn)
    dzn = dz + torch.einsum("bci,bij->bcj", zn, dA + dA.transpose(1, 2))
    dot = (dzn * zn).sum(-1, keepdim=True)
    dzp = torch.where((n2 > EPS)[..., None], dzn - zn * dot, dzn) / n[..., None]
    dS = dzp / (s * qs)
    dqs = -(dS * S / qs).sum(1)
    dcen = -(dzp / s).sum(0)
    ds = -(dzp * zp / s).sum(0)
    dq = torch.einsum("bcp,bcj->bpj", x, dS) + dqs[:, None, :]
    dl = q * (dq - (q * dq).sum(-1, keepdim=True))
    dl = torch.where(d > EPS, dl, torch.zeros_like(dl))
    dx = torch.einsum("bpj,bcj->bcp", q, dS)
    for j0 in range(0, J, chunk):
        rr = r[None, :, None, j0:j0 + chunk]
        z = (x[..., None] - cen[None, :, None, j0:j0 + chunk]) * rr
        t = dl[:, None, :, j0:j0 + chunk] * z * rr
        dx -= t.sum(-1)
        dcen[:, j0:j0 + chunk] += t.sum((0, 2))
        ds[:, j0:j0 + chunk] += (t * z).sum((0, 2))
    return zn, A, dx, dcen, ds * s * (1 - s)


def main():
    from sar_amd import ops
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    runs, chunk, B = opt("--runs", 12), opt("--chunk", 8), opt("--batch", 128)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    print("ProjectionGraphPool forward + backward, fp32, %d warm runs each, interleaved (ms); torch = the restatement in torch ops, "
          "%d vertices per chunk, the same batch" % (runs, chunk))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for C, P, J in ((256, 950, 512), (256, 512, 256)):
        g = torch.Generator(device=dev).manual_seed(0)
        X = torch.relu(torch.randn(C, B * P, generator=g, device=dev))
        lim = (6.0 / (C + J * C)) ** 0.5
        cen = (torch.rand(1, C, 1, J, generator=g, device=dev) * 2 - 1) * lim
        var = (torch.rand(1, C, 1, J, generator=g, device=dev) * 2 - 1) * lim
        dz = torch.randn(B, C, J, generator=g, device=dev)
        dA = torch.randn(B, J, J, generator=g, device=dev)
        dX, dcen, dvar = torch.empty_like(X), torch.empty_like(cen), torch.empty_like(var)
        x3 = X.reshape(C, B, P).permute(1, 0, 2).contiguous()
        cen2, s2 = cen.reshape(C, J), torch.sigmoid(var.reshape(C, J))
        state = {}

        def fwd():
            state["f"] = ops.pgpool_forward(X, B, P, cen, var)

        def bwd():
            zn, _, saved = state["f"]
            ops.pgpool_backward(X, B, P, cen, zn, saved, dz, dA, dX, dcen, dvar)

        def ours():
            fwd()
            bwd()

        def theirs():
            state["t"] = torch_pool(x3, cen2, s2, dz, dA, chunk)

        for _ in range(2):
            ours()
            theirs()
        torch.cuda.synchronize()
        zn, A = state["f"][0], state["f"][1]
        tz, tA, tdx = state["t"][:3]
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        agree = (rel(zn, tz), rel(A, tA), rel(dX.reshape(C, B, P).permute(1, 0, 2), tdx))
        t_ours, t_theirs, t_f, t_b = [], [], [], []
        for _ in range(runs):
            t_ours.append(timed(ours))
            t_theirs.append(timed(theirs))
            t_f.append(timed(fwd))
            t_b.append(timed(bwd))
        med = lambda v: sorted(v)[len(v) // 2]
        flops = 2.0 * B * P * J * C * (1.5 + 1 + 1 + 3 + 2) + 2.0 * B * J * J * C * 3
        print("(B, C, P, J) = (%d, %d, %d, %d)" % (B, C, P, J))
        print("  kernels   min %8.3f  median %8.3f   (forward median %.3f, backward median %.3f; %.1f TFLOP/s on %.3f TFLOP)"
              % (min(t_ours), med(t_ours), med(t_f), med(t_b), flops / med(t_ours) / 1e9, flops / 1e12))
        print("  torch     min %8.3f  median %8.3f" % (min(t_theirs), med(t_theirs)))
        print("  ratio torch / kernels (medians): %.2f" % (med(t_theirs) / med(t_ours)))
        print("  kernels against the torch restatement, max-norm relative: zn %.2e  A_out %.2e  dx %.2e" % agree)
        saved_mb = sum(t.numel() * t.element_size() for t in state["f"][2]) / 2 ** 20 + zn.numel() * 4 / 2 ** 20
        print("  kept for backward besides x: %.1f MB (q %.1f MB)" % (saved_mb, state["f"][2][0].numel() * 4 / 2 ** 20))
        del state, X, x3, dX
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
