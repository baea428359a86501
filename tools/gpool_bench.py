"""GPool alone (csrc/gpool.hip through sar_amd.ops), forward + backward, on the activations behind blocks 3 and 9 of ST-GCN at the
benchmark batch -- (N, C, T, V, K, keeprate) = (128, 64, 300, 25, 3, 0.5) and (128, 256, 75, 25, 3, 0.5), 245 MB each -- timed warm
and interleaved with a restatement of the layer in torch ops on the same GPU (transpose, matmul, argsort, gathers, multiply; autograd
for its backward).

  python tools/gpool_bench.py [--runs 12] [--batch 128]      (output: profiles/gpool.txt)

Reported: min and median of the runs, the ratio, the forward / backward split of the kernels, the bytes each pass has to move
(x once per kernel that walks it, the pooled tensors once) and the rate that is of the box's copy rate measured in this process
(sar_amd/box.py)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402


def torch_forward(x, A, p, keep):
    """the layer from torch ops, as the reference writes it"""
    N, C, T, V = x.shape
    K = A.shape[1]
    xr = x.reshape(N, C * T, V).transpose(1, 2)
    ph = p * torch.rsqrt(torch.clamp((p * p).sum(), min=1e-12))
    y = (xr @ ph)[..., 0]
    idx = torch.argsort(y.detach(), dim=1, descending=True, stable=True)[:, :keep]
    s = torch.sigmoid(torch.gather(y, 1, idx))
    xg = torch.gather(xr, 1, idx[:, :, None].expand(-1, -1, C * T)) * s[:, :, None]
    A2 = A @ A
    rows = torch.gather(A2, 2, idx[:, None, :, None].expand(-1, K, -1, V))
    A_out = torch.gather(rows, 3, idx[:, None, None, :].expand(-1, K, keep, -1))
    return xg.transpose(1, 2).reshape(N, C, T, keep), A_out, idx


def main():
    from sar_amd import box, ops
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    runs, N = opt("--runs", 12), opt("--batch", 128)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    copy_gbs = box.copy(dev)
    print("copy rate of this box (float4 copy of 1 GiB, read + write): %.0f GB/s" % copy_gbs)
    print("GPool forward + backward, fp32, %d warm runs each, interleaved (ms); torch = the restatement in torch ops with autograd, "
          "the same batch" % runs)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    for C, T, V, K, keeprate in ((64, 300, 25, 3, 0.5), (256, 75, 25, 3, 0.5)):
        keep = ops.gpool_keep(keeprate, V)
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.relu(torch.randn(N, C, T, V, generator=g, device=dev))
        A = torch.rand(N, K, V, V, generator=g, device=dev) * (torch.rand(N, K, V, V, generator=g, device=dev) < 0.3)
        p = (torch.rand(C * T, 1, generator=g, device=dev) * 2 - 1) * (6.0 / (C * T + 1)) ** 0.5
        dout = torch.randn(N, C, T, keep, generator=g, device=dev)
        dA_out = torch.randn(N, K, keep, keep, generator=g, device=dev)
        out, dx = torch.empty_like(dout), torch.empty_like(x)
        xt, At, pt = x.clone().requires_grad_(), A.clone().requires_grad_(), p.clone().requires_grad_()
        state = {}

        def fwd():
            state["f"] = ops.gpool_forward(x, A, p, keeprate, out=out)

        def bwd():
            state["b"] = ops.gpool_backward(x, A, state["f"][2], dout, dA_out, dx=dx)

        def ours():
            fwd()
            bwd()

        def theirs():
            xt.grad = At.grad = pt.grad = None
            o, Ao, idx = torch_forward(xt, At, pt, keep)
            torch.autograd.backward([o, Ao], [dout, dA_out])
            state["t"] = (o, Ao, idx)

        for _ in range(2):
            ours()
            theirs()
        torch.cuda.synchronize()
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        same = bool(torch.equal(state["f"][2][0].long(), state["t"][2]))
        agree = (rel(out, state["t"][0]), rel(state["f"][1], state["t"][1]), rel(dx, xt.grad), rel(state["b"][1].view(-1, 1), pt.grad),
                 rel(state["b"][2], At.grad))
        t_ours, t_theirs, t_f, t_b = [], [], [], []
        for _ in range(runs):
            t_ours.append(timed(ours))
            t_theirs.append(timed(theirs))
            t_f.append(timed(fwd))
            t_b.append(timed(bwd))
        med = lambda v: sorted(v)[len(v) // 2]
        nx, no = x.numel() * 4, out.numel() * 4
        b_f = 2 * nx + no                               # score reads x; gather reads x (whole sectors) and writes out
        b_b = 2 * nx + 2 * no + nx + N * C * T * 4 * 2   # ds reads x and dout; dx reads x and dout, writes dx and the dph partials (read back)
        print("(N, C, T, V, K, keeprate) = (%d, %d, %d, %d, %d, %g): x %.0f MB, keep %d" % (N, C, T, V, K, keeprate, nx / 1e6, keep))
        print("  kernels   min %8.3f  median %8.3f   (forward median %.3f, backward median %.3f)" % (min(t_ours), med(t_ours), med(t_f), med(t_b)))
        print("  torch     min %8.3f  median %8.3f" % (min(t_theirs), med(t_theirs)))
        print("  ratio torch / kernels (medians): %.2f;  kernels' median below torch's minimum: %s"
              % (med(t_theirs) / med(t_ours), med(t_ours) < min(t_theirs)))
        for what, nbytes, ms in (("forward", b_f, med(t_f)), ("backward", b_b, med(t_b))):
            rate = nbytes / ms / 1e6
            print("  %-8s has to move %.2f GB: %.0f GB/s = %.0f %% of the copy rate (%.3f ms at the copy rate)"
                  % (what, nbytes / 1e9, rate, 100.0 * rate / copy_gbs, nbytes / copy_gbs / 1e6))
        print("  kernels against the torch restatement, max-norm relative: out %.2e  A_out %.2e  dx %.2e  dp %.2e  dA %.2e; idx equal: %s"
              % (agree + (same,)))
        saved_mb = sum(t.numel() * t.element_size() for t in state["f"][2]) / 2 ** 20
        print("  kept for backward besides x and A: %.2f MB" % saved_mb)
        del state, x, dx, xt, out, dout
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
