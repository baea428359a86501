"""AdaptiveAdjacency alone (csrc/adjattn.hip through sar_amd.ops), forward + backward, at the two benchmark activations --
(N, C, T, V) = (128, 64, 300, 25) with K = 3, Ce = 16 and (128, 256, 75, 25) with Ce = 64 -- timed warm and interleaved with the same layer
written in torch ops under autograd (conv -> matmul -> softmax over axis -2) on the same GPU.

  python tools/adjattn_bench.py [--runs 12] [--batch 128]      (output: profiles/adjattn.txt)

Reported: min and median of the runs through ops (CN matrix in, CN gradient out: what an engine would call) and through the module
(NCHW <-> CN at its boundary), the forward / backward split, each kernel and each 1x1 product on its own, the ratio to the torch-ops
layer, and each MFMA kernel's ratio to its floor at this box's copy rate (sar_amd/box.py, measured in this process): the similarity
reads theta and phi once, the embeddings' gradient reads them once and writes dtheta and dphi once.  theta.kernel is scaled so that the
logits have a per-column standard deviation of 2, as in the tests."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402


def torch_layer(x, A, tk, pk, pb):
    """the layer in torch ops; tk, pk (C, K Ce)"""
    N, C, T, V = x.shape
    K = A.shape[0]
    Ce = tk.shape[1] // K
    theta = torch.nn.functional.conv2d(x, tk.t().reshape(-1, C, 1, 1))
    phi = torch.nn.functional.conv2d(x, pk.t().reshape(-1, C, 1, 1), pb)
    S = torch.matmul(theta.view(N, K, Ce * T, V).transpose(2, 3), phi.view(N, K, Ce * T, V)) / (Ce * T)
    return A + torch.softmax(S, dim=-2), S


def main():
    from models.agcn import AdaptiveAdjacency
    from models.gcn import to_cn
    from sar_amd import _lib as L
    from sar_amd import box, ops
    from sar_amd._lib import check, ptr, stream_ptr
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    runs, N = opt("--runs", 12), opt("--batch", 128)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    copy_gbs = box.copy(dev)
    print("this box: copy rate (float4 copy of 1 GiB, read + write) %.0f GB/s" % copy_gbs)
    print("AdaptiveAdjacency forward + backward (x and A require a gradient), fp32, K = 3, %d warm runs each, interleaved (ms); torch = the "
          "layer in torch ops under autograd, the same batch" % runs)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    med = lambda v: sorted(v)[len(v) // 2]
    K = 3
    for (C, T, V), Ce in (((64, 300, 25), 16), ((256, 75, 25), 64)):
        g = torch.Generator(device=dev).manual_seed(0)
        r = lambda shape: torch.randn(shape, generator=g, device=dev)
        x, dA_eff, A = r((N, C, T, V)), r((N, K, V, V)), 0.3 * torch.rand(K, V, V, generator=g, device=dev)
        tk, pk, pb = r((C, K * Ce)) / C ** 0.5, r((C, K * Ce)) / C ** 0.5, 0.1 * r((K * Ce,))
        tk = tk * (2.0 / float(torch_layer(x, A, tk, pk, pb)[1].std(dim=2, unbiased=False).mean()))
        tk4, pk4 = tk.reshape(1, 1, C, -1), pk.reshape(1, 1, C, -1)
        X = to_cn(x)
        n, kce = N * T * V, K * Ce
        state = {}

        def fwd():
            state["f"] = ops.adjattn_forward(X, N, T, V, A, tk4, pk4, pb)

        def bwd():
            state["b"] = ops.adjattn_backward(X, N, T, V, state["f"][1], tk4, pk4, dA_eff)

        def ours():
            fwd()
            bwd()

        layer = AdaptiveAdjacency(Ce, K)
        layer.load_state_dict({"theta.kernel": tk4, "phi.kernel": pk4, "phi.bias": pb})
        xm, Am = x.clone().requires_grad_(), A.clone().requires_grad_()

        def module():
            state["m"] = torch.autograd.grad(layer(xm, Am), [xm, Am] + list(layer.parameters()), dA_eff)

        leaves = [t.clone().requires_grad_() for t in (x, A, tk, pk, pb)]

        def theirs():
            out = torch_layer(*leaves)[0]
            state["t"] = (out.detach(), torch.autograd.grad(out, leaves, dA_eff))

        for _ in range(2):
            ours()
            module()
            theirs()
        torch.cuda.synchronize()
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        dX, dtk, dpk, dpb, dA = state["b"]
        tg = state["t"][1]
        agree = (rel(state["f"][0], state["t"][0]), rel(dX.view(C, N, T, V).permute(1, 0, 2, 3), tg[0]), rel(dA, tg[1]),
                 rel(dtk.reshape(C, -1), tg[2]), rel(dpk.reshape(C, -1), tg[3]), rel(dpb, tg[4]))
        t_ours, t_mod, t_theirs, t_f, t_b = [], [], [], [], []
        for _ in range(runs):
            t_ours.append(timed(ours))
            t_mod.append(timed(module))
            t_theirs.append(timed(theirs))
            t_f.append(timed(fwd))
            t_b.append(timed(bwd))
        # every launch of the layer on its own, on this run's tensors
        lib, st, geo = L.load(), stream_ptr(), dict(B=N, V=V, T_src=T, T_out=T)
        E, P = state["f"][1]
        keep = {}
        ops.adjattn_backward(X, N, T, V, (E, P), tk4, pk4, dA_eff, keep=keep)
        dS, dE = keep["dS"], keep["dE"]
        W, bias = torch.cat([tk, pk], dim=1), torch.cat([torch.zeros_like(pb), pb])
        new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)
        S, P2, A2, dS2, dA2, dE2, E2 = new(N, K, V, V), new(N, K, V, V), new(N, K, V, V), new(N, K, V, V), new(K, V, V), new(2 * kce, n), new(2 * kce, n)
        nslab = lib.sar_adjattn_sim_slabs(Ce, T, V)
        slab = new(nslab, N * K * V * V)
        each = {
            "1x1 fwd": lambda: ops.conv1x1_fwd(X, W, bias, geo, out=E2),
            "sim": lambda: check(lib.sar_adjattn_sim_f32(ptr(E), ptr(E[kce:]), n, N, K, Ce, T, V, ptr(S), ptr(slab), nslab, st)),
            "softmax": lambda: check(lib.sar_adjattn_softmax_f32(ptr(S), ptr(A), N, K, V, ptr(P2), ptr(A2), st)),
            "softmax_bwd": lambda: check(lib.sar_adjattn_softmax_bwd_f32(ptr(P), ptr(dA_eff), N, K, V, ptr(dS2), ptr(dA2), st)),
            "dembed": lambda: check(lib.sar_adjattn_dembed_f32(ptr(dS), ptr(E), ptr(E[kce:]), n, N, K, Ce, T, V, ptr(dE2), ptr(dE2[kce:]), n, st)),
            "1x1 wgrad": lambda: ops.conv1x1_wgrad(X, dE, geo),
            "1x1 dgrad": lambda: ops.conv1x1_dgrad(dE, W, geo),
            "to_cn(x)": lambda: to_cn(x),
        }
        for f in each.values():
            f()
        t_each = {k: med([timed(f) for _ in range(runs)]) for k, f in each.items()}
        eb = 2.0 * kce * n * 4
        floor_sim, floor_de = eb / (copy_gbs * 1e9) * 1e3, 2 * eb / (copy_gbs * 1e9) * 1e3
        print("(N, C, T, V) = (%d, %d, %d, %d), Ce = %d: x %.1f MB, theta + phi %.1f MB, contraction length %d in %d slabs"
              % (N, C, T, V, Ce, x.numel() * 4 / 1e6, eb / 1e6, Ce * T, nslab))
        print("  ops       min %8.3f  median %8.3f   (forward median %.3f, backward median %.3f)" % (min(t_ours), med(t_ours), med(t_f), med(t_b)))
        print("  module    min %8.3f  median %8.3f   (to_cn(x), from_cn(dx) at its boundary)" % (min(t_mod), med(t_mod)))
        print("  torch     min %8.3f  median %8.3f" % (min(t_theirs), med(t_theirs)))
        print("  ratio torch / ops (medians): %.2f;  torch / module: %.2f;  ops' median below torch's minimum: %s"
              % (med(t_theirs) / med(t_ours), med(t_theirs) / med(t_mod), med(t_ours) < min(t_theirs)))
        print("  each launch alone (median): " + "  ".join("%s %.3f" % kv for kv in t_each.items()))
        print("  floors at the copy rate: sim %.3f (theta and phi read once), measured / floor %.2f;  dembed %.3f (two reads, two writes), "
              "measured / floor %.2f" % (floor_sim, t_each["sim"] / floor_sim, floor_de, t_each["dembed"] / floor_de))
        print("  ops against the torch layer, max-norm relative: A_eff %.2e  dx %.2e  dA %.2e  dtheta.kernel %.2e  dphi.kernel %.2e  dphi.bias %.2e" % agree)
        print("  kept for backward besides X: %.1f MB" % (sum(t.numel() * 4 for t in state["f"][1]) / 2 ** 20))
        del state, x, X, dA_eff, leaves, each, E, P, dS, dE, dE2, E2, slab, keep, xm, layer
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
