"""TemporalAttention alone (csrc/tattn.hip through sar_amd.ops), forward + backward, at the two benchmark activations --
(N, C, T, V) = (128, 64, 300, 25) with num_hidden = [64] and (128, 256, 75, 25) with [128, 64] -- timed warm and interleaved with
the same layer written in torch ops under autograd (the reference's call: transpose, reshape, linear, multiply) on the same GPU.

  python tools/tattn_bench.py [--runs 12] [--batch 128]      (output: profiles/tattn.txt)

Reported: min and median of the runs, the forward / backward split, each of the five kernels on its own, the ratio to the torch-ops
layer, and the ratio to the floor implied by bytes and FLOP at this box's copy rate and fp32 MFMA rate (sar_amd/box.py, measured in
this process): forward 3 passes over x (score read, scale read + write) and one first-layer product, backward 5 passes (dscore reads
x and dout, wgrad reads x, dx reads dout and writes dx) and two products."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402


def torch_layer(x, params):
    """models/stgcn.py:75-85 in torch ops"""
    N, C, T, V = x.shape
    xt = x.permute(0, 2, 3, 1)
    h = xt.reshape(-1, T, V * C)
    nl = len(params) // 2
    for i in range(nl):
        h = torch.nn.functional.linear(h, params[2 * i].t(), params[2 * i + 1])
        h = torch.sigmoid(h) if i == nl - 1 else torch.relu(h)
    return (xt * h.reshape(N, T, 1, 1)).permute(0, 3, 1, 2)


def main():
    from sar_amd import _lib as L
    from sar_amd import box, ops
    from sar_amd._lib import check, ptr, stream_ptr
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    runs, N = opt("--runs", 12), opt("--batch", 128)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    copy_gbs = box.copy(dev)
    mfma_tf, ghz = box.mfma("f32", dev)
    print("this box: copy rate (float4 copy of 1 GiB, read + write) %.0f GB/s; v_mfma_f32_32x32x2_f32 %.1f TFLOP/s at %.2f GHz" % (copy_gbs, mfma_tf, ghz))
    print("TemporalAttention forward + backward (x requires a gradient), fp32, %d warm runs each, interleaved (ms); torch = the layer in "
          "torch ops under autograd, the same batch" % runs)

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    med = lambda v: sorted(v)[len(v) // 2]
    for (C, T, V), hidden in (((64, 300, 25), [64]), ((256, 75, 25), [128, 64])):
        g = torch.Generator(device=dev).manual_seed(0)
        x = torch.randn(N, C, T, V, generator=g, device=dev)
        dout = torch.randn(N, C, T, V, generator=g, device=dev)
        params, fan_in = [], V * C
        for units in hidden + [1]:
            lim = (6.0 / (fan_in + units)) ** 0.5
            params += [(torch.rand(fan_in, units, generator=g, device=dev) * 2 - 1) * lim, 0.1 * torch.randn(units, generator=g, device=dev)]
            fan_in = units
        state = {}

        def fwd():
            state["f"] = ops.tattn_forward(x, params)

        def bwd():
            state["b"] = ops.tattn_backward(x, state["f"][1], params, dout)

        def ours():
            fwd()
            bwd()

        leaves = [x.clone().requires_grad_()] + [p.clone().requires_grad_() for p in params]

        def theirs():
            out = torch_layer(leaves[0], leaves[1:])
            state["t"] = (out.detach(), torch.autograd.grad(out, leaves, dout))

        for _ in range(2):
            ours()
            theirs()
        torch.cuda.synchronize()
        rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
        agree = (rel(state["f"][0], state["t"][0]), rel(state["b"][0], state["t"][1][0]), rel(state["b"][1][0], state["t"][1][1]))
        # a hidden pre-activation within rounding of zero lands on either side of the ReLU in two float32 computations: such a frame's
        # dx differs as a whole, every other frame agrees to rounding
        ddx = (state["b"][0] - state["t"][1][0]).abs().amax(dim=(1, 3)) / state["t"][1][0].abs().max()
        flipped = int((ddx > 1e-4).sum())
        rest = float(ddx[ddx <= 1e-4].max())
        t_ours, t_theirs, t_f, t_b = [], [], [], []
        for _ in range(runs):
            t_ours.append(timed(ours))
            t_theirs.append(timed(theirs))
            t_f.append(timed(fwd))
            t_b.append(timed(bwd))
        # the five kernels on their own, on this run's tensors
        lib, st, n, u = L.load(), stream_ptr(), N * T, hidden[0]
        sn, sc = C * T * V, T * V
        a, h1 = state["f"][1][0], state["f"][1][1]
        keep = {}
        ops.tattn_backward(x, state["f"][1], params, dout, keep=keep)
        dz1, out, dx, dzL = keep["dz_1"], torch.empty_like(x), torch.empty_like(x), torch.empty(n, device=dev)
        nslab, size = lib.sar_tattn_wgrad_slabs(N, C, T, V), V * C * u + u
        slab = torch.empty(nslab, size, device=dev)
        each = {
            "score": lambda: check(lib.sar_tattn_score_f32(ptr(x), sn, sc, ptr(params[0]), ptr(params[1]), N, C, T, V, u, 0, ptr(h1), n, st)),
            "scale": lambda: check(lib.sar_tattn_scale_f32(ptr(x), sn, sc, ptr(a), N, C, T, V, ptr(out), sn, sc, st)),
            "dscore": lambda: check(lib.sar_tattn_dscore_f32(ptr(x), sn, sc, ptr(dout), sn, sc, ptr(a), N, C, T, V, ptr(dzL), st)),
            "wgrad": lambda: check(lib.sar_tattn_wgrad_f32(ptr(x), sn, sc, ptr(dz1), n, N, C, T, V, u, ptr(slab), nslab, st)),
            "dx": lambda: check(lib.sar_tattn_dx_f32(ptr(dout), sn, sc, ptr(a), ptr(params[0]), ptr(dz1), n, N, C, T, V, u, ptr(dx), sn, sc, st)),
        }
        t_each = {k: med([timed(f) for _ in range(runs)]) for k, f in each.items()}
        xb, gf = x.numel() * 4.0, 2.0 * n * V * C * u
        floor_f = 3 * xb / (copy_gbs * 1e9) * 1e3 + gf / (mfma_tf * 1e12) * 1e3
        floor_b = 5 * xb / (copy_gbs * 1e9) * 1e3 + 2 * gf / (mfma_tf * 1e12) * 1e3
        print("(N, C, T, V) = (%d, %d, %d, %d), num_hidden = %s: x %.1f MB, first-layer product %.2f GFLOP per pass" % (N, C, T, V, hidden, xb / 1e6, gf / 1e9))
        print("  kernels   min %8.3f  median %8.3f   (forward median %.3f, backward median %.3f)" % (min(t_ours), med(t_ours), med(t_f), med(t_b)))
        print("  torch     min %8.3f  median %8.3f" % (min(t_theirs), med(t_theirs)))
        print("  ratio torch / kernels (medians): %.2f;  kernels' median below torch's minimum: %s" % (med(t_theirs) / med(t_ours), med(t_ours) < min(t_theirs)))
        print("  each kernel alone (median): " + "  ".join("%s %.3f" % kv for kv in t_each.items()))
        print("  floor (bytes at the copy rate + FLOP at the fp32 MFMA rate): forward %.3f (3 passes + 1 product), backward %.3f (5 passes + 2 "
              "products); measured / floor: forward %.2f, backward %.2f" % (floor_f, floor_b, med(t_f) / floor_f, med(t_b) / floor_b))
        print("  kernels against the torch layer, max-norm relative: out %.2e  dx %.2e  dkernel_1 %.2e;  frames whose dx differs by more than "
              "1e-4 (a ReLU taken on the other side): %d of %d, the other frames within %.2e" % (agree + (flipped, n, rest)))
        print("  kept for backward besides x: %.1f MB" % (sum(t.numel() * 4 for t in state["f"][1]) / 2 ** 20))
        del state, x, dout, leaves, each, out, dx, slab, keep
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
