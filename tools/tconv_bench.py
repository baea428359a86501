"""TemporalConv alone (csrc/tconv.hip through sar_amd.ops), forward and backward separately, at the benchmark batch over the shapes
(N, C -> M, T, V; k, d, s) of the temporal units it stands for -- ST-GCN's own 9-tap convolution, a full-width dilated convolution,
MS-TCN branches of a 64- and a 256-channel block, a wide 3-tap dilated convolution, a stride-2 branch -- timed warm and interleaved with
the same layer as torch.nn.functional.conv2d under autograd (F.pad for the uneven SAME padding) on the same GPU, and at (9, 1, 1) with
the in-tree 9-tap kernels (ops.conv_gemm TEMPORAL forward and transposed, ops.conv_wgrad) on the same tensors as CN matrices.

  python tools/tconv_bench.py [--runs 12] [--batch 128]      (output: profiles/tconv.txt)

Reported per shape: median and minimum of each of the three kernels (the data gradient with its kernel transpose, the weight gradient
with its slab sum, as ops issues them), of torch's forward and backward, and of the 9-tap kernels; per kernel two floors and the ratio
of the median to each -- the time of its algorithmic bytes (both activations once, the kernel once) at this box's copy rate, and the
time of its FLOPs at this box's fp32 MFMA rate (sar_amd/box.py, both measured in this process)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "skeleton-action-recognition_amd"))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

SHAPES = [
    ((64, 64, 300, 25), (9, 1, 1), "ST-GCN's own temporal convolution"),
    ((64, 64, 300, 25), (5, 2, 1), "a full-width dilated convolution"),
    ((16, 16, 300, 25), (5, 2, 1), "an MS-TCN branch of a 64-channel block"),
    ((64, 64, 75, 25), (5, 2, 1), "an MS-TCN branch of a 256-channel block"),
    ((256, 256, 75, 25), (3, 3, 1), "a wide 3-tap dilated convolution"),
    ((32, 32, 300, 25), (5, 2, 2), "a stride-2 branch"),
]


def main():
    from models.gcn import to_cn
    from sar_amd import _lib as L
    from sar_amd import box, ops
    argv = sys.argv[1:]
    opt = lambda name, default: int(argv[argv.index(name) + 1]) if name in argv else default
    runs, N = opt("--runs", 12), opt("--batch", 128)
    dev = torch.device("cuda:0")
    print("device: %s" % torch.cuda.get_device_name(dev))
    copy_gbs = box.copy(dev)
    mfma_tf, ghz = box.mfma("f32", dev)
    print("this box: copy rate (float4 copy of 1 GiB, read + write) %.0f GB/s; v_mfma_f32_32x32x2_f32 dense loop %.1f TFLOP/s at %.2f GHz"
          % (copy_gbs, mfma_tf, ghz))
    print("TemporalConv, fp32, batch %d, %d warm runs each, interleaved (ms, median / min); torch = F.conv2d under autograd on the same "
          "tensors; floors: algorithmic bytes at the copy rate, FLOPs at the fp32 MFMA rate" % (N, runs))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    med = lambda v: sorted(v)[len(v) // 2]
    rel = lambda a, b: ((a - b).abs().max() / b.abs().max()).item()
    for (C, M, T, V), (k, d, s), what in SHAPES:
        T_out, pad = ops.tconv_geometry(T, k, s, d, "same")
        behind = max((T_out - 1) * s + (k - 1) * d + 1 - T - pad, 0)
        g = torch.Generator(device=dev).manual_seed(0)
        r = lambda *shape: torch.randn(shape, generator=g, device=dev)
        x, dout, W, b = r(N, C, T, V), r(N, M, T_out, V), r(k, 1, C, M) / (k * C) ** 0.5, 0.5 * r(M)
        state = {}
        ours = {
            "fwd": lambda: state.__setitem__("out", ops.tconv_forward(x, W, b, s, d, pad, T_out)),
            "bwd_data": lambda: state.__setitem__("dx", ops.tconv_backward_data(dout, W, T, s, d, pad)),
            "wgrad": lambda: state.__setitem__("dW", ops.tconv_wgrad(x, dout, k, s, d, pad)),
        }
        xt, Wt, bt = (t.clone().requires_grad_() for t in (x, W[:, 0].permute(2, 1, 0).unsqueeze(-1).contiguous(), b))

        def torch_fwd():
            state["t_out"] = F.conv2d(F.pad(xt, (0, 0, pad, behind)), Wt, bt, stride=(s, 1), dilation=(d, 1))

        def torch_bwd():
            state["t_grads"] = torch.autograd.grad(state["t_out"], (xt, Wt, bt), dout, retain_graph=True)

        theirs = {"torch fwd": torch_fwd, "torch bwd (dx, dW, dbias)": torch_bwd}
        nine = {}
        if (k, d) == (9, 1):
            X, D = to_cn(x), to_cn(dout)
            geo = dict(B=N, V=V, T_src=T, T_out=T_out, Kc=C, M=M, taps=9, stride=s, pad=pad)
            o9, dx9, WT9 = torch.empty((M, N * T_out * V), device=dev), torch.empty((C, N * T * V), device=dev), torch.empty((9, M, C), device=dev)
            flat9 = torch.empty(9 * C * M + M, device=dev)

            def nine_dgrad():
                ops.transpose(W, WT9, 9, C, M)
                ops.conv_gemm(L.SAR_CONV_TEMPORAL, D, dx9, WT9, M * C, C, B=N, V=V, T_src=T_out, T_out=T, Kc=M, M=C, taps=9, stride=s, pad=pad,
                              transposed=True, split=None)
            nine = {
                "9-tap fwd": lambda: ops.conv_gemm(L.SAR_CONV_TEMPORAL, X, o9, W, C * M, M, bias=b, split=None, **geo),
                "9-tap bwd_data": nine_dgrad,
                "9-tap wgrad": lambda: ops.conv_wgrad(L.SAR_CONV_TEMPORAL, X, D, flat9, w_stride_tap=C * M, w_stride_c=M, wsize=9 * C * M, bsize=M,
                                                     split=None, **geo),
            }
        every = dict(ours, **theirs, **nine)
        for _ in range(2):
            for f in every.values():
                f()
        torch.cuda.synchronize()
        tg = state["t_grads"]
        agree = (rel(state["out"], state["t_out"].detach()), rel(state["dx"], tg[0]), rel(state["dW"][0][:, 0], tg[1][..., 0].permute(2, 1, 0)),
                 rel(state["dW"][1], tg[2]))
        times = {name: [] for name in every}
        for _ in range(runs):
            for name, f in every.items():
                times[name].append(timed(f))
        flops = 2.0 * M * C * k * N * T_out * V
        nbytes = 4.0 * (N * C * T * V + N * M * T_out * V + k * C * M)
        f_bytes, f_flops = nbytes / (copy_gbs * 1e9) * 1e3, flops / (mfma_tf * 1e12) * 1e3
        print("(N, C -> M, T, V; k, d, s) = (%d, %d -> %d, %d, %d; %d, %d, %d): %s.  T_out %d, pad (%d, %d), %.2f GFLOP, %.1f MB; floors: bytes "
              "%.3f, FLOPs %.3f; wgrad in %d slabs" % (N, C, M, T, V, k, d, s, what, T_out, pad, behind, flops / 1e9, nbytes / 1e6, f_bytes, f_flops,
                                                       L.load().sar_tconv_wgrad_slabs(N, C, M, T_out, V)))
        for name in ours:
            t = med(times[name])
            print("  %-28s %8.3f / %8.3f    x bytes floor %6.2f   x FLOP floor %6.2f" % (name, t, min(times[name]), t / f_bytes, t / f_flops))
        for name in list(theirs) + list(nine):
            print("  %-28s %8.3f / %8.3f" % (name, med(times[name]), min(times[name])))
        m = lambda name: med(times[name])
        print("  ratio torch / ours (medians): fwd %.2f, bwd %.2f" % (m("torch fwd") / m("fwd"), m("torch bwd (dx, dW, dbias)") / (m("bwd_data") + m("wgrad"))))
        if nine:
            print("  ratio ours / 9-tap (medians): fwd %.2f, bwd_data %.2f, wgrad %.2f"
                  % (m("fwd") / m("9-tap fwd"), m("bwd_data") / m("9-tap bwd_data"), m("wgrad") / m("9-tap wgrad")))
        print("  ours against torch, max-norm relative: out %.2e  dx %.2e  dkernel %.2e  dbias %.2e" % agree)
        del state, x, dout, xt, every, ours, theirs, nine
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
