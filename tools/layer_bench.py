"""The layer level measured (output kept as profiles/layers.txt):

  1. the worst error of every case of tests/test_gpu_graph_sample.py, tests/test_gpu_layers.py, tests/test_gpu_gin_sample.py and
     tests/test_gpu_gin_layers.py (the tests print it; this tool runs them and keeps those lines);
  2. the per-sample adjacency contraction (csrc/graph_sample.hip) at the ST-PGCNP head shapes (N, F, V) = (128, 256, 512) and
     (128, 512, 256): time, achieved TFLOP/s, the fraction of the fp32 MFMA rate this box sustains (sar_amd.box.mfma) and the same
     product as torch.bmm on the SAME tensors -- the two interleaved in one process after a warm-up, several launches per timed
     interval, median of the repetitions with their spread;
  3. one SpatioTemporalGraphConv forward + backward at (128, 64, 300, 25), the engine's block forward + backward on the same CN
     tensors (no boundary conversion, no parameter copies), and the two boundary conversions alone;
  4. what the compiler reports for each instance of the kernel (registers, spills, LDS, waves per SIMD): graph_sample.hip compiled
     once more with the Makefile's flags and -Rpass-analysis=kernel-resource-usage, the object thrown away;
  5. the graph isomorphism aggregation (sar_gin_sample_fwd_f32: the contraction with the self term (1 + eps) x in its epilogue) at
     (N, F, V) = (128, 256, 512), (128, 16, 512) and (128, 64, 25) against the composition the code offered before it -- A + diag(1 + eps)
     formed by torch, then sar_graph_sample_fwd_f32 -- and against sar_graph_sample_fwd_f32 alone, on the same tensors, interleaved as
     in 2; and sar_gin_sample_eps_grad_f32 against its HBM floor of 2 F N V 4 bytes.

    python tools/layer_bench.py [--reps 10] [--no-errors] [--no-resources]
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")]

from sar_amd import box, ops  # noqa: E402

SHAPES = [(128, 256, 512), (128, 512, 256)]      # (N, F, V): the two ST-PGCNP heads
GIN_SHAPES = [(128, 256, 512), (128, 16, 512), (128, 64, 25)]      # the head, few channels under a large graph, the skeleton graph


def _ms(fn, inner):
    """milliseconds per call of `inner` back-to-back calls between one pair of events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(inner):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / inner


def _interleaved(fns, reps, inner):
    """median and (min, max) per function, the functions taking turns so that all see the same clocks"""
    for fn in fns:
        _ms(fn, 2)
    t = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t[i].append(_ms(fn, inner))
    return [(sorted(x)[len(x) // 2], min(x), max(x)) for x in t]


def errors():
    print("== worst error per test case (printed by the tests)")
    out = subprocess.run([sys.executable, "-m", "pytest", "-q", "-s", "-m", "gpu", os.path.join(ROOT, "tests", "test_gpu_graph_sample.py"),
                          os.path.join(ROOT, "tests", "test_gpu_layers.py"), os.path.join(ROOT, "tests", "test_gpu_gin_sample.py"),
                          os.path.join(ROOT, "tests", "test_gpu_gin_layers.py")], capture_output=True, text=True, cwd=ROOT).stdout
    for line in out.splitlines():
        line = line.lstrip(".")
        if "e-0" in line or "e-1" in line or " passed" in line or " failed" in line:
            print("  " + line)


def resources():
    print("== compiler's resource usage of csrc/graph_sample.hip (gs_kernel<WI, WJ, TM, TN, BK>: tile 32 WI TM x 32 WJ TN; SELF: the "
          "gin instantiation; eg_*: the eps-gradient reduction)")
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        print("  hipcc not found: not measured")
        return
    csrc = os.path.join(ROOT, "skeleton-action-recognition_amd", "csrc")
    with tempfile.TemporaryDirectory() as tmp:
        err = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize",
                              "-Rpass-analysis=kernel-resource-usage", "-c", os.path.join(csrc, "graph_sample.hip"), "-o",
                              os.path.join(tmp, "graph_sample.o")], capture_output=True, text=True, cwd=csrc).stderr
    keep = ("TotalSGPRs", "VGPRs:", "AGPRs", "ScratchSize", "Occupancy", "VGPRs Spill", "LDS Size")
    for line in err.splitlines():
        m = re.search(r"remark: \s*(.*?) \[-Rpass", line)
        if not m:
            continue
        text = m.group(1)
        if text.startswith("Function Name"):
            t = re.search(r"gs_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])E", text)
            e = re.search(r"(eg_\w+_kernel)(?:ILb([01])E)?", text)
            if t:
                print("  gs_kernel<%s>%s" % (", ".join(t.groups()[:5]), "  SELF (gin)" if t.group(6) == "1" else ""))
            elif e:
                print("  %s%s" % (e.group(1), {None: "", "1": "<16 B per lane>", "0": "<element loads>"}[e.group(2)]))
            else:
                print("  " + text)
        elif any(k in text for k in keep):
            print("      " + text)


def kernels(dev, reps):
    peak, ghz = box.mfma("f32", dev)
    print("== csrc/graph_sample.hip against torch.bmm; fp32 MFMA rate of this box (sar_box_mfma): %.1f TFLOP/s at %.2f GHz" % (peak, ghz))
    print("%-16s %-9s %8s %8s %7s %17s %8s %8s %17s" % ("(N, F, V)", "kernel", "ms", "TFLOP/s", "of box", "ms min-max", "bmm ms", "bmm TF",
                                                        "bmm ms min-max"))
    g = torch.Generator().manual_seed(0)
    for N, F, V in SHAPES:
        y, A, d = (torch.randn(s, generator=g).to(dev) for s in ((N, F, V), (N, V, V), (N, F, V)))
        cn = lambda t: t.permute(1, 0, 2).reshape(F, N * V).contiguous()
        yc, dc = cn(y), cn(d)
        out, dA = torch.empty_like(yc), torch.empty_like(A)
        o3, a3 = torch.empty_like(y), torch.empty_like(A)
        yT, AT = y.transpose(1, 2), A.transpose(1, 2)
        legs = [("fwd", lambda: ops.graph_sample_fwd(yc, A, out, F, V, N), lambda: torch.bmm(y, A, out=o3)),
                ("bwd_data", lambda: ops.graph_sample_bwd_data(dc, A, out, F, V, N), lambda: torch.bmm(d, AT, out=o3)),
                ("dadj", lambda: ops.graph_sample_dA(yc, dc, dA, F, V, N), lambda: torch.bmm(yT, d, out=a3))]
        flops = 2.0 * N * F * V * V
        for name, ours, theirs in legs:
            (mo, lo, ho), (mb, lb, hb) = _interleaved([ours, theirs], reps, 5)
            print("%-16s %-9s %8.3f %8.1f %6.1f%% %8.3f-%-8.3f %8.3f %8.1f %8.3f-%-8.3f" % (
                (N, F, V), name, mo, flops / mo / 1e9, 100.0 * flops / mo / 1e9 / peak, lo, ho, mb, flops / mb / 1e9, lb, hb))


def gin(dev, reps):
    print("== sar_gin_sample_fwd_f32 (self term in the epilogue) against torch's A + diag(1 + eps) then sar_graph_sample_fwd_f32, and "
          "against sar_graph_sample_fwd_f32 alone; ms median (min-max)")
    print("%-16s %-26s %-26s %-26s %-34s" % ("(N, F, V)", "fused", "A + diag by torch, then plain", "plain contraction alone",
                                              "eps_grad (GB/s of 2 F N V 4 bytes)"))
    g = torch.Generator().manual_seed(1)
    for N, F, V in GIN_SHAPES:
        x, A, d = (torch.randn(s, generator=g).to(dev) for s in ((N, F, V), (N, V, V), (N, F, V)))
        cn = lambda t: t.permute(1, 0, 2).reshape(F, N * V).contiguous()
        xc, dc = cn(x), cn(d)
        out = torch.empty_like(xc)
        eps = torch.tensor(0.3, device=dev)
        deps = torch.empty((), device=dev)
        eye = torch.eye(V, device=dev)
        scratch = torch.empty(4 * 8192, device=dev)

        def composed():
            ops.graph_sample_fwd(xc, A + (1 + eps) * eye, out, F, V, N)
        legs = [lambda: ops.gin_sample_fwd(xc, A, eps, out, F, V, N), composed, lambda: ops.graph_sample_fwd(xc, A, out, F, V, N),
                lambda: ops.gin_sample_eps_grad(xc, dc, deps, F, V, N, scratch=scratch)]
        res = _interleaved(legs, reps, 5)
        cells = ["%.3f (%.3f-%.3f)" % r for r in res]
        cells[3] += "  %.0f GB/s" % (2.0 * F * N * V * 4 / res[3][0] / 1e6)
        print("%-16s %-26s %-26s %-26s %-34s" % ((str((N, F, V)),) + tuple(cells)))


def block(dev, reps):
    from graph.ntu_rgb_d import Graph
    from models.gcn import from_cn, to_cn
    from models.stgcn import SpatioTemporalGraphConv
    B, C, T, V = 128, 64, 300, 25
    print("== SpatioTemporalGraphConv(64) forward + backward at (B, C, T, V) = (%d, %d, %d, %d)" % (B, C, T, V))
    A = torch.from_numpy(Graph().A).float().to(dev)
    x = torch.randn(B, C, T, V, device=dev).requires_grad_(True)
    dout = torch.randn(B, C, T, V, device=dev)
    layer = SpatioTemporalGraphConv(64)
    layer(x, A, True)
    eng = layer._engines[False]
    X, dY = to_cn(x.detach()), to_cn(dout)

    def as_layer():
        y, _ = layer(x, A, True)
        torch.autograd.grad(y, [x] + list(layer.parameters()), dout)

    def as_engine():
        _, _, sb = eng.block_forward(0, X, B, T, True)
        eng.block_backward(0, sb, dY.clone(), B)

    def conversions():          # what one layer call adds at its boundary: x and dout in, y and dx out
        to_cn(dout), to_cn(dout), from_cn(X, (B, C, T, V)), from_cn(X, (B, C, T, V))

    res = _interleaved([as_layer, as_engine, conversions], reps, 2)
    for name, (m, lo, hi) in zip(("layer (one autograd node)", "engine block, CN in and out", "four boundary conversions"), res):
        print("  %-30s %8.3f ms   (%.3f-%.3f)" % (name, m, lo, hi))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--no-errors", action="store_true")
    ap.add_argument("--no-resources", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    kernels(dev, args.reps)
    block(dev, args.reps)
    gin(dev, args.reps)
    if not args.no_errors:
        errors()
    if not args.no_resources:
        resources()


if __name__ == "__main__":
    main()
