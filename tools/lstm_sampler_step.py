"""TemporalSampler (models/lstm_sampler.py) forward + backward at the reference's use: N = 128 sequences (64 clips x 2 bodies), C = 3,
T = 300, V = 25, top_k = 200, for num_hidden = [64] and [128, 64].  Prints, per configuration,
  * the step time (device events around forward + backward, median and spread over interleaved rounds),
  * the same LSTM stack as torch.nn.LSTM on the device (MIOpen), forward + backward, timed in the same process in alternating rounds
    (information, not a pass mark: the stack alone, without pack / top-k / gather),
  * the time of every library call of one step (device events around each sar_amd.ops call, a separate pass: the events serialise
    nothing but add their own overhead, so the sum is an upper bound of the step).
Output committed as profiles/lstm_sampler.txt.  Needs a GPU; there is no fallback.

    python tools/lstm_sampler_step.py [--rounds 7] [--iters 10] [--warmup 5]
"""
import argparse
import collections
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

from models.lstm_sampler import TemporalSampler  # noqa: E402
from sar_amd import ops  # noqa: E402

TIMED_OPS = ("lstm_pack", "conv_gemm", "lstm_fwd", "topk_desc", "frame_gather", "frame_gather_bwd", "lstm_bwd", "conv_wgrad", "transpose",
             "lstm_unpack_add")


def timed(fn, iters):
    """milliseconds per call of fn over `iters` calls between two device events"""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / iters


def per_call_times(step):
    """one step with device events around every sar_amd.ops call the module makes -> [(name, ms)] in call order"""
    log, saved = [], {}

    def wrap(name, fn):
        def inner(*a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            r = fn(*a, **kw)
            e1.record()
            rows = next((t.shape[0] for t in a if torch.is_tensor(t) and t.dim() == 2), None)
            log.append((name if rows is None else "%s [%d rows]" % (name, rows), e0, e1))
            return r
        return inner

    for name in TIMED_OPS:
        saved[name] = getattr(ops, name)
        setattr(ops, name, wrap(name, saved[name]))
    try:
        step()
        torch.cuda.synchronize()
    finally:
        for name, fn in saved.items():
            setattr(ops, name, fn)
    return [(name, e0.elapsed_time(e1)) for name, e0, e1 in log]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--T", type=int, default=300)
    ap.add_argument("--top-k", type=int, default=200)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/lstm_sampler_step.py needs a GPU"
    dev = torch.device("cuda:0")
    N, C, T, V, k = args.N, 3, args.T, 25, args.top_k
    print("device: %s; N %d C %d T %d V %d top_k %d; %d rounds x %d iterations after %d warm-up steps"
          % (torch.cuda.get_device_name(0), N, C, T, V, k, args.rounds, args.iters, args.warmup))
    for num_hidden in ([64], [128, 64]):
        torch.manual_seed(0)
        x = torch.randn(N, C, T, V, device=dev, requires_grad=True)
        dout = torch.randn(N, C, k, V, device=dev)
        m = TemporalSampler(num_hidden, top_k=k)

        def ours():
            x.grad = None
            m.zero_grad(set_to_none=True)
            m(x, True).backward(dout)

        def ours_forward():
            with torch.no_grad():
                m(x, False)

        widths, F = list(num_hidden) + [1], V * C
        stack = torch.nn.ModuleList()
        for u in widths:
            stack.append(torch.nn.LSTM(F, u).to(dev))
            F = u
        xs = torch.randn(T, N, V * C, device=dev, requires_grad=True)
        ds = torch.randn(T, N, 1, device=dev)

        def miopen():
            xs.grad = None
            stack.zero_grad(set_to_none=True)
            h = xs
            for layer in stack:
                h = layer(h)[0]
            h.backward(ds)

        baseline = True
        for _ in range(args.warmup):
            ours(), ours_forward()
        try:
            for _ in range(args.warmup):
                miopen()
        except Exception as e:      # the comparison is information: the module's own numbers are still reported
            baseline = False
            print("torch.nn.LSTM on the device: not measured (%s: %s)" % (type(e).__name__, e))
        torch.cuda.synchronize()
        t_ours, t_fwd, t_base = [], [], []
        for _ in range(args.rounds):
            t_ours.append(timed(ours, args.iters))
            if baseline:
                t_base.append(timed(miopen, args.iters))
            t_fwd.append(timed(ours_forward, args.iters))
        show = lambda t: "%.3f ms (min %.3f, max %.3f)" % (statistics.median(t), min(t), max(t))
        print("\nnum_hidden = %s" % (num_hidden,))
        print("  TemporalSampler forward + backward:          %s" % show(t_ours))
        print("  TemporalSampler forward (no_grad):           %s" % show(t_fwd))
        if baseline:
            print("  torch.nn.LSTM stack forward + backward:      %s   (MIOpen; the stack alone)" % show(t_base))
        calls = per_call_times(ours)
        total = sum(ms for _, ms in calls)
        print("  per library call of one step (ms; sum %.3f):" % total)
        for name, ms in calls:
            print("    %-34s %8.3f" % (name, ms))
        by = collections.OrderedDict()
        for name, ms in calls:
            key = name.split(" ")[0]
            by[key] = by.get(key, 0.0) + ms
        print("  by entry point: " + ", ".join("%s %.3f" % kv for kv in by.items()))
        print("  the stack alone (conv_gemm + lstm_fwd + lstm_bwd + conv_wgrad + transpose): %.3f ms"
              % sum(by.get(n, 0.0) for n in ("conv_gemm", "lstm_fwd", "lstm_bwd", "conv_wgrad", "transpose")))


if __name__ == "__main__":
    main()
