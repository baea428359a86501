"""Writes tests/golden/pathb_schedule.json: the launch schedule of one train step of Path B's classifier (sar_amd/resnet.py), with the
launch wrappers of sar_amd.ops replaced by recorders -- in issue order, every launch of the step; for a conv2d_gemm / conv2d_wgrad its
geometry, the split arithmetic it is ASKED to take (and, for conv2d_gemm, the one left after the wrapper's own demotion rule,
ops.conv2d_split_applicable; a weight gradient's demotion needs the library), the term image, weight bound and bound cells it is handed;
every pass that raises a cell (a Samuelson bound with its BatchNorm and sample count); every fork onto the third stream and every join.
ResNet18(num_classes=7, num_filters=16) on the clips CLIPS (admitted and demoted launches of every family, the compact stride-2 skip
gradient), for both split arithmetics times every subset of the kinds of SAR_SPLIT_KINDS_PATHB and for fp32, without streams
(eng._aux = eng._side = None); with all kinds on also forked as constructed, with need_dx.  Nothing is named by address: cells by order
of first appearance, images and weight bounds by their key, so a trace does not depend on the device it was recorded on.

The fixture was written ONCE, on an MI355X, at commit 27ae1eb ("ST-GCN split engines: per-block arithmetic plan built at
construction"), the parent of the change that moved this engine's per-launch decisions into sar_amd/split_plan.py: at that commit a CPU
engine built no term images.  The run allocates device memory and launches none of the project's kernels.  It is never regenerated from
the code under test (tests/test_pathb_schedule.py imports trace() from here and replays on the CPU what needs no streams).  Uses the
public wrappers of sar_amd.ops, resnet._SPLIT_KINDS, the engine's `spacked` / `p`, and its _fork / _join / _aux / _side."""
import itertools
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import make_golden_split_schedule as S  # noqa: E402  (puts the repository on sys.path)

import torch  # noqa: E402

KINDS = ("fwd", "dgrad", "wgrad")
SPLIT_MODES = S.SPLIT_MODES
CLIPS = ((2, 1, 64, 64), (1, 1, 96, 128))
# wrappers a step calls that launch one kernel and return nothing
_SILENT = ("bn_finalize", "bn_bwd_finalize", "bn_relu_maxpool_fwd", "pool_fwd", "fc_fwd", "fc_bwd", "pool_bwd", "transpose",
           "conv2d_stem_dgrad")
_GEO = ("B", "Kc", "M", "H_src", "W_src", "H_out", "W_out", "KH", "stride")


def subsets():
    for n in range(len(KINDS) + 1):
        yield from itertools.combinations(KINDS, n)


def configs():
    """(arithmetic, kinds or None = as the module has them, forked): 17 without streams, 2 forked"""
    out = [(m, ks, False) for m in SPLIT_MODES for ks in subsets()] + [("fp32", None, False)]
    return out + [(m, KINDS, True) for m in SPLIT_MODES]


def key(mode, kinds, forked, clip):
    return "%s|%s|%s|%s" % (mode, "default" if kinds is None else ",".join(kinds), "forked" if forked else "serial",
                            "x".join(map(str, clip)))


FULL_TRACES = tuple(key(m, KINDS, False, c) for m in SPLIT_MODES for c in CLIPS)


class Recorder(S.Recorder):
    """the ST-GCN recorder's cell names, raises and installation, with the launch wrappers of the 2-d convolutions"""

    def __init__(self, ops, L, eng):
        self.ops, self.L, self.eng, self.trace, self._names, self._saved = ops, L, eng, [], {}, {}
        pk = eng.spacked
        keys = list(pk.index) if pk is not None else []
        self._images = {pk.image(k).data_ptr(): "%s:%s" % k for k in keys}
        self._w_bounds = {pk.bound(k).data_ptr(): "w:%s:%s" % k for k in keys}
        self._gammas = {eng.p[n + ".weight"].data_ptr(): n for n, _ in eng.bn_names}

    def launch(self, op, **what):
        self.trace.append(dict(op=op, **what))

    def bn_bound(self, gamma, beta, count, cell):
        if cell is not None:
            self.trace.append({"raise": "bn_bound", "cell": self.cell(cell), "bn": self._gammas.get(gamma.data_ptr(), "?"), "count": count})

    def bn_add_relu_fwd(self, *a, **k):
        self.launch("bn_add_relu_fwd")
        super().bn_add_relu_fwd(*a, **k)

    def bn_add_relu_bwd_apply(self, *a, **k):
        self.launch("bn_add_relu_bwd_apply")
        super().bn_add_relu_bwd_apply(*a, **k)

    def affine2(self, *a, **k):
        self.launch("affine2")
        super().affine2(*a, **k)

    def bn_add_relu_bwd_reduce(self, dy, y, u, r, mu=None, mr=None, tail=None, mask=None):
        self.launch("bn_add_relu_bwd_reduce", tail=tail is not None)
        return super().bn_add_relu_bwd_reduce(dy, y, u, r, mu, mr, tail, mask)

    def bn_relu_maxpool_bwd(self, x, scale, shift, mean, dy, dz, B, H, W):
        self.launch("bn_relu_maxpool_bwd")
        return torch.empty((x.shape[0], 1, 2)), 1

    def conv2d_gemm(self, src, out, W, w_stride_tap, w_stride_c, *, epi=None, aux=None, aux_affine=None, aux_mean=None,
                    aux_even_pixels=False, ctx=None, split="default", packed=None, bounds=None, kslab=None, **geo):
        ops, L = self.ops, self.L
        epi = L.SAR_EPI_NONE if epi is None else epi
        if split == "default":
            split = ops.DEFAULT_SPLIT
        # the wrapper's own demotion rule
        runs = split if (split in ("f16x3a", "bf16x6") and ops.conv2d_split_applicable(aux_even_pixels=aux_even_pixels, epi=epi, **geo)) else None
        rec = dict(transposed=bool(geo.get("transposed")), epi=epi, pro=geo.get("pro") is not None, even=bool(aux_even_pixels),
                   asked=split, split=runs, packed=None if packed is None else self._images.get(packed.data_ptr(), "?"),
                   **{k: geo[k] for k in _GEO})
        if split and split.startswith("f16"):      # (source cell, the weight's bound by the key of its image)
            rec["bounds"] = [self.cell(bounds[0]), self._w_bounds.get(bounds[1].data_ptr(), "?")] if bounds is not None else None
        self.launch("conv2d_gemm", **rec)
        return (torch.empty((geo["M"], 1, 2)), 1) if epi in (L.SAR_EPI_STATS, L.SAR_EPI_MASK) else None

    def conv2d_wgrad(self, src, dout, dW_tcm, *, split="default", bounds=None, slabs=None, **geo):
        if split == "default":
            split = self.ops.DEFAULT_SPLIT
        rec = dict(transposed=False, epi=None, pro=geo.get("pro") is not None, asked=split, **{k: geo[k] for k in _GEO})
        if split and split.startswith("f16"):      # (source cell, output-gradient cell)
            rec["bounds"] = [self.cell(c) for c in bounds] if bounds is not None else None
        self.launch("conv2d_wgrad", **rec)

    # ---- installation
    def __enter__(self):
        ops, eng = self.ops, self.eng
        put = {n: (lambda *a, _n=n, **k: self.launch(_n)) for n in _SILENT}
        put["make_bn_tail"] = lambda *a, **k: "tail"
        put.update({n: getattr(self, n) for n in ("bn_bound", "bn_add_relu_fwd", "bn_add_relu_bwd_apply", "affine2", "bn_add_relu_bwd_reduce",
                                                  "bn_relu_maxpool_bwd", "conv2d_gemm", "conv2d_wgrad")})
        for n, fn in put.items():
            self._saved[(ops, n)] = getattr(ops, n)
            setattr(ops, n, fn)
        for cls, n in ((ops.PackedSplitWeights, "refresh"), (ops.PermuteBatch, "run")):
            self._saved[(cls, n)] = cls.__dict__[n]
            setattr(cls, n, lambda self_, *a, _n="%s.%s" % (cls.__name__, n), **k: self.launch(_n))
        # what runs between a "fork" and its "forked" is issued on the third stream (in place on an engine without one)
        fork, join = eng._fork, eng._join

        def _fork(fn, *tensors, after="main"):
            self.trace.append({"fork": after if isinstance(after, str) else "event"})
            fork(fn, *tensors, after=after)
            self.trace.append({"forked": True})

        def _join():
            self.trace.append({"join": True})
            join()
        eng._fork, eng._join = _fork, _join
        return self

    def __exit__(self, *exc):
        del self.eng._fork, self.eng._join
        return super().__exit__(*exc)


def traces(mode, kinds=None, forked=False, device="cpu"):
    """the schedules of forward(training=True) + backward() on each of CLIPS, of one engine in arithmetic `mode`; kinds: the value of
    resnet._SPLIT_KINDS the engine is built and run under (None: as the module has it); forked: the engine's streams as constructed
    (and need_dx), else none"""
    from sar_amd import _lib as L
    from sar_amd import ops, resnet
    old, out = resnet._SPLIT_KINDS, []
    if kinds is not None:
        resnet._SPLIT_KINDS = set(kinds)
    try:
        eng = resnet.ResNet18(num_classes=7, num_filters=16, device=device, mfma=mode)
        if not forked:
            eng._aux = eng._side = None
        for clip in CLIPS:
            x = torch.zeros(clip, device=device)
            with Recorder(ops, L, eng) as rec:
                logits = eng.forward(x if x.is_cuda else x.as_subclass(S._Clip), training=True)
                eng.backward(torch.zeros_like(logits), need_dx=forked)
            out.append(rec.trace)
    finally:
        resnet._SPLIT_KINDS = old
    return out


if __name__ == "__main__":
    device = sys.argv[1] if len(sys.argv) > 1 else "cuda"
    digests, full = {}, {}
    for mode, ks, forked in configs():
        for clip, tr in zip(CLIPS, traces(mode, ks, forked, device)):
            assert not S.unraised_reads(tr)[0], (mode, ks, forked, clip, S.unraised_reads(tr)[0])
            digests[key(mode, ks, forked, clip)] = S.digest(tr)
            if key(mode, ks, forked, clip) in FULL_TRACES:
                full[key(mode, ks, forked, clip)] = tr
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(HERE, "pathb_schedule.json")
    with open(out, "w") as fh:
        fh.write('{"digests": {\n' + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v)) for k, v in digests.items()) + '\n},\n'
                 + '"traces": {\n' + ",\n".join("%s: [\n  %s\n]" % (json.dumps(k), ",\n  ".join(json.dumps(e, sort_keys=True) for e in v))
                                               for k, v in full.items()) + "\n}}\n")
    print("wrote %d digests, %d full traces" % (len(digests), len(full)))
