"""Writes tests/golden/resnet_layouts.json: what the constructor of Path B's classifier (sar_amd/resnet.py) lays out on device="cpu"
(parameter table, flat buffer, gradient buckets, BatchNorm states, the data-gradient re-layout, the initial parameters' digest, which
streams / images exist).  Run at the commit whose layout is the reference -- the fixture pins it for every later restructuring of the
constructor, so it is never regenerated from the code under test (tests/test_resnet_layout.py imports configs() and layout() from
here).  The reference commit's constructor entered torch.cuda.device() whatever the device: build() replaces it by a null context
while it constructs (harmless where the constructor no longer does).  One recorded value was changed by hand since: a CPU engine in a
split arithmetic now builds its term images and its plan like a device one (sar_amd/split_plan.py ResNetPlan; the schedule of
tests/test_pathb_schedule.py is replayed on it), so "spacked" is None of the two fp32 configurations only."""
import contextlib
import hashlib
import json
import os
import sys
from unittest import mock

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def configs():
    """name -> keyword arguments; every engine is built with device="cpu", num_classes=7, seed=0"""
    return {"resnet-nf%d-%s" % (nf, m): dict(num_filters=nf, mfma=m) for nf in (8, 64) for m in ("fp32", "f32_split")}


def layout(eng):
    # a bucket is (block index, lo, hi); the reference commit held dict(stage, lo, hi)
    buckets = [[b["lo"], b["hi"]] if isinstance(b, dict) else [b[1], b[2]] for b in eng._buckets]
    return {
        "params": [[k, list(eng.shapes[k]), eng.offsets[k]] for k in eng.shapes],
        "flat_numel": eng.flat.numel(),
        "buckets": buckets,
        "bn": list(eng.bn),
        "woff": {k: list(v) for k, v in eng._woff.items()},
        "perm_bwd": [list(it) for it in eng._perm_bwd.items],
        "flat_sha256": hashlib.sha256(eng.flat.detach().cpu().numpy().tobytes()).hexdigest(),
        "none": {k: getattr(eng, k) is None for k in ("_side", "_aux", "_slabs", "_ctx", "spacked")},
    }


def build(name):
    import torch
    from sar_amd.resnet import ResNet18
    with mock.patch.object(torch.cuda, "device", lambda dev: contextlib.nullcontext()):
        return ResNet18(device="cpu", num_classes=7, seed=0, **configs()[name])


if __name__ == "__main__":
    out = {name: layout(build(name)) for name in configs()}
    with open(os.path.join(HERE, "resnet_layouts.json"), "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in out.items()) + "\n}\n")
    print("wrote %d resnet layouts" % len(out))
