"""Writes tests/golden/engine_layouts.json: what the constructor of every engine of the ST-GCN family lays out on device="cpu"
(parameter table, flat buffer, gradient buckets, BatchNorm states, operand-image keys, the initial parameters' digest).  Run at the
commit whose layout is the reference -- the fixture pins it for every later restructuring of the constructors, so it is never
regenerated from the code under test (tests/test_engine_layout.py imports CONFIGS and layout() from here)."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "skeleton-action-recognition_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

MFMA = ("fp32", "bf16", "bf16_operands", "f32_split", "f32_split_bf16x6")


def configs():
    """name -> (engine class, keyword arguments); every engine is built with device="cpu", num_classes=7, seed=0"""
    from sar_amd.bone import NTU_BONE_PAIRS
    from sar_amd.stgcn import STGCN
    from sar_amd.stgcn_ta import STGCNTA
    from sar_amd.stgin import STGIN
    from sar_amd.stpgcn import STPGCN
    out = {"stgcn-" + m: (STGCN, dict(mfma=m)) for m in MFMA}
    out["stgcn-trainable_adjacency"] = (STGCN, dict(trainable_adjacency=True))
    out["stgcn-bone_motion"] = (STGCN, dict(bone_pairs=NTU_BONE_PAIRS, motion=True))
    out["stgcn-two_blocks"] = (STGCN, dict(blocks=[(64, 1, False), (64, 1, True)]))
    out["stgin"] = (STGIN, {})
    out["stpgcn"] = (STPGCN, {})
    out["stgcn_ta"] = (STGCNTA, dict(frames=12, blocks=[(64, 1, False), (64, 2, True)]))
    return out


def layout(eng):
    keys = lambda pk: sorted(pk.index) if pk is not None else None
    return {
        "params": [[k, list(eng.shapes[k]), eng.offsets[k]] for k in eng.shapes],
        "kinds": list(eng.kinds),
        "buckets": [list(b) for b in eng._buckets],
        "flat_numel": eng.flat.numel(),
        "bn": sorted(eng.bn),
        "packed": keys(eng.packed),
        "spacked": keys(eng.spacked),
        "wT_off": dict(eng._wT_off),
        "flat_sha256": hashlib.sha256(eng.flat.detach().cpu().numpy().tobytes()).hexdigest(),
        "none": {k: getattr(eng, k) is None for k in ("_slabs", "_aux", "_wT_perm")},
    }


def build(name):
    cls, kw = configs()[name]
    return cls(device="cpu", num_classes=7, seed=0, **kw)


if __name__ == "__main__":
    out = {name: layout(build(name)) for name in configs()}
    with open(os.path.join(HERE, "engine_layouts.json"), "w") as fh:
        fh.write("{\n" + ",\n".join("%s: %s" % (json.dumps(k), json.dumps(v, sort_keys=True)) for k, v in out.items()) + "\n}\n")
    print("wrote %d engine layouts" % len(out))
