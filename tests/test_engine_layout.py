"""The constructors of the ST-GCN engine family lay out what tests/golden/engine_layouts.json recorded (written once by
tests/golden/make_golden_engine_layouts.py, before the constructors were unified): parameter names, shapes and offsets in order,
residual kinds, gradient buckets, flat size, BatchNorm states, which operand images exist, the batched re-layout's offsets, the bytes
of the initial parameters, and which engine has slab batching / a third stream / the batched re-layout.  CPU only."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_engine_layouts as G  # noqa: E402

with open(os.path.join(G.HERE, "engine_layouts.json")) as _fh:
    GOLD = json.load(_fh)


def test_the_fixture_covers_every_configuration():
    assert sorted(GOLD) == sorted(G.configs())


@pytest.mark.parametrize("name", sorted(GOLD))
def test_engine_layout(name):
    got = json.loads(json.dumps(G.layout(G.build(name))))      # (tuples -> lists, as the fixture holds them)
    want = GOLD[name]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (name, field)
