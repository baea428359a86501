"""The constructor of Path B's classifier lays out what tests/golden/resnet_layouts.json recorded (written once by
tests/golden/make_golden_resnet_layouts.py, before the engine moved onto sar_amd/engine.py): parameter names, shapes and offsets in
order, flat size, gradient buckets in hand-over order, BatchNorm names, the data-gradient re-layout, the bytes of the initial
parameters, and which streams / images a CPU engine has (no streams; term images exactly in a split arithmetic).  CPU only."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_resnet_layouts as G  # noqa: E402

with open(os.path.join(G.HERE, "resnet_layouts.json")) as _fh:
    GOLD = json.load(_fh)


def build(name):
    """on the CPU, as it is: no patch of torch.cuda (the generator's build() carries one for the commit the fixture was written at)"""
    from sar_amd.resnet import ResNet18
    return ResNet18(device="cpu", num_classes=7, seed=0, **G.configs()[name])


def test_the_fixture_covers_every_configuration():
    assert sorted(GOLD) == sorted(G.configs())


@pytest.mark.parametrize("name", sorted(GOLD))
def test_resnet_layout(name):
    got = json.loads(json.dumps(G.layout(build(name))))      # (tuples -> lists, as the fixture holds them)
    want = GOLD[name]
    assert sorted(got) == sorted(want)
    for field in want:
        assert got[field] == want[field], (name, field)


@pytest.mark.parametrize("name", sorted(GOLD))
def test_buckets_partition_the_flat_gradient_in_backward_order(name):
    """as tests/test_ddp_gloo.py asserts for STGCN: contiguous slices, handed over from the end of the buffer to its start, together
    [0, total) without gaps; the last one is complete at the end of backward only"""
    eng = build(name)
    total, hi = eng.grad.numel(), eng.grad.numel()
    for blk, lo, top in eng._buckets:
        assert top == hi and 0 <= lo < top, (blk, lo, top)
        hi = lo
    assert hi == 0 and sum(top - lo for _, lo, top in eng._buckets) == total
    done_at = [blk for blk, _, _ in eng._buckets]
    assert done_at[-1] == -1 and all(b >= 0 for b in done_at[:-1]) and done_at[:-1] == sorted(done_at[:-1], reverse=True)
    for blk, lo, top in eng._buckets[:-1]:      # a bucket starts with the first parameter of the block that completes it
        assert lo == eng.offsets[eng.blocks[blk][0] + "conv1.weight"]
