"""What the layer wrappers of sar_amd.ops (pgc_*, pgpool_*, gpool_*, tattn_*, adjattn_*), the shared 1x1 product (ops.conv1x1_fwd /
conv1x1_wgrad / conv1x1_dgrad, ops.column_geometry) and the modules built on them hand to the C ABI is what
tests/golden/layer_launch_abi.json recorded at the commit its header names (written once by
tests/golden/make_golden_layer_launch_abi.py): every library call in issue order with its scalars, leading dimensions, pointer offsets
and pointer identities (tests/abi_trace.py; a digest of three hex digits per call, so a mismatch names the first call that differs).
CPU only: nothing is launched."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_layer_launch_abi as G  # noqa: E402
from test_conv_launch_abi import knob_set  # noqa: E402

FIXTURE = os.path.join(G.HERE, "layer_launch_abi.json")
with open(FIXTURE) as _fh:
    GOLD = json.load(_fh)


def test_the_fixture_names_its_commit_and_covers_every_case():
    assert GOLD["commit"] == G.COMMIT and G.COMMIT in GOLD["header"]
    count = {}
    for group, name, _ in G.cases():
        count[group] = count.get(group, 0) + 1
    assert count == {g: len(v) for g, v in GOLD["digests"].items()}
    assert all(d for v in GOLD["digests"].values() for d in v), "a case that recorded no call"
    assert set(GOLD["traces"]) == set(G.FULL)
    assert os.path.getsize(FIXTURE) <= os.path.getsize(os.path.join(G.HERE, "conv_launch_abi.json"))


@pytest.mark.parametrize("group", [g for g, _ in G.GROUPS])
def test_every_case_hands_the_library_what_was_recorded(group):
    knob = knob_set()
    if knob is not None:
        pytest.skip("%s is set: the fixture was recorded with the default of every SAR_* knob" % knob)
    want = iter(GOLD["digests"][group])
    for g, name, fn in G.cases():
        if g != group:
            continue
        calls, rec = G.record(fn), next(want)
        got = G.digest(calls)
        if got != rec:      # the digest has three hex digits per call: name the first call that differs
            n = G.first_difference(got, rec)
            full = GOLD["traces"].get(name, [])      # (a few cases are spelled out in the fixture)
            recorded = full[n] if n < len(full) else ("digest " + rec[3 * n:3 * n + 3] if n < len(rec) // 3 else "nothing")
            pytest.fail("%s: call %d is %s; recorded: %s (%d calls, recorded %d)" % (
                name, n, calls[n] if n < len(calls) else "missing", recorded, len(calls), len(rec) // 3))


def test_the_spelled_out_traces_are_the_digested_ones():
    """the readable copies in the fixture are the traces their digests were taken from"""
    index = {name: (group, k) for group, gen in G.GROUPS for k, (name, _) in enumerate(gen())}
    for name, trace in GOLD["traces"].items():
        group, k = index[name]
        assert G.digest(trace) == GOLD["digests"][group][k], name
