"""The launch schedule of the train step of Path B's classifier (sar_amd/resnet.py) is what tests/golden/pathb_schedule.json recorded
(written once, on the GPU, by tests/golden/make_golden_pathb_schedule.py at the commit before the engine's per-launch decisions moved
into sar_amd/split_plan.py): for both split arithmetics times every subset of the kinds of SAR_SPLIT_KINDS_PATHB and for fp32, on two
clips, every launch in issue order -- which convolution asks for which arithmetic and is left with which, the term image, weight bound
and bound cells it is handed, which pass raises which cell, every fork and join (a digest of three hex digits per entry, so a mismatch
names the first entry that differs).  Every configuration also keeps the invariant of the bound cells that this engine has: a cell read
by an fp16 split launch was raised earlier in the step (a cell here may be raised and never read: ResNetPlan's docstring).  The
configurations without streams are replayed on the CPU; the two forked ones need the engine's streams: one GPU test, which launches
none of the project's kernels."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_pathb_schedule as G  # noqa: E402
from make_golden_split_schedule import digest, first_difference, unraised_reads  # noqa: E402

with open(os.path.join(G.HERE, "pathb_schedule.json")) as _fh:
    GOLD = json.load(_fh)


def check(mode, kinds, forked, device):
    for clip, tr in zip(G.CLIPS, G.traces(mode, kinds, forked, device)):
        name = G.key(mode, kinds, forked, clip)
        got, want = digest(tr), GOLD["digests"][name]
        if got != want:      # the digest has three hex digits per entry of the trace: name the first entry that differs
            n = first_difference(got, want)
            full = GOLD["traces"].get(name, [])      # (the all-kinds configurations without streams are spelled out in the fixture)
            recorded = full[n] if n < len(full) else ("digest " + want[3 * n:3 * n + 3] if n < len(want) // 3 else "nothing")
            pytest.fail("%s: entry %d of the schedule is %s; recorded: %s (%d entries, recorded %d)" % (
                name, n, tr[n] if n < len(tr) else "missing", recorded, len(tr), len(want) // 3))
        assert not unraised_reads(tr)[0], (name, unraised_reads(tr)[0])
        if mode == "fp32":
            assert not any("raise" in ev or ev.get("asked") for ev in tr), name


def test_the_fixture_covers_every_configuration():
    want = {G.key(m, ks, forked, clip) for m, ks, forked in G.configs() for clip in G.CLIPS}
    assert len(want) == 38 and set(GOLD["digests"]) == want
    assert set(GOLD["traces"]) == set(G.FULL_TRACES)
    for name in G.FULL_TRACES:
        assert digest(GOLD["traces"][name]) == GOLD["digests"][name]


def test_both_clips_cover_admitted_and_demoted_launches():
    """what the clips were chosen for, read from the recorded traces: every family has launches that keep the split kernels and launches
    the wrapper demotes, and the compact stride-2 skip gradient runs"""
    evs = [ev for name in G.FULL_TRACES if name.startswith("f32_split|") for ev in GOLD["traces"][name] if ev.get("op") == "conv2d_gemm"]
    for transposed in (False, True):
        assert {bool(ev["split"]) for ev in evs if ev["asked"] and ev["transposed"] == transposed} == {True, False}
    assert any(ev["even"] and ev["split"] for ev in evs)


@pytest.mark.parametrize("mode,kinds", [(m, ks) for m, ks, forked in G.configs() if not forked],
                         ids=lambda v: v if isinstance(v, str) else ",".join(v) if v is not None else "default")
def test_the_serial_step_keeps_the_recorded_schedule(mode, kinds):
    check(mode, kinds, False, "cpu")


@pytest.mark.gpu
def test_the_forked_step_keeps_the_recorded_schedule():
    for mode in G.SPLIT_MODES:
        check(mode, G.KINDS, True, "cuda")
