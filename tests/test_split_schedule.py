"""The launch schedule of the fp32-storage ST-GCN train step is what tests/golden/split_schedule.json recorded (written once by
tests/golden/make_golden_split_schedule.py, before the split engines' per-launch decisions moved into sar_amd/split_plan.py): for both
split arithmetics and every subset of the nine kernel kinds of SAR_SPLIT_KINDS, which launch takes which arithmetic, which term image, weight
bound and bound cell it is handed and which pass raises which cell, in issue order (a digest of three hex digits per entry, so a
mismatch names the first entry that differs).  Every configuration also keeps the two invariants of the bound cells: a cell
read by an fp16 split launch was raised earlier in the step, and no cell is raised that nothing reads.  CPU only."""
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_golden_split_schedule as G  # noqa: E402

with open(os.path.join(G.HERE, "split_schedule.json")) as _fh:
    GOLD = json.load(_fh)


def test_the_fixture_covers_every_configuration():
    want = {G.key(m, ks) for m in G.SPLIT_MODES for ks in G.subsets()} | {G.key(m, ("default",)) for m in ("fp32", "bf16_operands")}
    assert len(want) == 1026 and set(GOLD["digests"]) == want
    assert set(GOLD["traces"]) == {"%s|%s" % c for c in G.FULL_TRACES}


@pytest.mark.parametrize("mode", G.SPLIT_MODES)
def test_every_kind_subset_keeps_the_recorded_schedule(mode):
    for ks in G.subsets():
        tr = G.trace(mode, ks)
        name = G.key(mode, ks)
        got, want = G.digest(tr), GOLD["digests"][name]
        if got != want:      # the digest has three hex digits per entry of the trace: name the first entry that differs
            n = G.first_difference(got, want)
            full = GOLD["traces"].get(name, [])      # (four configurations are spelled out in the fixture)
            recorded = full[n] if n < len(full) else ("digest " + want[3 * n:3 * n + 3] if n < len(want) // 3 else "nothing")
            pytest.fail("%s: entry %d of the schedule is %s; recorded: %s (%d entries, recorded %d)" % (
                name, n, tr[n] if n < len(tr) else "missing", recorded, len(tr), len(want) // 3))
        assert not G.check_invariants(tr), (name, G.check_invariants(tr))
        if mode == "f32_split_bf16x6":
            assert not any("raise" in ev or "bounds" in ev for ev in tr), name      # this arithmetic scales nothing: no cells


@pytest.mark.parametrize("mode", ["fp32", "bf16_operands"])
def test_engines_without_a_split_arithmetic(mode):
    tr = G.trace(mode)
    assert G.digest(tr) == GOLD["digests"][G.key(mode, ("default",))]
    assert not any("raise" in ev or ev["split"] for ev in tr)
