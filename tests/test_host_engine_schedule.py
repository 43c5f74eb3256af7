"""UNetEngine issues the launches it issued before its decoder routes were gathered into classes: every case of tests/engine_schedule.py,
recorded on the CPU, line for line against tests/golden/engine_schedule.json (no launch reordered, merged, added or dropped, no buffer laid
out differently, the same in-place torch ops).  A difference is a defect of the engine, never a reason to regenerate the fixture."""
import json
import os

import pytest

import engine_schedule as ES


@pytest.fixture(scope="module")
def fixture(golden_dir):
    with open(os.path.join(golden_dir, "engine_schedule.json")) as f:
        return ES.unpack(json.load(f))


def test_the_fixture_holds_exactly_the_cases(fixture):
    assert sorted(fixture) == sorted(ES.CASES)


@pytest.mark.parametrize("case", sorted(ES.CASES))
def test_engine_schedule_is_the_recorded_one(fixture, case, monkeypatch):
    for k in [k for k in os.environ if k.startswith("FMRI_")]:
        monkeypatch.delenv(k)
    got, want = ES.record(case), fixture[case]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, "%s: line %d differs\n  recorded: %s\n  fixture:  %s" % (case, i, g, w)
    assert len(got) == len(want), "%s: %d lines recorded, %d in the fixture; first extra: %s" % (
        case, len(got), len(want), max(got, want, key=len)[min(len(got), len(want))])
