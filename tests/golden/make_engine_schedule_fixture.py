"""Writes tests/golden/engine_schedule.json: the launch schedule of every case of tests/engine_schedule.py, recorded on the CPU from the
fmri_hip package on the path (by default this tree's).

The committed fixture was recorded from the fmri_hip package of the commit BEFORE the decoder up-sampling routes were gathered into classes
(that commit's package in front on PYTHONPATH).  It is the evidence that the refactored engine issues the same launches; a fixture
regenerated from a later tree proves nothing about that tree.  Regenerate it only for a change that is meant to alter the schedule, and
say so.

    [PYTHONPATH=<another tree>/fetal-mri-segmentation_amd] python tests/golden/make_engine_schedule_fixture.py [out.json]
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "fetal-mri-segmentation_amd")):
    if p not in sys.path:
        sys.path.append(p)          # behind what the caller put there: another tree's fmri_hip wins

import engine_schedule as ES  # noqa: E402


def main(out):
    data = {case: ES.record(case) for case in sorted(ES.CASES)}
    packed = ES.pack(data)
    assert ES.unpack(packed) == data
    rows = lambda v, n: "[\n%s\n]" % ",\n".join(", ".join(json.dumps(e) for e in v[i:i + n]) for i in range(0, len(v), n))
    with open(out, "w") as f:          # eight layouts, one line, one case per row
        f.write('{"layouts": %s,\n"lines": %s,\n"cases": {\n%s\n}}\n' % (rows(packed["layouts"], 8), rows(packed["lines"], 1), ",\n".join(
            "%s: %s" % (json.dumps(c), json.dumps(i, separators=(",", ":"))) for c, i in packed["cases"].items())))
    print("%s: %d cases, %d lines, %d distinct" % (out, len(data), sum(len(v) for v in data.values()), len(packed["lines"])))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "engine_schedule.json"))
