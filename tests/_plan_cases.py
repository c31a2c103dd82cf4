"""The case table of tests/golden/lml_schedule_mi355x.json (tools/record_lml_schedule.py), shared by tests/test_cpu_plan.py and
tests/test_gpu_plan.py."""
import json
import os

from conftest import GOLDEN

with open(os.path.join(GOLDEN, "lml_schedule_mi355x.json")) as _f:
    RECORD = json.load(_f)
CASES = RECORD["cases"]


def case_id(c):
    extra = [k + "=" + str(c[k]) for k in ("streams", "panel_fused", "persist") if c[k] is not None]
    return "-".join(["%dx%d" % (c["n"], c["B"])] + (["d%d" % c["d"]] if c["d"] != 4 else []) + (["warped"] if c["warped"] else []) + extra)
