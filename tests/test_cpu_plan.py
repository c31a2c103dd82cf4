"""The launch planner (csrc/bgp_plan.h) against what the library launched BEFORE it had one: tests/golden/lml_schedule_mi355x.json
was recorded on an MI355X (256 CUs) by tools/record_lml_schedule.py at the commit in front of the planner, from the counters of real
LML calls.  ``_lib.lml_plan`` answers without a device; path, Gram generation, generating and fused launches, the launch counts per
timing category and the launch-free task total must be the recorded integers exactly -- any glue condition of the planner that
differs from the decisions the executors used to make for themselves shows here."""
import pytest

from _plan_cases import CASES, RECORD, case_id


def plan_of(lib, c, ncu, timing):
    return lib.lml_plan(c["n"], c["B"], ncu, d=c["d"], warped=c["warped"], timing=timing,
                        persist=-1 if c["persist"] is None else c["persist"],
                        panel_fused=-1 if c["panel_fused"] is None else c["panel_fused"], nstreams=c["streams"] or 0)


@pytest.fixture(scope="module")
def lib():
    import bayes_skopt_amd  # noqa: F401
    from bayes_skopt_amd import _lib

    return _lib


def test_the_record_is_of_a_256_cu_device_and_reaches_every_branch(lib):
    assert RECORD["device_cus"] == 256 and len(CASES) == 19
    plans = [plan_of(lib, c, 256, False) for c in CASES]
    timed = [plan_of(lib, c, 256, True) for c in CASES]
    assert {p["path"] for p in plans} == {"small", "launch_free", "launches"}
    assert any(p["path"] == "launch_free" and p["pair"] for p in plans)                         # chain pairs
    assert {p["ps_gen"] for p in plans if p["path"] == "launch_free"} == {0, 1}                # Gram blocks inside / kernel in front
    assert {p["gen_first"] for p in plans if p["path"] == "launches" and p["nblk"] > 1} == {0, 1}
    assert {p["P"] for p in timed if p["nblk"] >= 4} == {2, 4}
    assert any(p["ngroups"] == 2 and p["share"] == 2 for p in plans)                             # two walker groups share the CUs
    assert any(p["nblk"] == 2 and p["fused"] == 0 for p in timed)                                # too few row blocks to fuse
    assert any(p["nblk"] > 2 and p["fused"] == 0 and c["panel_fused"] is None for p, c in zip(timed, CASES))  # one workgroup per matrix


@pytest.mark.parametrize("c", CASES, ids=case_id)
def test_planner_gives_the_schedule_the_library_launched_before_it(lib, c):
    got, want = plan_of(lib, c, 256, False), c["default"]
    assert (got["path"] == "launch_free") == bool(want["launch_free"])
    assert (got["path"] == "small") == (c["timed"]["kbuild"] == 0)  # (n <= 128: no Gram kernel, one launch)
    assert got["launch_free"] == want["launch_free"]
    assert (got["gen_groups"], got["generating"], got["fused"]) == (want["gen_batches"], want["gen_launches"], want["fused_launches"])
    if want["launch_free"]:
        assert got["total"] == want["ps_total"]  # (the Gram blocks generated inside the launch are tasks of their own)
    # under per-launch timing (no launch-free path): every launch, by category
    got, want = plan_of(lib, c, 256, True), c["timed"]
    assert got["path"] != "launch_free" and got["launch_free"] == 0
    assert (got["gen_groups"], got["generating"], got["fused"]) == (want["gen_batches"], want["gen_launches"], want["fused_launches"])
    for k, name in (("kbuild", "kbuild"), ("potrf", "potrf"), ("trsm", "trsm"), ("syrk", "syrk"), ("columns", "syrk_columns")):
        assert got[k] == want[name], (k, got[k], want[name])
    if got["path"] == "launches":  # (the per-column answer and the count agree: every group but the last has gsz matrices)
        per_group = [sum(1 for s in got[k] if s) for k in ("fused_wgs", "fused_wgs_last")]
        assert got["fused"] == (got["ngroups"] - 1) * per_group[0] + per_group[1]
