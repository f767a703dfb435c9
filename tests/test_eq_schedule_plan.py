"""The CPU anchor of tests/eq_schedule_plan.py (no GPU): the plans reach every case they claim -- every offset at which a set cuts
its predecessor's block, every R, sets 1 and R - 1 apart, the runs of one-sample sets at a step end, sets on a step's first and last
sample, tails that end around a step end, the borders of the groups of 256 positions and of the chain's batches of 64 blocks, steps
shorter than the history --; every plan obeys the schedule's spacing rule (the model's own assertion) and stays small; the model
alone runs over every plan and gives the same bits however its pieces are cut."""
import numpy as np
import pytest

from tests import eq_model as em
from tests import eq_schedule_plan as sp
from tests.test_eq_model import same_bits


def test_every_case_is_reached():
    reached = {}
    for pl in sp.PLANS:
        for r in sp.reach(pl):
            reached.setdefault(r, []).append(pl["name"])
    missing = [r for r in sp.REQUIRED if r not in reached]
    print("\n".join(f"{r:22s} {len(reached.get(r, [])):3d}  {', '.join(reached.get(r, [])[:3])}" for r in sp.REQUIRED))
    assert not missing, missing


def test_the_coverage_check_is_not_vacuous():
    def reached(plans):
        return set().union(*(sp.reach(p) for p in plans))

    assert not {"run70 -1", "run70 +0", "run70 +1"} & reached([p for p in sp.PLANS if not p["name"].startswith("run70")])
    assert {"V batch block 63", "V batch block 64", "V batch block 65"} <= sp.reach(sp.BY_NAME["batch-edge V"])
    assert "F batch edge" in sp.reach(sp.BY_NAME["batch-edge F R=200"]) and "F batch edge" not in sp.reach(sp.BY_NAME["batch-edge V"])
    for R in (3, 64, 200):
        for d in (-1, 0, 1):
            assert f"tail end {d:+d}" in sp.reach(sp.BY_NAME[f"tail-end R={R} d={d}"]), (R, d)
    assert not {"tail end -1", "tail end +0", "tail end +1"} & sp.reach(sp.BY_NAME["first-last R=0"])
    without = reached([p for p in sp.PLANS if not p["name"].startswith("offsets")])
    assert len([r for r in without if r.startswith("offset=")]) < em.P
    # the chosen samples, by hand
    assert "group offset 256" in sp.reach(sp.BY_NAME["group-edge R=0"]) and "first sample" in sp.reach(sp.BY_NAME["first-last R=64"])
    assert "last sample" in sp.reach(sp.BY_NAME["first-last R=64"]) and "n<H" in sp.reach(sp.BY_NAME["short-steps R=3"])
    assert sp.vblocks(sp.BY_NAME["first-last R=0"], 54, 27, 0) == [(54, 26, 54), (80, 1, 80)]


def test_the_plans_obey_the_rules_and_stay_small():
    for pl in sp.PLANS:
        ts, R = sorted(pl["sets"]), pl["R"]
        assert pl["frames"] in (27, 513) and sp.total(pl) <= 20000 and len(ts) <= 300, pl["name"]
        assert ts[0] >= 0 and ts[-1] < sp.total(pl), pl["name"]
        # the identity is a predecessor at 0; every set against the one before it
        for a, b in zip([0] + ts[:-1], ts):
            assert b > a or (a == 0 and b == 0 and R < 2), (pl["name"], a, b)
            assert R < 2 or b - a + 1 >= R, (pl["name"], a, b)


@pytest.fixture(scope="module")
def outputs():
    """the model's output of every plan, computed once"""
    return {p["name"]: sp.run_model(p) for p in sp.PLANS}


def test_the_model_over_every_plan_is_finite_and_not_silent(outputs):
    for pl in sp.PLANS:
        y = outputs[pl["name"]]
        assert y.shape == (pl["C"], sp.total(pl)) and y.dtype == np.float32, pl["name"]
        assert np.isfinite(y).all() and (np.abs(y).max(axis=1) > 0.1).all(), pl["name"]
        assert not np.array_equal(y, sp.signal(pl)), pl["name"]


def test_the_model_does_not_depend_on_the_step_edges(outputs):
    """cut at the t_sets alone (one step), and at every buffer as well: the same bits"""
    for pl in sp.PLANS:
        for label, cuts in sp.other_cuts(pl).items():
            if label == "one buffer per step" and sp.total(pl) > 6000:
                continue                                  # (thousands of pieces of the model: the short plans show it)
            same_bits(sp.run_model(dict(pl, cuts=cuts)), outputs[pl["name"]], (pl["name"], label))
