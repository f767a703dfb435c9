"""tests/master_window_plan.py held to its claims, without a GPU: the plan reaches every level count k = 1 .. 16 of the master bus's
sliding minimum, every count 0 .. 6 of passes over the whole array (so both arrays of the ping-pong hold a last pass), D = 0, 1 and
2^k - 1 at every k where such a W exists, and both gain launches; on every case's staircase a(t) rises on at least three samples
and falls on at least three, and the exits and entries placed on the borders of the minimum's strips and of the steps are there
and move a(t); the model gives the same bits for both cuts of every case."""
import time

import numpy as np
import pytest

from tests import master_window_plan as wp
from tests.master_model import Model

CASES = wp.cases()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def model_run(case, x, cut):
    m = Model(case["C"], wp.T, case["L"], case["H"], 0)
    ys, gs, ms, at = [], [], [], 0
    for nb in cut:
        ys.append(m.process(x[:, at * wp.B:(at + nb) * wp.B]))
        gs.append(m.gains)
        ms.append(m.meters)
        at += nb
    return np.concatenate(ys, axis=1), np.concatenate(gs), np.concatenate(ms, axis=0)


@pytest.fixture(scope="module")
def runs():
    """every case: its input and layout, a(t) by the plan's own numpy minimum, and the model's output for both cuts"""
    out, t0 = [], time.perf_counter()
    for case in CASES:
        x, lay = wp.staircase(case)
        a = wp.window_minimum(wp.ratios(x), case["W"])
        single, uneven = wp.cuts(lay["n"] // wp.B)
        out.append(dict(case=case, x=x, lay=lay, a=a, single=single, uneven=uneven, one=model_run(case, x, single),
                        many=model_run(case, x, uneven)))
    return out, time.perf_counter() - t0


def test_classes_against_hand_computed_cases():
    c = wp.classes(1, 0, 513)
    assert (c["W"], c["k"], c["lds_levels"], c["passes"], c["D"], c["wide"], c["gain_strips"], c["ragged"]) == (2, 1, 1, 0, 0, False, 9, True)
    c = wp.classes(2, 65536, 3 * 513)                    # tests/test_gpu_master.py's longest hold
    assert (c["W"], c["k"], c["lds_levels"], c["passes"], c["D"], c["last_in"]) == (65539, 16, 10, 6, 3, "M0")
    c = wp.classes(300, 5000, 33 * 513)                  # and its hold beyond the LDS levels on the wide launch
    assert (c["W"], c["k"], c["passes"], c["D"], c["wide"], c["gain_strips"], c["ragged"]) == (5301, 12, 2, 1205, True, 17, True)
    c = wp.classes(4096, 65536, 64 * 256)
    assert (c["W"], c["k"], c["passes"], c["D"], c["wide"], c["gain_strips"], c["ragged"]) == (69633, 16, 6, 4097, True, 16, False)
    c = wp.classes(1, 2046, 64 * 513)                    # W = 2048: the first pass over the whole array, its result in M1
    assert (c["k"], c["lds_levels"], c["passes"], c["D"], c["last_in"], c["wide"]) == (11, 10, 1, 0, "M1", True)
    assert wp.classes(1, 1021, 64)["lds_levels"] == 9 and wp.classes(1, 1022, 64)["lds_levels"] == 10
    assert not wp.classes(1, 0, 16383)["wide"] and wp.classes(1, 0, 16384)["wide"]


def test_the_numpy_minimum_is_the_sliding_minimum():
    rng = np.random.default_rng(0)
    r = rng.uniform(0, 1, 300).astype(np.float32)
    padded = np.concatenate([np.ones(200, dtype=np.float32), r])
    for W in (1, 2, 3, 4, 5, 7, 8, 9, 31, 32, 33, 100, 127, 128, 129):
        want = np.array([padded[200 + t - W + 1:200 + t + 1].min() for t in range(300)], dtype=np.float32)
        assert np.array_equal(wp.window_minimum(r, W), want), W


def test_the_plan_holds_every_window_around_a_power_of_two():
    ws = set(wp.windows())
    for k in range(1, 17):
        assert {W for W in ((1 << k) - 1, 1 << k, (1 << k) + 1) if W >= 2} <= ws
    assert wp.MAX_L + wp.MAX_H + 1 == 69633 in ws
    by_w = {}
    for c in CASES:
        by_w.setdefault(c["W"], []).append(c)
        assert 1 <= c["L"] <= wp.MAX_L and 0 <= c["H"] <= wp.MAX_H and c["L"] + c["H"] + 1 == c["W"]
    assert set(by_w) == ws
    for W, cs in by_w.items():
        # L = 1 at every W that a hold of at most 65536 leaves it; the two beyond run with L = 2048 and L = 4096
        assert any(c["L"] == 1 for c in cs) or (W > wp.MAX_H + 2 and cs[0]["L"] == {67584: 2048, 69633: 4096}[W])
        assert any(c["H"] == 0 for c in cs) == (W <= 4097)
    assert len({c["name"] for c in CASES}) == len(CASES)
    for Cn in (1, 3, 8):                                 # the channel counts are spread: each one at short and at long windows
        ks = {wp.classes(c["L"], c["H"], 513)["k"] for c in CASES if c["C"] == Cn}
        assert min(ks) <= 2 and max(ks) == 16 and len(ks) >= 12


def test_the_plan_reaches_every_class(runs):
    seen = []
    for r in runs[0]:
        c = r["case"]
        for cut in (r["single"], r["uneven"]):
            for nb in cut:
                seen.append(wp.classes(c["L"], c["H"], nb * wp.B))
    assert {s["k"] for s in seen} == set(range(1, 17))
    assert {s["lds_levels"] for s in seen} == set(range(1, 11))
    assert {s["passes"] for s in seen} == set(range(0, 7))
    for k in range(1, 17):
        ds = {s["D"] for s in seen if s["k"] == k}
        assert {0, 1} <= ds
        if (2 << k) - 1 <= wp.MAX_L + wp.MAX_H + 1:      # W = 2^(k+1) - 1 exists up to k = 15
            assert (1 << k) - 1 in ds
        else:
            assert k == 16 and max(ds) == 4097
        if k >= 11:
            assert any((1 << k) // 4 <= d <= 3 * (1 << k) // 4 or (k == 16 and d == 2048) for d in ds), k   # D in mid range
    # every count of passes on both gain launches; the last pass's result in M1 (never run before this plan) and in M0
    # (without a pass, W < 2048, a staircase is shorter than a wide launch: tests/test_gpu_master.py and the border test of
    # tests/test_gpu_master_windows.py run those)
    assert {s["wide"] for s in seen if s["passes"] == 0} == {False}
    for p in range(1, 7):
        assert {s["wide"] for s in seen if s["passes"] == p} == {False, True}, p
    assert {s["last_in"] for s in seen} == {"M0", "M1"}
    # the narrow launch at its longest step, 31 buffers; wide launches of 16 strips up
    assert max(s["gain_strips"] for s in seen if not s["wide"]) == -(-31 * wp.B // 64)
    assert min(s["gain_strips"] for s in seen if s["wide"]) <= 24
    for r in runs[0]:
        if r["case"]["W"] >= 2048:
            assert len(r["uneven"]) >= 5 and r["uneven"][1] == 1 and max(r["uneven"]) <= 31
            assert all(not wp.classes(r["case"]["L"], r["case"]["H"], nb * wp.B)["wide"] for nb in r["uneven"])
        if r["lay"]["n"] >= 16384:
            assert wp.classes(r["case"]["L"], r["case"]["H"], r["lay"]["n"])["wide"]


def test_every_staircase_moves_the_minimum_where_the_plan_says(runs):
    for r in runs[0]:
        c, lay, a, name = r["case"], r["lay"], r["a"], r["case"]["name"]
        W, HL, n = c["W"], 2 * c["L"] + c["H"], lay["n"]
        # eight peaks W / 24 apart; each run waits at most twice for a strip border and once for a step border behind 31 buffers
        assert n % wp.B == 0 and n <= 100000 and n <= W + 2 * W // 5 + 2 * (2 * 1024 + 31 * wp.B) + wp.B, name
        da = np.diff(np.concatenate([np.ones(1, dtype=np.float32), a]))
        assert (da > 0).sum() >= 3 and (da < 0).sum() >= 3, name
        pos = [p for p, _, _ in lay["peaks"]]
        assert pos == sorted(set(pos)) and pos[0] >= 1 and pos[-1] < n
        assert {ch for _, ch, _ in lay["peaks"]} == set(range(min(c["C"], 8)))      # the peaks rotate over all the channels
        assert a.max() == 1 and (wp.ratios(r["x"]) < 1).sum() == 8                   # r = 1 between the peaks
        starts = np.cumsum([0] + r["uneven"])[:-1] * wp.B
        ends = np.cumsum(r["uneven"]) * wp.B
        assert set(lay["exits"]) == set(lay["entries"]) == set(wp.KINDS)
        for events, moved in ((lay["exits"], lambda t: a[t] > a[t - 1]), (lay["entries"], lambda t: a[t] < a[t - 1])):
            for kind, t in events.items():
                assert 1 <= t < n and moved(t), (name, kind, t)
            assert (HL + events["strip-last"]) % 1024 == 1023 and (HL + events["strip-first"]) % 1024 == 0, name
            assert events["step-last"] + 1 in ends and events["step-first"] in starts[1:], name
        for t in lay["exits"].values():                  # an exit is the first sample whose window no longer holds the peak
            assert t - W in pos
        for t in lay["entries"].values():
            assert t in pos


def test_the_model_agrees_with_the_plan_and_with_itself_on_both_cuts(runs):
    for r in runs[0]:
        c, name = r["case"], r["case"]["name"]
        y1, g1, m1 = r["one"]
        y2, g2, m2 = r["many"]
        assert np.array_equal(bits(y1), bits(y2)) and np.array_equal(bits(g1), bits(g2)) and m1.tobytes() == m2.tobytes(), name
        assert np.abs(y1).max() <= np.float32(wp.T)
        if c["L"] == 1:                                  # w = [1]: g(t) = min(a(t), r(t - 1)) = a(t)
            assert np.array_equal(bits(g1), bits(r["a"])), name
        else:
            assert g1.max() <= 1 and (g1 < 1).any(), name
    assert runs[1] < 10.0, runs[1]                       # the whole plan through the model, twice: seconds
