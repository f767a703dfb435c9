"""The CPU anchor of tests/eq_phase_plan.py (no GPU): the plans reach every block phase and every class of step they claim, for the
cascade in force (To) and the one faded out (From); the model alone runs over every plan, gives the same bits in one cut, stays
within test_eq_model.py's bar of the plain serial fp64 recurrence, and its output is pinned per plan, so that an edit of a plan
shows here before it shows as a changed GPU run."""
import zlib

import numpy as np
import pytest

from tests import eq_model as em
from tests import eq_phase_plan as pp
from tests.test_eq_model import same_bits

P = pp.P
SWEEPS = ("sweep-1", "sweep-3", "sweep-9")
BAR = 1e-8            # test_eq_model.py's bar for the block form against the serial recurrence, relative to the serial output's peak


def launches(names, which):
    return [(k0, n) for name in names for w, k0, n in pp.phases(pp.BY_NAME[name]) if w == which]


def fades_plans():
    return [p["name"] for p in pp.PLANS if p["name"].startswith("fades ")]


def test_the_sweeps_reach_every_start_and_end_phase():
    to = launches(SWEEPS, "to")
    assert {k0 for k0, _ in to} == set(range(P)) and {(k0 + n) % P for k0, n in to} == set(range(P))
    for name in SWEEPS + ("sweep-513", "sweep-1 C8 S8", "sweep-1 C3 S3"):
        assert {k0 for k0, _ in launches([name], "to")} == set(range(P)), name
    assert {(k0 + n) % P for k0, n in launches(["sweep-1"], "to")} == set(range(P))
    # the steps the plans were chosen for: (plan, step since the set) -> k0 and its class
    for name, step, k0, cls in (("sweep-1", 44, 36, "only_first_of_pair"), ("sweep-1", 45, 63, "first_from_history"),
                                ("sweep-3", 14, 46, "tail_first_of_pair"), ("sweep-3", 15, 63, "first_from_history"),
                                ("sweep-9", 63, 13, "grid_edge_0"), ("sweep-9", 58, 14, "grid_edge_1"),
                                ("sweep-9", 4, 12, "tail_first_of_pair"), ("sweep-9", 5, 63, "first_from_history")):
        s = list(pp.steps(pp.BY_NAME[name]))[step]
        assert s["to"][0] == k0 and cls in pp.classes(*s["to"]), (name, step, s)
    assert sum("no_pair" in pp.classes(k0, n) for k0, n in launches(["sweep-1"], "to")) == 38


def test_the_fades_reach_from_at_the_block_border_with_one_two_and_three_samples():
    frm = set(launches(fades_plans(), "from"))
    assert {(k0, n) for k0 in (0, 61, 62, 63) for n in (1, 2, 3)} <= frm
    assert "only_first_of_pair" in pp.classes(62, 1) and "only_first_of_pair" in pp.classes(61, 2) and {(62, 1), (61, 2)} <= frm
    # R = 27, 28, 29: the fade ends one sample before, on and one sample behind the step edge; R = 64 .. 66: over three steps
    for m in (7, 26, 45, 64):
        for R, want in ((27, [26]), (28, [27]), (29, [27, 1]), (64, [27, 27, 9]), (65, [27, 27, 10]), (66, [27, 27, 11])):
            pl = pp.BY_NAME[f"fades m={m} R={R}"]
            got = [s["frm"] for s in pp.steps(pl) if s["step"] >= 2 and s["frm"]]
            assert [n for _, n in got] == want and got[0][0] == 27 * m % P, (m, R, got)
    # fade-long: From's rows grow in the middle of the second fade
    got = [s["frm"][1] for s in pp.steps(pp.BY_NAME["fade-long"]) if s["frm"]]
    assert got == [27] * 7 + [10] + [27, 81, 91]


def test_the_batches_and_the_big_plan():
    want = {"batches 0+152": (0, 63, 8), "batches 0+154": (0, 63, 62), "batches 0+155": (0, 64, 25), "batches 0+157": (0, 65, 15),
            "batches 18+155": (38, 64, 63), "batches 0+304": (0, 127, 16), "batches 0+306": (0, 128, 6), "batches 7+306": (61, 129, 3)}
    for name, (k0, G, end) in want.items():
        pl = pp.BY_NAME[name]
        s = list(pp.steps(pl))[len(pl["cuts"]) - 3]
        assert (s["to"][0], pp.whole_blocks(*s["to"]), sum(s["to"]) % P) == (k0, G, end), (name, s)
    assert max(max(p["cuts"]) * p["frames"] for p in pp.PLANS) == 306 * 27
    big = list(pp.steps(pp.BY_NAME["big"]))
    assert [s["to"][0] for s in big] == [0, 0, 32] and [s["frm"] for s in big] == [(0, 699), (32, 699), None]


def test_every_class_is_reached():
    """a hard condition: a class without a launch fails, for To every class and for From every one but the long batches"""
    table = pp.coverage()
    text = pp.coverage_text(table)
    print(text)
    missing = [("to", c) for c in pp.CLASSES if not table["to"][c]] + [("from", c) for c in pp.FROM_CLASSES if not table["from"][c]]
    assert not missing, (missing, "\n" + text)
    assert set().union(*(pp.classes(k0, n) for k0 in range(P) for n in (1, 2, 27, 81, 243, 4185, 8262))) <= set(pp.CLASSES)


def test_the_coverage_check_is_not_vacuous():
    """without the batches no long batch, without the sweeps no pair that ends between its two samples"""
    table = pp.coverage([p for p in pp.PLANS if not p["name"].startswith("batches")])
    assert not table["to"]["G=64"] and not table["to"]["G=129"] and table["to"]["G=1"]
    table = pp.coverage([p for p in pp.PLANS if not p["name"].startswith("sweep")])
    assert not table["to"]["only_first_of_pair"] and table["from"]["only_first_of_pair"]
    # the classes by hand, at the borders of each
    assert pp.classes(63, 1) == {"first_from_history", "ends_on_block", "G=0", "shorter_than_history"}
    assert pp.classes(0, 62) == {"no_pair", "G=0", "shorter_than_history"} and pp.classes(0, 63) == {"only_first_of_pair", "G=0", "shorter_than_history"}
    assert pp.classes(1, 126) == {"tail_first_of_pair", "G=0"} and pp.classes(0, 128) == {"ends_on_block", "G=1"}
    assert pp.classes(13, 243) == {"ends_on_block", "grid_edge_0"} and pp.classes(14, 243) == {"grid_edge_1"}
    assert pp.classes(0, 64 * 65) == {"ends_on_block", "G=64"} and pp.classes(1, 64 * 65 - 1) == {"ends_on_block", "G=64"}


@pytest.fixture(scope="module")
def outputs():
    """the model's output of every plan, computed once"""
    return {p["name"]: pp.run_model(p) for p in pp.PLANS}


def test_the_model_over_every_plan_is_finite_and_not_silent(outputs):
    for pl in pp.PLANS:
        y = outputs[pl["name"]]
        assert y.shape == (pl["C"], pp.total_buffers(pl) * pl["frames"]) and y.dtype == np.float32, pl["name"]
        assert np.isfinite(y).all() and (np.abs(y).max(axis=1) > 0.1).all(), pl["name"]
        assert not np.array_equal(y, pp.signal(pl)), pl["name"]     # (a set is in force from sample 0 on)


def test_one_cut_gives_the_same_bits(outputs):
    one_set = [p for p in pp.PLANS if set(p["sets"]) == {0}]
    assert {p["name"] for p in one_set} >= set(SWEEPS) | {"sweep-513", "batches 7+306"}
    for pl in one_set:
        same_bits(pp.run_model(pl, cuts=[pp.total_buffers(pl)]), outputs[pl["name"]], pl["name"])


def serial_cascade(sos, state, u):
    """u [C][n] f32 through sos [C][S][5] by the plain recurrence, from and to state [C][S][4] -> [C][n] f64"""
    out = np.empty(u.shape)
    for c in range(u.shape[0]):
        y = np.ascontiguousarray(u[c], dtype=np.float64)
        for s in range(sos.shape[1]):
            nxt = np.empty_like(y)
            em.ref_lib().eq_ref_serial(em._dp(np.ascontiguousarray(sos[c, s])), y.size, em._dp(y), em._dp(state[c, s]), em._dp(nxt))
            y = nxt
        out[c] = y
    return out


def serial_twin(pl, x):
    """the fp64 signal S of every launch of a cascade, in phases()'s order, by the serial recurrence: at a set To starts from
    From's direct-form-I state"""
    to = (em.identity(pl["C"], pl["S"]), np.zeros((pl["C"], pl["S"], 4)))
    frm = None
    for s in pp.steps(pl):
        if s["step"] in pl["sets"]:
            frm = to
            to = (pp.coefficients(pl["C"], pl["S"], pl["sets"][s["step"]]), frm[1].copy())
        yield serial_cascade(to[0], to[1], x[:, s["t"]:s["t"] + s["n"]])
        if s["frm"]:
            yield serial_cascade(frm[0], frm[1], x[:, s["t"]:s["t"] + s["frm"][1]])


def test_the_model_against_the_serial_recurrence(monkeypatch):
    """every launch's fp64 output (taken where the model's cascade returns it, before the rounding to f32) against the serial
    recurrence carried through the whole plan, sets and fades included"""
    taken = []
    inner = em._Cascade.run

    def tap(self, u, t, block):
        out = inner(self, u, t, block)
        taken.append(out)
        return out

    monkeypatch.setattr(em._Cascade, "run", tap)
    worst = 0.0
    for pl in pp.PLANS:
        del taken[:]
        x = pp.signal(pl)
        pp.run_model(pl, x=x)
        want = list(serial_twin(pl, x))
        assert [a.shape for a in taken] == [b.shape for b in want] and len(want) == len(list(pp.phases(pl))), pl["name"]
        peak = max(np.abs(b).max() for b in want)
        err = max(np.abs(a - b).max() for a, b in zip(taken, want)) / peak
        worst = max(worst, err)
        assert err < BAR, (pl["name"], err)
    print(f"worst |block - serial| / peak over {len(pp.PLANS)} plans: {worst:.2e}")


PINNED = {"sweep-1": 0x07cbb15d, "sweep-3": 0x0c86c6dd, "sweep-9": 0xf6758f02, "sweep-513": 0xa659d497,
          "sweep-1 C8 S8": 0x164992b2, "sweep-1 C3 S3": 0x30d8f1b2, "batches 0+152": 0x49a35587, "batches 0+154": 0xeb70a6ff,
          "batches 0+155": 0x449d3fa0, "batches 0+157": 0x43417151, "batches 18+155": 0x6e7de82d, "batches 0+304": 0x00fa758d,
          "batches 0+306": 0xcaafb9e1, "batches 7+306": 0x85d033fb, "fades m=7 R=2": 0x72e8ba09, "fades m=7 R=3": 0x5ff9dcbc,
          "fades m=7 R=4": 0xcd4b39ac, "fades m=7 R=27": 0xef8c89ed, "fades m=7 R=28": 0x1b8ad140, "fades m=7 R=29": 0x0c41b1eb,
          "fades m=7 R=64": 0xe82d67aa, "fades m=7 R=65": 0x5d434b17, "fades m=7 R=66": 0x3ed67968, "fades m=26 R=2": 0xb6a06342,
          "fades m=26 R=3": 0x7b293891, "fades m=26 R=4": 0x0018a4ec, "fades m=26 R=27": 0x2b5e4e87,
          "fades m=26 R=28": 0xd60405ac, "fades m=26 R=29": 0x898c22aa, "fades m=26 R=64": 0x017b4eb6,
          "fades m=26 R=65": 0xd077dc3c, "fades m=26 R=66": 0xd58b8cf5, "fades m=45 R=2": 0x7bf70e7e,
          "fades m=45 R=3": 0xa39b2d55, "fades m=45 R=4": 0x16407526, "fades m=45 R=27": 0xc1c664dc,
          "fades m=45 R=28": 0xd3908429, "fades m=45 R=29": 0xa67390ce, "fades m=45 R=64": 0xa598c684,
          "fades m=45 R=65": 0x509bc02d, "fades m=45 R=66": 0x11f84b65, "fades m=64 R=2": 0x48152d6d,
          "fades m=64 R=3": 0xbf5fa509, "fades m=64 R=4": 0x8862a180, "fades m=64 R=27": 0x6aff02d4,
          "fades m=64 R=28": 0x609da8e2, "fades m=64 R=29": 0xf3a8ee89, "fades m=64 R=64": 0x2b10b22c,
          "fades m=64 R=65": 0xb8b177bd, "fades m=64 R=66": 0xf80607f4, "fades m=7 R=67 long": 0x767125d8,
          "fades m=71 R=196 long": 0x75e78df3, "fades m=71 R=197 long": 0xe982fbfe, "fade-long": 0xd8472f76,
          "sweep-1 fades": 0x4739dd8f, "big": 0xb8ffe092, "fade-sets R=0": 0xdd678964, "fade-sets R=1": 0xbdb25939,
          "fade-sets R=2": 0xc1ae5427, "fade-sets R=28": 0xc3d18793}
PINNED_BANK = 0xe88c4f5d


def test_the_model_output_is_pinned(outputs):
    """the CRC-32 of the model's f32 output per plan (the arithmetic is fma() and fp64 in a stated order: the same bits anywhere)"""
    got = {name: zlib.crc32(y.tobytes()) for name, y in outputs.items()}
    assert got == PINNED, {k: (hex(v), hex(PINNED.get(k, 0))) for k, v in got.items() if PINNED.get(k) != v}
    assert zlib.crc32(np.array(pp.coefficients(8, 8, 3)).tobytes()) == PINNED_BANK
