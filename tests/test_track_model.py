"""What makes tests/track_model.py a yardstick: on every script the C oracle can play, the model equals the oracle (no GPU).

* track-free scripts (point, Gaussian, clearAllForces, sustained start / end): 1e-12 relative, the bar of
  test_oracle_crosschecks.py::test_step_bookkeeping_oracle_vs_python_restatement -- per sample and in the lfilter form;
* the one-sample track [1.0] at start_sample 0 is the oracle's PointForce, and at start_sample s that output s samples later,
  across buffer boundaries;
* a sustained stroke with a looping track of the constant mu is the oracle's sustained AutoregressiveForce after
  enqueue_arprm(a, sigma = 0, mu): sigma = 0 makes the AR profile the constant mu from its first buffer on."""
import numpy as np
import pytest

from openpbso_amd import capi, synth
from tests.scenarios import B, ObjSpec, force_ev, run_oracle
from tests.track_model import run_model, track_ev, track_total, track_value

REL = 1e-12


def _close(got, want, what):
    peak = np.abs(want).max()
    err = np.abs(got - want).max() / max(peak, 1e-300)
    print(f"{what}: max|model - oracle| / peak = {err:.3e}")
    assert err <= REL, (what, err)


def _unit(objs):
    return [dict(t=0, obj=i, kind="use_transfer", use=False) for i in range(len(objs))]


def _track_free_script(n, rng):
    d = [rng.standard_normal(n) * 1e-3 for _ in range(10)]
    return [
        force_ev(0, 0, data=d[0], force_type=1, width=3000.0),               # a long Gaussian (3 buffers)
        force_ev(1, 0, data=d[1]), force_ev(1, 0, data=d[2]),                # two hits in one frame: one per step
        force_ev(4, 0, clear=True, data=np.zeros(n)),
        force_ev(5, 0, data=d[3]),
        force_ev(6, 0, data=d[4], force_type=1, width=0.0),                  # zero width: rejected at once
        force_ev(7, 0, data=d[5], force_type=1, width=150.0),
        force_ev(9, 0, data=np.zeros(n), force_type=1, width=9000.0, start=True),      # a sustained Gaussian, its data replaced
        force_ev(10, 0, data=d[6], force_type=1, width=9000.0),
        force_ev(11, 0, data=d[7], force_type=1, width=9000.0),
        force_ev(13, 0, data=d[8], force_type=1, width=9000.0, end=True),
        force_ev(15, 0, data=d[9]),
    ]


@pytest.mark.parametrize("per_sample", [True, False])
def test_track_free_scripts_equal_the_oracle(oracle, per_sample):
    n = 12
    objs = [ObjSpec(synth.eigenvalues(n, 17))]
    evs = _unit(objs) + _track_free_script(n, np.random.default_rng(17))
    want = run_oracle(objs, evs, 18)
    got = run_model(objs, [], evs, 18, per_sample=per_sample)
    assert np.array_equal(got["emitted"], want["emitted"]) and not want["emitted"].all()
    _close(got["audio"], want["audio"], f"track-free script, per_sample={per_sample}")
    for key, row in want["qnorm"].items():
        np.testing.assert_allclose(got["qnorm"][key], row, rtol=1e-9 if not per_sample else REL, atol=REL * np.abs(row).max() + 1e-300)
    for (a1, a2), (b1, b2) in zip(got["state"], want["state"]):
        _close(np.concatenate([a1, a2]), np.concatenate([b1, b2]), "final state")


def test_lfilter_form_on_a_long_gaussian(oracle):
    """a 9 ms Gaussian over six buffers"""
    n = 16
    objs = [ObjSpec(synth.eigenvalues(n, 19))]
    evs = _unit(objs) + [force_ev(1, 0, data=np.random.default_rng(19).standard_normal(n) * 1e-3, force_type=1, width=9000.0)]
    want = run_oracle(objs, evs, 9)
    _close(run_model(objs, [], evs, 9, per_sample=False)["audio"], want["audio"], "lfilter form, 9 ms Gaussian")


@pytest.mark.parametrize("s", [0, 1, 17, 256, 512])
def test_one_sample_track_is_a_point_force_delayed_by_start_sample(oracle, s):
    n = 24
    objs = [ObjSpec(synth.eigenvalues(n, 29))]
    d = np.random.default_rng(29).standard_normal(n) * 1e-3
    nb = 5
    want = run_oracle(objs, _unit(objs) + [force_ev(1, 0, data=d)], nb)["audio"][0]
    got = run_model(objs, [np.array([1.0])], _unit(objs) + [track_ev(1, 0, 0, start_sample=s, data=d)], nb)
    assert got["track_rows"] == 1
    delayed = np.concatenate([np.zeros(s), want[:nb * B - s]])
    _close(got["audio"][0], delayed, f"delta track, start_sample {s}")


def test_constant_looping_track_is_the_ar_force_with_sigma_zero(oracle):
    n, nb, mu = 20, 12, 0.140625                                             # (mu exact in f32: a track is f32)
    objs = [ObjSpec(synth.eigenvalues(n, 31))]
    rng = np.random.default_rng(31)
    data = [rng.standard_normal(n) * 1e-3 for _ in range(8)]

    def script(first, **kw):
        evs = [first(0, start=True)]
        evs += [force_ev(1 + k, 0, data=dk, **kw) for k, dk in enumerate(data)]
        return evs + [force_ev(9, 0, data=np.zeros(n), end=True, **kw)]
    ar = _unit(objs) + [dict(t=0, obj=0, kind="arprm", a=[0.783, 0.116], sigma=0.0, mu=mu)]
    ar += script(lambda t, **k: force_ev(t, 0, data=np.zeros(n), force_type=2, **k), force_type=2)
    tr = _unit(objs) + script(lambda t, **k: track_ev(t, 0, 0, loop=True, data=np.zeros(n), **k))
    want = run_oracle(objs, ar, nb)
    got = run_model(objs, [np.array([mu])], tr, nb)
    assert got["track_rows"] == 9                                            # buffers 0 .. 8; the end message clears the list first
    _close(got["audio"], want["audio"], "constant looping track against AR(sigma = 0)")


def test_track_arithmetic_corners():
    s = np.array([1.0, 3.0, -2.0, 0.5], dtype=np.float32)
    assert track_value(s, 1.0, 1.0, 2.0, False, 1) == -4.0                   # f == 0 reads S(i) exactly
    assert track_value(s, 0.5, 1.0, 1.0, False, 0) == 2.0
    assert track_value(s, 3.5, 1.0, 1.0, False, 0) == 0.25                   # S(L) = 0 without loop
    assert track_value(s, 3.5, 1.0, 1.0, True, 0) == 0.75                    # ... s[0] with it
    assert track_value(s, 0.0, 1.0, 1.0, False, 7) == 0.0
    assert track_total(4, 0.0, 1.0, 0, False) == 4 and track_total(4, 0.0, 0.5, 0, False) == 8
    assert track_total(4, 4.0, 1.0, 0, False) == 0 and track_total(4, 3.999, 2.5, 0, False) == 1
    assert track_total(4, 0.0, 1.0, 9, False) == 9 and track_total(4, 0.0, 1.0, 0, True) == float("inf")
    for first, rate in ((0.3, 0.37), (1.7, 2.5), (0.0, 1.0 / 3.0)):
        N = track_total(4000, first, rate, 0, False)
        assert first + rate * float(N - 1) < 4000 <= first + rate * float(N)
    assert capi.TRACK_FORCE == 3
