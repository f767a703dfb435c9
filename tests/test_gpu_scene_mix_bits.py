"""The scene mix (include/openpbso_amd.h "scene mix"; kernels_mix.hip) on the device, every output compared BIT FOR BIT with the
reference of the stated order of arithmetic (tests/cpp/scene_mix_ref.c through tests/scene_mix_model.py, anchored by
tests/test_scene_mix_model.py): every channel count (each its own build of stage 1, batches of 8, 4, 2 and 1 objects), the
steady and the per-sample path, ramps that end at, before and after a 64-sample tile's start, and the edges of the delay.
The rows are the engine's own audio of the same step: objects of 64 modes, each hit at buffer 0."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, synth
from tests.scene_mix_model import Model

pytestmark = pytest.mark.gpu
B = 513


def make_engine(n_obj, nb_total, seed, n_modes=64, force=1e-3):
    eng = Engine()
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 8000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), 2)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * force), t)
    return eng


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    assert np.abs(want).max() > 0, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def set_both(eng, model, gain, delay=None):
    g = np.asarray(gain, dtype=np.float32)
    d = None if delay is None else np.asarray(delay, dtype=np.float32)
    eng.scene_mix_set(g, d)
    model.set(g, d)


def step_and_mix(eng, model, nb, label, samples=None, silent=False):
    """one step of nb buffers through the engine's mixer and, with the same rows, through the model"""
    eng.step(nb)
    eng.scene_mix()
    rows = eng.audio()
    got = eng.read_scene_mix()
    assert got.shape == (model.C, nb * B) and np.abs(rows).max(axis=1).min() > 0, label     # (no row is silent)
    want = model.mix(rows, samples)
    if samples is not None:
        got = np.ascontiguousarray(got[:, samples])
    if silent:
        assert not want.any() and not got.view(np.uint32).any(), label
    else:
        same_bits(got, want, label)


def signed(rng, lo, hi, shape):
    """magnitudes in [lo, hi) of either sign: about half of the gains are negative"""
    return rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)


@pytest.mark.parametrize("C", [1, 2, 3, 4, 5, 6, 7, 8])
def test_every_channel_count_through_ramps(C):
    """37 objects: a full group of 32, then 5 (a ragged batch at 8, 4 and 2 objects per batch).  Steps of 1, 2, 1, 1 buffers: a
    set without a ramp; one whose ramp of 700 ends inside the two-buffer step; one whose step lies wholly inside its ramp; a set
    of gains only that lands during that delay ramp."""
    n_obj, max_delay, R = 37, 1400, 700
    rng = np.random.default_rng(100 + C)
    eng = make_engine(n_obj, 5, C)
    model = Model(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        d = rng.uniform(0, max_delay, (C, n_obj))
        d[0, :4] = [0.0, 1.0, 513.25, 1400.0]
        d[C - 1, 33:37] = [1400.0, 513.25, 1.0, 0.0]                 # (and in the ragged batch of the last channel)
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), d)
        step_and_mix(eng, model, 1, "no ramp")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(600, max_delay, (C, n_obj)))
        step_and_mix(eng, model, 2, "the ramp ends inside the step")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, 50, (C, n_obj)))
        step_and_mix(eng, model, 1, "the step inside the ramp")
        set_both(eng, model, signed(rng, 0.1, 2.0, (C, n_obj)))
        step_and_mix(eng, model, 1, "gains only, during the delay ramp")
    finally:
        eng.close()


@pytest.mark.parametrize("C", [1, 2, 4, 5])
def test_steady_path_with_real_delays_at_every_batch_width(C):
    """R = 0: every full batch takes the steady path (8, 4, 2 and 1 objects per batch).  70 objects: groups of 32, 32 and 6, so
    stage 2 adds three groups.  The edges of the split of t - d are planted in every channel."""
    n_obj, max_delay = 70, 1400
    assert np.float32(1.0 - 2.0 ** -30) == 1.0            # the fraction 2^-30: v = x0 + 1.0f * (x1 - x0), which is not x1
    edges = np.array([0.0, 1.0, max_delay, 36.5, np.nextafter(np.float32(37), np.float32(0)), np.nextafter(np.float32(37), np.float32(99)),
                      2.0 ** -30, 700.75, np.nextafter(np.float32(max_delay), np.float32(0))], dtype=np.float32)
    assert edges[4] < 37 < edges[5] and edges[7] > B      # (700.75: longer than the first step)
    rng = np.random.default_rng(200 + C)
    eng = make_engine(n_obj, 3, 20 + C)
    model = Model(C, n_obj, max_delay, 0)
    try:
        eng.scene_mix_enable(C, max_delay, 0)
        d = rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32)
        for c in range(C):
            at = (np.arange(edges.size) * 7 + 5 * c) % n_obj         # full batches of all three groups, and the ragged end
            d[c, at] = edges
        d[C - 1, 64:70] = edges[[6, 4, 0, 5, 2, 3]]
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), d)
        step_and_mix(eng, model, 1, "first step")
        step_and_mix(eng, model, 2, "second step")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), np.roll(d, 3, axis=1))     # at once (R = 0)
        step_and_mix(eng, model, 1, "new values at once")
    finally:
        eng.close()


@pytest.mark.parametrize("R", [1, 2, 64, 65, 66, 513, 514])
def test_where_a_ramp_ends_relative_to_a_tile(R):
    """9 objects at C = 2: batches of 4, 4 and 1.  In the step at which a set takes effect the tile that starts at local sample
    64 m has k = 64 m + 1 at its first sample: R = 65 turns the steady condition exactly at a tile's start, 64 and 66 on either
    side of it; R = 513 ends the ramp at the step's last sample, 514 at the next step's first."""
    n_obj, C, max_delay = 9, 2, 300
    rng = np.random.default_rng(300 + R)
    eng = make_engine(n_obj, 3, 40)
    model = Model(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)))
        step_and_mix(eng, model, 1, "no ramp")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)))
        step_and_mix(eng, model, 1, "the ramp's step")
        step_and_mix(eng, model, 1, "the step after")
    finally:
        eng.close()


def test_max_delay_zero():
    """a history of one sample that is never read: C = 3, 33 objects (a group of one), one set with a ramp"""
    n_obj, C, R = 33, 3, 300
    rng = np.random.default_rng(7)
    eng = make_engine(n_obj, 3, 50)
    model = Model(C, n_obj, 0, R)
    try:
        eng.scene_mix_enable(C, 0, R)
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), np.zeros((C, n_obj)))
        step_and_mix(eng, model, 1, "no ramp")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), np.zeros((C, n_obj)))
        step_and_mix(eng, model, 2, "ramp")
    finally:
        eng.close()


def test_one_object_one_channel():
    """a batch of 8 that holds one object: the ragged path alone"""
    eng = make_engine(1, 2, 60)
    model = Model(1, 1, 100, 0)
    try:
        eng.scene_mix_enable(1, 100, 0)
        set_both(eng, model, [[-0.7]], [[37.3]])
        step_and_mix(eng, model, 1, "first step")
        step_and_mix(eng, model, 1, "second step")
    finally:
        eng.close()


def test_silence_before_a_set_and_reset():
    n_obj, C, max_delay, R = 9, 2, 200, 100
    rng = np.random.default_rng(8)
    eng = make_engine(n_obj, 6, 70)
    model = Model(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        step_and_mix(eng, model, 1, "before any set", silent=True)
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)))                      # gains only: the delays stay 0, no ramp
        step_and_mix(eng, model, 1, "gains-only first set")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)))
        step_and_mix(eng, model, 1, "ramp to delays")
        step_and_mix(eng, model, 1, "at the targets")
        eng.scene_mix_reset()
        model.reset()
        step_and_mix(eng, model, 1, "after the reset: the values kept, the history silent")
        set_both(eng, model, signed(rng, 0.1, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)))
        step_and_mix(eng, model, 1, "the first set after the reset: no ramp")
    finally:
        eng.close()


def test_subnormal_products_and_sums_are_kept():
    """gains near 2^-120 on the engine's rows of a quiet scene (the audio is linear in the force: scaled to a peak near 1e-4):
    every product and every sum lies below the smallest normal f32, which the reference keeps -- so must the kernel"""
    n_obj, C, max_delay = 5, 2, 64
    rng = np.random.default_rng(9)
    g = signed(rng, 1.0, 2.0, (C, n_obj)) * 2.0 ** -120
    d = rng.uniform(0, max_delay, (C, n_obj))

    def run(force):
        eng = make_engine(n_obj, 2, 80, force=force)
        model = Model(C, n_obj, max_delay, 0)
        try:
            eng.scene_mix_enable(C, max_delay, 0)
            set_both(eng, model, g, d)
            eng.step(2)
            eng.scene_mix()
            rows = eng.audio()
            return rows, eng.read_scene_mix(), model.mix(rows)
        finally:
            eng.close()

    loud = float(np.abs(run(1e-3)[0]).max())
    rows, got, want = run(1e-3 * 1e-4 / loud)
    print(f"\nsubnormal: peak of the rows at force 1e-3 {loud:.3e}, scaled {np.abs(rows).max():.3e}, of the mix {np.abs(want).max():.3e}")
    assert 1e-5 < np.abs(rows).max() < 1e-3               # (so 5 terms of at most 2^-119 * 1e-3 stay below 2^-126)
    small = (want != 0) & (np.abs(want) < np.finfo(np.float32).tiny)
    assert small.any() and small.sum() == (want != 0).sum()
    same_bits(got, want, "subnormal")


def test_many_groups():
    """1024 objects: stage 2 adds 32 groups, the workgroups of a larger grid are renumbered over the XCDs.  Steps of 4, 4 and 5
    buffers; the second set ramps over 4410 samples, which end inside the third step.  A seeded sample of each step is compared,
    with the step's first and last 40 samples and the six samples around the ramp's end."""
    n_obj, C, max_delay, R = 1024, 2, 2048, 4410
    rng = np.random.default_rng(10)
    eng = make_engine(n_obj, 13, 90)
    model = Model(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        t0 = 0
        for k, nb in enumerate((4, 4, 5)):
            if k < 2:
                set_both(eng, model, signed(rng, 0.05, 1.0, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj)))
            n = nb * B
            pick = [rng.choice(n, 2000, replace=False), np.arange(40), np.arange(n - 40, n)]
            end = 4 * B + R - 1 - t0                                 # the local sample with k = R
            if 3 <= end < n - 3:
                pick.append(np.arange(end - 3, end + 3))
            assert k < 2 or len(pick) == 4
            step_and_mix(eng, model, nb, f"step {k}", samples=np.unique(np.concatenate(pick)))
            t0 += n
    finally:
        eng.close()
