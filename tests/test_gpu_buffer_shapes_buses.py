"""The buses behind the engine at buffer lengths other than 513: the scene mix, the scene filter mix with its delay stage, the
scene reverb and the master bus at 27 and 864 frames, in steps of 1 and 3 buffers, each against its existing C reference, BIT FOR
BIT.  The references work on sample streams (the rows Engine.audio() returned, or a given input): only the step lengths, the
master's per-buffer meters and the read-backs know the buffer length.  A 27-sample step is shorter than a FIR strip, a reverb
piece and every history here: that is the edge.  And one loopback device group at 270 frames against the single engine."""
import numpy as np
import pytest
import torch                      # before the engine's library: loaded second, torch brings a HIP runtime of its own and finds no device

from openpbso_amd import Engine, ForceMessage, capi, synth
from tests import master_model, scene_fir_delay_model, scene_mix_model, scene_reverb_model

pytestmark = pytest.mark.gpu
FRAMES = [27, 864]
STEPS = [1, 3, 1, 3, 3]


def make_engine(frames, n_obj, n_modes, nb_total, seed):
    """objects with explicit-data impulses at buffer 0 and two later buffers, unit transfer, the velocity form"""
    eng = Engine(form=capi.FORM_VELOCITY, frames_per_buffer=frames)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 9000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), 2)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


def same_bits(got, want, label, silent_ok=False):
    assert got.shape == want.shape, label
    assert silent_ok or np.abs(want).max() > 0, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def signed(rng, lo, hi, shape):
    return rng.uniform(lo, hi, shape) * rng.choice([-1.0, 1.0], shape)


@pytest.mark.parametrize("frames", FRAMES)
def test_scene_mix(frames):
    """37 objects (a ragged second group), C = 3, delays up to 1400 samples (52 buffers of 27), a ramp of 700 that crosses steps"""
    n_obj, C, max_delay, R = 37, 3, 1400, 700
    rng = np.random.default_rng(frames)
    eng = make_engine(frames, n_obj, 64, sum(STEPS), 1)
    model = scene_mix_model.Model(C, n_obj, max_delay, R)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        for k, nb in enumerate(STEPS):
            if k in (0, 1, 3):
                g = signed(rng, 0.1, 1.5, (C, n_obj)).astype(np.float32)
                d = rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32)
                d[0, :4] = [0.0, 1.0, frames + 0.25, max_delay]
                eng.scene_mix_set(g, d)
                model.set(g, d)
            eng.step(nb)
            eng.scene_mix()
            rows, got = eng.audio(), eng.read_scene_mix()
            assert got.shape == (C, nb * frames) and np.abs(rows).max(axis=1).min() > 0
            same_bits(got, model.mix(rows), (frames, k))
    finally:
        eng.close()


@pytest.mark.parametrize("frames", FRAMES)
def test_scene_filter_mix_with_its_delay_stage(frames):
    """40 objects, C = 3, K = 37, onsets up to 1400, a cross-fade of 700, delays up to 1200 with a ramp of 600: a filter set and a
    delay set in one step, a delay set during the running ramp"""
    n_obj, C, K, max_onset, xfade, max_delay, rd = 40, 3, 37, 1400, 700, 1200, 600
    rng = np.random.default_rng(100 + frames)
    eng = make_engine(frames, n_obj, 96, sum(STEPS), 2)
    model = scene_fir_delay_model.Model(C, n_obj, K, max_onset, xfade, max_delay, rd)
    taps = lambda: ((rng.standard_normal((C, n_obj, K)) * np.exp(-np.arange(K) / (K / 4.0))).astype(np.float32),
                    rng.integers(0, max_onset + 1, n_obj).astype(np.int32))
    delays = lambda: rng.uniform(0, max_delay, n_obj).astype(np.float32)
    # at 27 frames a cross-fade of 700 samples runs for 26 buffers: the second filter set comes only where it has ended
    script = {0: (taps(), delays()), 1: (None, delays()), 4: (taps() if frames > 500 else None, delays())}
    script[0][0][1][:3] = [0, max_onset, frames]                     # (object 0 is heard in the very first 27 samples)
    script[0][1][:4] = [0.0, max_delay, frames, 0.5]
    try:
        eng.scene_fir_enable(C, K, max_onset, xfade)
        eng.scene_fir_delay_enable(max_delay, rd)
        for k, nb in enumerate(STEPS):
            fs, ds = script.get(k, (None, None))
            if fs is not None:
                eng.scene_fir_set(*fs)
                model.set(*fs)
            if ds is not None:
                eng.scene_fir_set_delay(ds)
                model.set_delay(ds)
            eng.step(nb)
            eng.scene_fir()
            rows, got = eng.audio(), eng.read_scene_fir()
            assert got.shape == (C, nb * frames)
            same_bits(got, model.mix(rows), (frames, k))
            assert eng.scene_fir_delay_info() == model.info(), k
    finally:
        eng.close()


@pytest.mark.parametrize("frames", FRAMES)
def test_scene_reverb(frames):
    """n_in = n_out = 2, K = 4101 (three segments; 152 buffers of 27), a fade of 700, with and without a dry mix to add onto"""
    n_in, n_out, K, R = 2, 2, 4101, 700
    rng = np.random.default_rng(200 + frames)
    eng = make_engine(frames, 1, 64, sum(STEPS), 3)
    model = scene_reverb_model.Model(n_in, n_out, K, R)
    new = lambda: (rng.standard_normal((n_out, n_in, K)) * np.exp(-np.arange(K) / (K / 4.0))).astype(np.float32)
    try:
        eng.scene_reverb_enable(n_in, n_out, K, R)
        for k, nb in enumerate(STEPS):
            if k in (0, 1) or (k == 4 and frames > 500):             # (at 27 frames the fade of step 1 still runs at step 4)
                h = new()
                eng.scene_reverb_set(h)
                model.set(h)
            x = rng.standard_normal((n_in, nb * frames)).astype(np.float32)
            add = rng.standard_normal((n_out, nb * frames)).astype(np.float32) if k % 2 else None
            eng.step(nb)
            dx, da = device(x), None if add is None else device(add)
            eng.scene_reverb(dx.data_ptr(), None if da is None else da.data_ptr())
            got = eng.read_scene_reverb()
            assert got.shape == (n_out, nb * frames)
            same_bits(got, model.process(x, add), (frames, k))
        assert eng.scene_reverb_info()["t"] == sum(STEPS) * frames
    finally:
        eng.close()


@pytest.mark.parametrize("frames", FRAMES)
def test_master_bus(frames):
    """two channels, ceiling 0.7, look-ahead 200, hold 37, a gain ramp of 300: the output, the 16-bit PCM and the meters of every
    buffer of `frames` samples"""
    Cn, T, L, H, R = 2, 0.7, 200, 37, 300
    rng = np.random.default_rng(300 + frames)
    eng = make_engine(frames, 1, 64, sum(STEPS), 4)
    model = master_model.Model(Cn, T, L, H, R, frames=frames)
    try:
        eng.master_enable(Cn, T, L, H, R)
        for k, nb in enumerate(STEPS):
            if k in (1, 3):
                gain = float(rng.uniform(0.3, 1.6))
                eng.master_set_gain(gain)
                model.set_gain(gain)
            x = rng.standard_normal((Cn, nb * frames)).astype(np.float32)
            dx = device(x)
            eng.step(nb)
            eng.master(dx.data_ptr())
            got = eng.read_master()
            want = model.process(x)
            assert got.shape == (Cn, nb * frames)
            same_bits(got, want, (frames, k), silent_ok=sum(STEPS[:k + 1]) * frames <= L)   # (the look-ahead: the first L samples out are silence)
            assert np.array_equal(eng.read_master_pcm16(), master_model.pcm16(want)), k
            m, w = eng.read_master_meters(), model.meters
            assert m.shape == (nb, Cn) == w.shape
            for f in ("in_peak", "out_peak", "min_gain"):
                same_bits(np.ascontiguousarray(m[f]), np.ascontiguousarray(w[f]), (frames, k, f), silent_ok=f == "out_peak")
            assert np.array_equal(m["n_limited"], w["n_limited"]), k
            # (any order of `frames` non-negative fp64 terms is within frames * 2^-53 of exact)
            assert (np.abs(m["sumsq"] - w["sumsq"]) <= 1e-12 * w["sumsq"]).all(), k
        assert 0 < np.abs(got).max() <= np.float32(T)
    finally:
        eng.close()


def test_loopback_group_scene_gather_at_270_frames_equals_the_single_engine():
    """world 2, ragged shards, PBSO_GATHER_SCENE: the ranks' mixes summed in rank order equal one engine's scene mix within f32
    reassociation (the bound of tests/test_gpu_group_scene_mix.py)"""
    from openpbso_amd.group import Group
    from tests.test_gpu_group_scene_mix import _feed, _scene, _sets
    frames, world, modes, steps = 270, 2, [1100, 64, 65, 37], [3, 1, 2, 4]
    C, max_delay, R = 2, 800, 600
    lams, shapes, hits, vns = _scene(modes, sum(steps), world)
    sets = _sets(C, len(modes), max_delay, world)
    with Engine(frames_per_buffer=frames) as eng, Group([0] * world, transport=capi.GROUP_LOOPBACK, frames_per_buffer=frames) as grp:
        _feed(eng, grp, modes, lams, shapes, hits, vns)
        assert eng.info()["recurrence_form"] == capi.FORM_VELOCITY
        eng.scene_mix_enable(C, max_delay, R)
        grp.scene_mix_enable(C, max_delay, R)
        xmax = np.zeros(len(modes))
        for k, nb in enumerate(steps):
            if k in sets:
                eng.scene_mix_set(*sets[k])
                grp.scene_mix_set(*sets[k])
            eng.step(nb)
            eng.scene_mix()
            want = eng.read_scene_mix().astype(np.float64)
            rows = eng.audio()
            grp.step(nb)
            grp.gather(capi.GATHER_SCENE)
            xmax = np.maximum(xmax, np.abs(rows).max(axis=1))
            bound = np.abs(np.concatenate([s[0] for j, s in sets.items() if j <= k], axis=1)).max() * xmax.sum()
            assert np.abs(want).max() > 0
            for r in range(world):
                got = grp.result(r)
                assert got.shape == (C, nb * frames), (k, r)
                err = np.abs(got - want).max()
                print(f"step {k} rank {r}: max |group - engine| {err:.3e}, bound {1e-5 * bound:.3e}")
                assert err <= 1e-5 * bound, (k, r, err, bound)
