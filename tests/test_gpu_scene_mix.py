"""The scene mix (include/openpbso_amd.h "scene mix"; kernels_mix.hip): C output channels, a ramped gain and a fractional delay
per (channel, object), a history of every object's recent samples on the device.  Checked against pbso_mix_objects (unity gains
and no delay: bit for bit), against an fp64 model of the stated semantics over consecutive steps, under three cuts of the same
samples (bit for bit), at the headline size, for no effect on the engine's own output, and along its error paths."""
import numpy as np
import pytest

from openpbso_amd import Engine, ForceMessage, capi, synth
from openpbso_amd.solver import PbsoError

B = 513


def test_scene_mix_entry_points_are_bound():
    lib = capi.lib()
    for name in ("pbso_scene_mix_enable", "pbso_scene_mix_set", "pbso_scene_mix", "pbso_read_scene_mix", "pbso_scene_mix_reset",
                 "pbso_group_scene_mix_enable", "pbso_group_scene_mix_set"):
        assert name in capi.EXPORTS and getattr(lib, name)
    assert capi.GATHER_SCENE == 4 and capi.ABI_VERSION == 6 == lib.pbso_abi_version()


def make_engine(n_obj, n_modes, nb_total, seed, hits_per_obj=3, **kw):
    """n_obj objects with explicit-data impulses at buffer 0 and spread over nb_total buffers, unit transfer"""
    eng = Engine(**kw)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 7000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, nb_total, hits_per_obj - 1)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


class Model:
    """fp64 model of the semantics in include/openpbso_amd.h: parameters (from, to, t_set) per (channel, object), ramps per
    absolute sample, linear interpolation at t - d, the object sum in exact arithmetic (as far as fp64 goes)"""

    def __init__(self, n_channels, n_obj, max_delay, ramp):
        self.C, self.N, self.R = n_channels, n_obj, ramp
        self.p = np.zeros((2, n_channels, n_obj, 3))      # gain / delay: from, to, t_set
        self.any = False
        self.t = 0
        self.L = max_delay + 2
        self.tail = np.zeros((n_obj, self.L), dtype=np.float32)     # x(t - L) .. x(t - 1)

    def _at(self, kind, t):
        f, to, ts = (self.p[kind, ..., j][..., None] for j in range(3))
        k = np.asarray(t, dtype=np.float64)[None, None, :] - ts + 1
        return np.broadcast_to(to, k.shape) if self.R == 0 else np.where(k >= self.R, to, f + (to - f) * k / self.R)

    def set(self, gain, delay=None):
        for kind, v in ((0, gain), (1, delay)):
            if v is None:
                continue
            v = np.asarray(v, dtype=np.float32).astype(np.float64).reshape(self.C, self.N)
            self.p[kind, ..., 0] = self._at(kind, [self.t - 1])[..., 0] if self.any else v
            self.p[kind, ..., 1] = v
            self.p[kind, ..., 2] = self.t
        self.any = True

    def mix(self, rows):
        """rows [N][n] float32 of the next step -> (out [C][n] fp64, bound [C] = sum_o max|g_co| max|x_o|)"""
        n = rows.shape[1]
        xx = np.concatenate([self.tail, rows], axis=1)       # xx[:, L + j] = x(t0 + j)
        t = np.arange(self.t, self.t + n)
        g_all, d_all = self._at(0, t), self._at(1, t)
        out, bound = np.zeros((self.C, n)), np.zeros(self.C)
        xmax = np.abs(xx).max(axis=1).astype(np.float64)
        for o0 in range(0, self.N, 64):
            o1 = min(self.N, o0 + 64)
            xs = xx[o0:o1].astype(np.float64)
            for c in range(self.C):
                g, d = g_all[c, o0:o1], d_all[c, o0:o1]
                pos = t[None, :] - d
                i0 = np.floor(pos)
                f = pos - i0
                j0 = (i0 - self.t + self.L).astype(np.int64)
                x0 = np.take_along_axis(xs, j0, 1)
                x1 = np.take_along_axis(xs, np.minimum(j0 + 1, xs.shape[1] - 1), 1)
                out[c] += (g * (x0 + f * (x1 - x0))).sum(axis=0)
                bound[c] += (np.abs(g).max(axis=1) * xmax[o0:o1]).sum()
        self.tail = xx[:, -self.L:]
        self.t += n
        return out, bound


def _check(got, want, bound, label):
    assert got.shape == want.shape, label
    err = np.abs(got.astype(np.float64) - want).max(axis=1)
    assert (err <= 1e-5 * bound).all(), (label, err, bound)


@pytest.mark.gpu
@pytest.mark.parametrize("n_obj", [1, 33, 1024])
@pytest.mark.parametrize("nb", [3, 4])
def test_unity_scene_mix_equals_the_object_mix_bit_for_bit(n_obj, nb):
    """C = 1, every gain 1, every delay 0: the same sum in the same order as pbso_mix_objects (groups of 32 objects, then the
    groups) -- ragged last groups, odd and even buffer counts (mix_objects' 8-byte loads and its scalar path)"""
    import torch
    eng = make_engine(n_obj, 64, 2 * nb, n_obj + nb)
    try:
        eng.scene_mix_enable(1, 8, 0)
        eng.scene_mix_set(np.ones((1, n_obj)), np.zeros((1, n_obj)))
        mono = torch.zeros(nb * B, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        for k in range(2):
            eng.step(nb)
            eng.scene_mix()
            eng.mix_objects(mono.data_ptr())
            eng.sync()
            got = eng.read_scene_mix()
            want = mono.cpu().numpy()
            assert got.shape == (1, nb * B) and np.abs(want).max() > 0
            assert np.array_equal(got[0], want), (k, np.abs(got[0] - want).max())
    finally:
        eng.close()


@pytest.mark.gpu
def test_scene_mix_against_the_model_over_steps():
    """three channels, 40 objects (a ragged second group), five steps: negative gains, fractional delays, delays longer than a
    one-buffer step (the history of two steps back), ramps that cross step boundaries, a set during a ramp, a set of gains only"""
    n_obj, C, max_delay, R = 40, 3, 1400, 700
    steps = [2, 1, 1, 3, 2]
    eng = make_engine(n_obj, 96, sum(steps), 11)
    model = Model(C, n_obj, max_delay, R)
    rng = np.random.default_rng(5)
    sets = {0: (rng.uniform(-1.5, 1.5, (C, n_obj)), rng.uniform(0, max_delay, (C, n_obj))),
            1: (rng.uniform(-1, 1, (C, n_obj)), rng.uniform(600, max_delay, (C, n_obj))),     # ramps across the next steps
            2: (rng.uniform(-1, 1, (C, n_obj)), rng.uniform(0, 50, (C, n_obj))),              # during the ramp of step 1's set
            3: (rng.uniform(-2, 2, (C, n_obj)), None)}
    sets[0][1][0, :4] = [0.0, 1.0, 513.25, 1400.0]                                           # integral, and a delay of max_delay
    try:
        eng.scene_mix_enable(C, max_delay, R)
        for k, nb in enumerate(steps):
            if k in sets:
                g, d = (None if a is None else a.astype(np.float32) for a in sets[k])
                eng.scene_mix_set(g, d)
                model.set(g, d)
            eng.step(nb)
            eng.scene_mix()
            rows = eng.audio()
            got = eng.read_scene_mix()
            want, bound = model.mix(rows)
            assert np.abs(want).max() > 0
            _check(got, want, bound, f"step {k}")
    finally:
        eng.close()


def _cut_run(cuts, n_obj, seed):
    """the same scene stepped in `cuts` after a common first step; the set calls at samples 0 and 2 * 513 in every run"""
    eng = make_engine(n_obj, 64, 2 + sum(cuts), seed, time_chunks=1)      # time_chunks = 1: the rows themselves do not depend on the cut
    rng = np.random.default_rng(seed)
    C = 2
    try:
        eng.scene_mix_enable(C, 900, 1500)
        eng.scene_mix_set(rng.uniform(-1, 1, (C, n_obj)), rng.uniform(0, 900, (C, n_obj)))
        eng.step(2)
        eng.scene_mix()
        first = eng.read_scene_mix()
        eng.scene_mix_set(rng.uniform(-1, 1, (C, n_obj)), rng.uniform(0, 900, (C, n_obj)))     # a ramp over 1500 samples
        mixes, rows = [first], []
        for nb in cuts:
            eng.step(nb)
            eng.scene_mix()
            mixes.append(eng.read_scene_mix())
            rows.append(eng.audio())
        return np.concatenate(mixes, axis=1), np.concatenate(rows, axis=1)
    finally:
        eng.close()


@pytest.mark.gpu
def test_scene_mix_does_not_depend_on_the_cut_into_steps():
    """1 x 8, 2 x 4 and 4 x 2 buffers after the same first step: bit-identical mixes (every per-sample quantity comes from the
    absolute sample; a tile where the ramps have ended in one cut is in the middle of them in another)"""
    k = 4
    base_mix, base_rows = _cut_run([2 * k], 37, 3)
    assert np.abs(base_mix).max() > 0
    for cuts in ([k, k], [2] * k):
        mix, rows = _cut_run(cuts, 37, 3)
        assert np.array_equal(rows, base_rows), cuts                 # (the precondition: the same rows)
        assert np.array_equal(mix, base_mix), (cuts, np.abs(mix - base_mix).max())


@pytest.mark.gpu
def test_scene_mix_at_the_headline_size():
    """1024 objects x 512 modes x 86 buffers, stereo, against the model over two steps (the second one ramps to new values)"""
    n_obj, M, nb, C, max_delay, R = 1024, 512, 86, 2, 2048, 4410
    eng = make_engine(n_obj, M, 2 * nb, 17, hits_per_obj=2)
    model = Model(C, n_obj, max_delay, R)
    rng = np.random.default_rng(17)
    try:
        eng.scene_mix_enable(C, max_delay, R)
        for k in range(2):
            g = rng.uniform(-1, 1, (C, n_obj)).astype(np.float32)
            d = rng.uniform(0, max_delay, (C, n_obj)).astype(np.float32)
            eng.scene_mix_set(g, d)
            model.set(g, d)
            eng.step(nb)
            eng.scene_mix()
            rows = eng.audio()
            got = eng.read_scene_mix()
            want, bound = model.mix(rows)
            assert np.abs(want).max() > 0
            _check(got, want, bound, f"step {k}")
    finally:
        eng.close()


@pytest.mark.gpu
def test_scene_mix_leaves_the_engines_output_alone():
    """with the mixer enabled and mixing every step, pbso_read_audio and pbso_mix_objects are bit-identical to an engine without it"""
    import torch
    n_obj, nb = 70, 5
    plain = make_engine(n_obj, 128, 3 * nb, 23)
    mixed = make_engine(n_obj, 128, 3 * nb, 23)
    mono = torch.zeros((2, nb * B), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rng = np.random.default_rng(2)
    try:
        mixed.scene_mix_enable(2, 700, 300)
        for k in range(3):
            mixed.scene_mix_set(rng.uniform(-1, 1, (2, n_obj)), rng.uniform(0, 700, (2, n_obj)))
            plain.step(nb)
            mixed.step(nb)
            mixed.scene_mix()
            plain.mix_objects(mono[0].data_ptr())
            mixed.mix_objects(mono[1].data_ptr())
            plain.sync()
            mixed.sync()
            a, b = plain.audio(), mixed.audio()
            assert np.abs(a).max() > 0 and np.array_equal(a, b), k
            m = mono.cpu().numpy()
            assert np.array_equal(m[0], m[1]), k
            assert np.abs(mixed.read_scene_mix()).max() > 0
    finally:
        plain.close()
        mixed.close()


@pytest.mark.gpu
def test_scene_mix_error_paths():
    n_obj = 3
    eng = Engine()
    try:
        for i in range(n_obj):
            eng.add_object(synth.eigenvalues(32, 40 + i), synth.RHO, synth.ALPHA, synth.BETA)
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix_enable(2, 10, 0)                   # before finalize
        assert ei.value.status == capi.ERR_STATE
        eng.finalize()
        for i in range(n_obj):
            eng.set_use_transfer(i, False)
            eng.enqueue_force(i, ForceMessage(data=np.ones(32) * 1e-3), 0)
        for bad in ((0, 10, 0), (9, 10, 0), (2, -1, 0), (2, (1 << 20) + 1, 0), (2, 10, (1 << 20) + 1)):
            with pytest.raises(PbsoError) as ei:
                eng.scene_mix_enable(*bad)
            assert ei.value.status == capi.ERR_INVALID, bad
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix()                                  # not enabled
        assert ei.value.status == capi.ERR_STATE
        eng.scene_mix_enable(2, 10, 4)
        g, d = np.ones((2, n_obj)), np.full((2, n_obj), 3.5)
        for gg, dd in ((g, d + 7), (g, -d), (np.where(np.eye(2, n_obj) > 0, np.nan, g), d), (g, np.where(np.eye(2, n_obj) > 0, np.nan, d)),
                       (np.where(np.eye(2, n_obj) > 0, np.inf, g), None)):
            with pytest.raises(PbsoError) as ei:
                eng.scene_mix_set(gg, dd)                    # a delay above max_delay, negative, NaN; a NaN / infinite gain
            assert ei.value.status == capi.ERR_INVALID
        eng.scene_mix_set(g, d)
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix()                                  # no step since enable
        assert ei.value.status == capi.ERR_STATE
        eng.step(1)
        eng.scene_mix()
        first = eng.read_scene_mix()
        assert first.shape == (2, B) and np.abs(first).max() > 0
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix()                                  # the same step twice
        assert ei.value.status == capi.ERR_STATE
        eng.step(1)
        eng.step(1)
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix()                                  # a step was not mixed
        assert ei.value.status == capi.ERR_STATE
        eng.scene_mix_reset()
        eng.step(2)
        eng.scene_mix()                                      # works again
        assert eng.read_scene_mix().shape == (2, 2 * B)
        # rows of a step to host memory are not on the device
        host = eng.host_buffer(1)
        eng.step_to_host(1, host)
        eng.host_wait()
        with pytest.raises(PbsoError) as ei:
            eng.scene_mix()
        assert ei.value.status == capi.ERR_STATE
        eng.scene_mix_reset()
        eng.step(1)
        eng.scene_mix()
        assert np.isfinite(eng.read_scene_mix()).all()
    finally:
        eng.close()
