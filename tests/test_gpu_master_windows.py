"""The master bus's sliding minimum, gain launches and PCM on the device at the borders kernels_master.hip is built around: every
case of tests/master_window_plan.py (every level count k = 1 .. 16, every count of passes over the whole array, D = 0, 1, 2^k - 1
and in mid range, both gain launches, peaks that enter and leave on the borders of strips and steps), the two gain launches on
either side of their threshold, the first look-ahead whose chain over the taps ends below 1.f, magnitudes whose ratios and products
are subnormal, a gain ramp through zero and every tie of the 16-bit conversion.  Every step's output and meters are compared BIT
FOR BIT with tests/master_model.py (sumsq to the bar tests/test_gpu_master.py derives); tests/test_master_window_plan.py proves
without a GPU what the plan reaches."""
import numpy as np
import pytest
import torch                      # before the engine's library (as in test_gpu_eq.py)

from openpbso_amd import Engine, ForceMessage, synth
from tests import master_window_plan as wp
from tests.master_model import Model, pcm16

pytestmark = pytest.mark.gpu
B = 513
CASES = wp.cases()


def make_engine(n_obj=1, n_modes=64, nb_total=4, seed=1, **kw):
    eng = Engine(**kw)
    for i in range(n_obj):
        eng.add_object(synth.eigenvalues(n_modes, 9000 + 131 * seed + i), synth.RHO, synth.ALPHA, synth.BETA)
    eng.finalize()
    rng = np.random.default_rng(seed)
    for i in range(n_obj):
        eng.set_use_transfer(i, False)
        for t in [0] + sorted(int(x) for x in rng.integers(1, max(nb_total, 2), 2)):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n_modes) * 1e-3), t)
    return eng


def device(a):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()
    torch.cuda.synchronize()
    return t


def same_bits(got, want, label):
    assert got.shape == want.shape, label
    bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
    assert bad.size == 0, (label, bad.size, bad[:4], got.ravel()[bad[:4]], want.ravel()[bad[:4]])


def same_meters(got, want, label):
    for f in ("in_peak", "out_peak", "min_gain"):
        same_bits(np.ascontiguousarray(got[f]), np.ascontiguousarray(want[f]), (label, f))
    assert np.array_equal(got["n_limited"], want["n_limited"]), label
    # (tests/test_gpu_master.py: any two orders of at most 513 non-negative fp64 terms differ by at most 1.2e-13 relative)
    assert (np.abs(got["sumsq"] - want["sumsq"]) <= 1e-12 * want["sumsq"]).all(), label


def run(eng, model, x, cuts, label, frames=B):
    """x [C][n] through the engine and the model in steps of cuts[i] buffers; every step's output and meters compared.  Returns the
    concatenated output and the meters of all the steps"""
    outs, meters, at = [], [], 0
    for k, nb in enumerate(cuts):
        part = x[:, at * frames:(at + nb) * frames]
        dx = device(part)
        eng.step(nb)
        eng.master(dx.data_ptr())
        got = eng.read_master()
        same_bits(got, model.process(part), (label, k, nb))
        m = eng.read_master_meters()
        same_meters(m, model.meters, (label, k, nb))
        outs.append(got)
        meters.append(m)
        at += nb
    assert at * frames == x.shape[1]
    return np.concatenate(outs, axis=1), np.concatenate(meters, axis=0)


@pytest.mark.parametrize("case", CASES, ids=[c["name"].replace(" ", "_") for c in CASES])
def test_window_case(case):
    """one case of the plan on its staircase: a single step (the wide gain launch from 16384 samples on) and the uneven steps of at
    most 31 buffers (narrow launches, the history carried from step to step), each against the model, and against each other"""
    x, lay = wp.staircase(case)
    Cn, L, H = case["C"], case["L"], case["H"]
    outs = []
    eng = make_engine()
    try:
        for cut in wp.cuts(lay["n"] // B):
            eng.master_enable(Cn, wp.T, L, H, 0)         # (a second enable is a fresh bus: silence for a history, t = 0)
            w = eng.master_window()
            y, meters = run(eng, Model(Cn, wp.T, L, H, 0, w), x, cut, (case["name"], len(cut)))
            assert np.abs(y).max() <= np.float32(wp.T)
            assert meters["n_limited"][:, 0].sum() >= 8 and meters["min_gain"].min() < 1       # (eight peaks)
            outs.append(y)
    finally:
        eng.close()
    same_bits(outs[1], outs[0], (case["name"], "the uneven steps against the single step"))


@pytest.mark.parametrize("W", [2, 3, 5, 64, 1023, 1024, 1025, 2048, 4097, 8192, 32768, 65537])
def test_the_reach_of_one_peak(W):
    """L = 1, so g = a: a peak at sample s holds g below 1 at the outputs s .. s + 2 L + H - 1 and at no others.  Stated without
    the model: outside the reaches the output is the input one sample late, bit for bit; n_limited sums to peaks x (2 L + H).
    The windows: the plan's L = 1 shapes at no pass over the whole array and at 1, 2, 3, 5 and 6 of them"""
    L, H, Cn = 1, W - 2, 3
    HL = 2 * L + H
    at = [7 + i * (HL + 19) for i in range(5)]
    at[2] = -(-at[2] // B) * B - 1                       # one peak on the last sample of a buffer (its reach begins a buffer's end)
    at[3:] = [at[2] + (i + 1) * (HL + 19) for i in range(2)]
    nb = -(-(at[-1] + HL + 2) // B)
    n = nb * B
    rng = np.random.default_rng(W)
    x = (rng.standard_normal((Cn, n)) * wp.NOISE).astype(np.float32)
    for i, s in enumerate(at):
        x[i % Cn, s] = (-1) ** i * (1.5 + i)
    assert all(b - a > HL for a, b in zip(at, at[1:])) and at[-1] + HL <= n        # the reaches do not overlap and all end inside
    clear = np.ones(n, dtype=bool)
    for s in at:
        clear[s:s + HL] = False
    cut = [nb] if nb < 3 else [1, nb - 2, 1]
    eng = make_engine()
    try:
        eng.master_enable(Cn, wp.T, L, H, 0)
        model = Model(Cn, wp.T, L, H, 0, eng.master_window())
        y, meters = run(eng, model, x, cut, ("reach", W))
    finally:
        eng.close()
    delayed = np.concatenate([np.zeros((Cn, L), dtype=np.float32), x[:, :-L]], axis=1)
    same_bits(np.ascontiguousarray(y[:, clear]), np.ascontiguousarray(delayed[:, clear]), ("outside the reaches", W))
    assert (np.abs(y[:, ~clear]) <= np.float32(wp.T)).all()
    for s in at:                                         # inside a reach the peak's own channel is scaled down: never the input
        assert abs(y[at.index(s) % Cn, s + L]) <= np.float32(wp.T) < abs(x[at.index(s) % Cn, s])
    assert (meters["n_limited"].sum(axis=0) == len(at) * HL).all()
    assert np.array_equal(meters["n_limited"][:, 0], (~clear).reshape(nb, B).sum(axis=1))


def test_the_gain_launches_on_either_side_of_their_border():
    """buffers of 27 samples, L = 200, H = 37, two channels, dense noise: a step of 606 buffers is 16362 samples, the narrow launch
    with 256 strips of 64, the last one of 42 samples; a step of 607 is 16389, the wide launch, whose seventeenth strip of 1024 has
    five.  A one-buffer step behind each reads the history that launch's step left"""
    frames, L, H, Cn = 27, 200, 37, 2
    assert wp.classes(L, H, 606 * frames) == dict(wp.classes(L, H, 606 * frames), wide=False, gain_strips=256, ragged=True)
    assert wp.classes(L, H, 607 * frames) == dict(wp.classes(L, H, 607 * frames), wide=True, gain_strips=17, ragged=True)
    assert 606 * frames == 255 * 64 + 42 and 607 * frames == 16 * 1024 + 5
    rng = np.random.default_rng(606)
    for nb in (606, 607):
        x = rng.standard_normal((Cn, (nb + 1) * frames)).astype(np.float32)
        eng = make_engine(frames_per_buffer=frames)
        try:
            eng.master_enable(Cn, wp.T, L, H, 0)
            model = Model(Cn, wp.T, L, H, 0, eng.master_window(), frames=frames)
            y, meters = run(eng, model, x, [nb, 1], ("border", nb), frames)
            assert np.abs(y).max() <= np.float32(wp.T) and meters["n_limited"][-1].min() > 0
        finally:
            eng.close()


@pytest.mark.parametrize("L", [12, 13])
def test_the_chain_over_the_taps_ending_below_and_at_one(L):
    """T = 1, |u| < 1 but for one peak: away from the peak's reach the output is the delayed input times the end value of the f32
    chain over the taps, bit for bit.  L = 12 is the first look-ahead where that value is below 1.f (include/openpbso_amd.h): every
    sample counts as limited.  At L = 13 it is above 1.f and the fminf with r = 1 takes it back"""
    rng = np.random.default_rng(L)
    n, s = 3 * B, 700
    x = rng.uniform(-0.999, 0.999, (1, n)).astype(np.float32)
    x[0, s] = 3.0
    eng = make_engine()
    try:
        eng.master_enable(1, 1.0, L, 0, 0)
        w = eng.master_window()
        y, meters = run(eng, Model(1, 1.0, L, 0, 0, w), x, [1, 2], ("chain end", L))
    finally:
        eng.close()
    end = np.float32(0)
    for k in range(L - 1, -1, -1):
        end = np.float32(w[k] + end)                     # fmaf(w[k], 1.f, acc) is one rounded addition
    assert (end < 1) == (L == 12) and 1 - 2.3e-6 <= end
    g = min(end, np.float32(1))
    clear = np.ones(n, dtype=bool)
    clear[s:s + 2 * L] = False
    delayed = np.concatenate([np.zeros((1, L), dtype=np.float32), x[:, :-L]], axis=1)
    same_bits(np.ascontiguousarray(y[:, clear]), np.ascontiguousarray((delayed * g)[:, clear]), ("away from the peak", L))
    lim = meters["n_limited"][:, 0].tolist()
    assert lim == [B, B, B] if L == 12 else (lim[0] == lim[2] == 0 < lim[1] <= 2 * L)
    assert meters["min_gain"][0, 0] == g


@pytest.mark.parametrize("T,peaks,scale", [(0.7, (1e30, 3e38, -3.4028235e38), 0.05), (2.0 ** -126, (), 1.0), (1e-40, (), 1.0)],
                         ids=["huge-peaks", "T=2^-126", "T=1e-40"])
def test_extreme_magnitudes(T, peaks, scale):
    """no denormal flag and a correctly rounded division (the header comment of kernels_master.hip): peaks up to FLT_MAX give a
    subnormal r = T / pk; under a ceiling of 2^-126 or of a subnormal every r and every product of the chain is subnormal or zero"""
    L, H, Cn = 64, 32, 2
    rng = np.random.default_rng(len(peaks))
    x = (rng.standard_normal((Cn, 2 * B)) * scale).astype(np.float32)
    for i, p in enumerate(peaks):
        x[i % Cn, 100 + 300 * i] = p
    r = wp.ratios(x, T)
    tiny = np.float32(2.0 ** -126)
    if peaks:
        assert ((r > 0) & (r < tiny)).sum() == 2 and np.isfinite(x).all()      # 0.7 / 3e38 and 0.7 / FLT_MAX are subnormal
    else:
        assert (r < tiny).mean() > 0.3 and (r < 1e-30).all() and (r > 0).any()      # (2^-126 / pk is subnormal where pk > 1)
    eng = make_engine()
    try:
        eng.master_enable(Cn, T, L, H, 0)
        y, meters = run(eng, Model(Cn, T, L, H, 0, eng.master_window()), x, [1, 1], ("extreme", T))
    finally:
        eng.close()
    assert not np.isnan(y).any() and np.abs(y).max() <= np.float32(T)
    if peaks:
        assert meters["n_limited"].max() > 0 and 0 < meters["min_gain"].min() < tiny
    else:
        assert meters["n_limited"].min() == B and meters["min_gain"].max() < tiny


def test_a_gain_ramp_through_zero_keeps_the_signs_of_its_zeros():
    """R = 700: 3.0, then -2.0 inside that ramp (the gain passes zero), then 0.0; steps of one buffer until 0.0 is in force and one
    more.  0 * u keeps u's sign and (-p) * u flips it: the zeros of the output are compared with their signs, by bits"""
    Cn, L, R = 2, 64, 700
    rng = np.random.default_rng(70)
    x = rng.standard_normal((Cn, 8 * B)).astype(np.float32) * np.float32(0.4)
    x[0, 2 * B + 5], x[1, 2 * B + 6] = 0.0, -0.0
    eng = make_engine(nb_total=9)
    outs = []
    try:
        eng.master_enable(Cn, 0.7, L, 0, R)
        model = Model(Cn, 0.7, L, 0, R, eng.master_window())
        k = 0

        def step():
            nonlocal k
            outs.append(run(eng, model, x[:, k * B:(k + 1) * B], [1], ("through zero", k))[0])
            assert eng.master_info()["ramp_end"] == model.ramp_end() and eng.master_info()["t"] == model.t
            k += 1

        for gain in (3.0, -2.0, 0.0):
            eng.master_set_gain(gain)
            model.set_gain(gain)
            if gain == -2.0:                             # from above zero to below it inside this step
                p = model._p(model.t + np.arange(B))
                assert p[0] > 0 > p[-1]
            step()
            assert model.ramp_end() > model.t             # 513 < 700: the next set falls inside this ramp
        while model.ramp_end() > model.t:
            step()
        step()                                           # a whole buffer at 0.0
        assert k <= 8 and eng.master_info()["sets"] == 3
    finally:
        eng.close()
    y = np.concatenate(outs, axis=1)
    last = y[:, -B + L:]                                 # behind the look-ahead's delay the last buffer is 0.f * u: u's sign
    assert (last == 0).all() and np.signbit(last).any() and not np.signbit(last).all()
    assert np.array_equal(np.signbit(last), np.signbit(x[:, (k - 1) * B:k * B - L]))


def test_pcm16_at_every_tie():
    """T = 1, L = 1, H = 0: an input with |x| < 1 comes out one sample late, bit for bit.  x = (float)((k + 0.5) / 32767) for every
    k = 0 .. 32766 with alternating sign: on the host every f32 product x * 32767.f lands exactly on k + 0.5 (asserted below before
    anything is trusted), so the conversion has a tie at every sample, 16384 with an even k and 16383 with an odd one; then +-1
    exactly, and values beyond +-1, which the ceiling brings back to +-1"""
    nb = 64
    n = nb * B
    k = np.arange(32767)
    x = np.full((1, n), 0.25, dtype=np.float32)
    x[0, :32767] = ((k + 0.5) / 32767.0).astype(np.float32) * np.where(k % 2 == 0, 1, -1).astype(np.float32)
    x[0, 32767:32769] = (1.0, -1.0)
    x[0, [32775, 32785, 32795, 32805]] = (1.5, -2.0, 1.0000001, -7e37)
    eng = make_engine()
    try:
        eng.master_enable(1, 1.0, 1, 0, 0)
        model = Model(1, 1.0, 1, 0, 0, eng.master_window())
        dx = device(x)
        eng.step(nb)
        eng.master(dx.data_ptr())
        want = model.process(x)
        same_bits(eng.read_master(), want, "pcm input")
        got = eng.read_master_pcm16()
    finally:
        eng.close()
    same_bits(np.ascontiguousarray(want[:, 1:32770]), np.ascontiguousarray(x[:, :32769]), "one sample late")
    prod = want[0] * np.float32(32767.0)
    tie = np.abs(prod[1:32768]) == (k + 0.5).astype(np.float32)
    assert tie[k % 2 == 0].sum() >= 16000 and tie[k % 2 == 1].sum() >= 16000
    expected = pcm16(want)
    assert np.array_equal(expected[1:32768, 0][tie], (np.where(k % 2 == 0, k, -(k + 1)))[tie])         # to the even neighbour
    assert expected[32768:32770, 0].tolist() == [32767, -32767]
    assert [int(expected[i + 1, 0]) for i in (32775, 32785, 32795, 32805)] == [32767, -32767, 32767, -32767]
    halves_up = np.floor(prod + np.float32(0.5)).astype(np.int16)          # what (int)floorf(x + 0.5f) would give
    even_ties = np.flatnonzero(tie & (k % 2 == 0)) + 1
    assert (halves_up[even_ties] != expected[even_ties, 0]).all()
    assert got.shape == expected.shape and np.array_equal(got, expected)
