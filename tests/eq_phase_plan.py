"""The EQ bus's phase plans (no GPU, no engine library): runs of steps chosen so that every branch of the block form is reached.  A
cascade's time axis is cut into blocks of P samples from its t_set on (include/openpbso_amd.h "EQ bus"); what a step of n samples
has to do for a cascade depends on where it starts on that grid, k0 = (t - t_set) mod P, and where it ends, (k0 + n) mod P.
phases() walks a plan's clock by the header's rules and yields every launch of a cascade as (which, k0, n); classes() names the
cases of one launch from the block definition alone.  tests/test_eq_phase_plan.py proves the coverage and pins the model's output
of every plan; tests/test_gpu_eq_phases.py runs the plans on the device against the model, bit for bit.

A plan: frames per buffer, C channels, S sections, R cross-fade samples, cuts = the step lengths in buffers, sets = {step index:
shift}: the coefficient set coefficients(C, S, shift) of the bank is given before that step."""
import zlib

import numpy as np

from tests import eq_model as em

P = em.P
H = P + 2
RATE = 44100.0
# tests/test_gpu_eq.py's bank (that file loads the engine's library; test_gpu_eq_phases.py asserts that the two are one list)
BANK = [("highpass", 30.0, 0.707, 0.0), ("peak", 100.0, 4.0, 12.0), ("highshelf", 8000.0, 0.707, 6.0), ("highpass", 5.0, 8.0, 0.0),
        ("peak", 1000.0, 2.0, -9.0), ("lowpass", 18000.0, 0.707, 0.0), ("lowshelf", 200.0, 0.707, -6.0), ("highpass", 20.0, 2.0, 0.0),
        ("peak", 3000.0, 1.0, 3.0), ("lowpass", 9000.0, 1.2, 0.0)]
BATCH_G = (0, 1, 63, 64, 65, 127, 128, 129)


def plan(name, frames, Cn, S, R, cuts, sets):
    return dict(name=name, frames=frames, C=Cn, S=S, R=R, cuts=list(cuts), sets=dict(sets))


def _sweeps():
    out = [plan("sweep-1", 27, 2, 2, 0, [1] * 66, {0: 0}), plan("sweep-3", 27, 2, 2, 0, [3] * 66, {0: 0}),
           plan("sweep-9", 27, 2, 2, 0, [9] * 66, {0: 0}), plan("sweep-513", 513, 2, 2, 0, [1] * 66, {0: 0}),
           # once more with all the channels and sections, and with an odd S: the work rows end on the other side of the ping-pong
           plan("sweep-1 C8 S8", 27, 8, 8, 0, [1] * 66, {0: 0}), plan("sweep-1 C3 S3", 27, 3, 3, 0, [1] * 66, {0: 0})]
    return out


def _batches():
    """single-buffer steps choose k0 (t_set = 0: k0 = 27 k mod 64), then one long step, then two short ones that read what it left.
    At k0 = 0 a step of 152 buffers (4104 samples) has G = 63 and 154 (4158) too, ending at phase 62; 155 (4185) has G = 64 and 157
    (4239) G = 65; 304 (8208) G = 127 and 306 (8262) G = 128; 306 behind 7 single steps (k0 = 61) G = 129; 155 behind 18 single steps
    (k0 = 38) ends at phase 63"""
    return [plan(f"batches {lead}+{long}", 27, 2, 2, 0, [1] * lead + [long, 1, 1], {0: 0})
            for lead, long in ((0, 152), (0, 154), (0, 155), (0, 157), (18, 155), (0, 304), (0, 306), (7, 306))]


def _fades():
    """a first set at step 0 (it fades from the identity), a second one m buffers later: From is then the first set's cascade at
    k0 = 27 m mod 64 = 61, 62, 63, 0 for m = 7, 26, 45, 64, and it runs for R - 1 samples.  R = 2, 3, 4: a From of 1, 2, 3 samples;
    R = 27, 28, 29: the fade ends one sample before, on and one sample behind a step edge; R = 64, 65, 66: a fade of about a block
    over three steps.  The last three give From one long step from k0 = 61 (m = 7 and m = 71): R - 1 = 66 samples end at 127 (a
    later block's sample P - 2 is the last), 195 end at 256 and 196 at 257 (the edges of the groups of 256 positions)"""
    out = []
    for m in (7, 26, 45, 64):
        for R in (2, 3, 4, 27, 28, 29, 64, 65, 66):
            out.append(plan(f"fades m={m} R={R}", 27, 2, 2, R, [1, m - 1, 1, 1, 1, 3, 1], {0: 0, 2: 4}))
    out.append(plan("fades m=7 R=67 long", 27, 2, 2, 67, [7, 3, 1, 1], {0: 0, 1: 4}))
    out.append(plan("fades m=71 R=196 long", 27, 2, 2, 196, [9, 62, 9, 1, 1], {0: 0, 2: 4}))
    out.append(plan("fades m=71 R=197 long", 27, 2, 2, 197, [9, 62, 9, 1, 1], {0: 0, 2: 4}))
    return out


def _others():
    out = [
        # R = 200: the first fade runs through eight single-buffer steps (From's rows are sized for 27 samples), the second through
        # steps of 1, 3 and 9 buffers: n_fade = 27, 81, 91, and From's work rows grow twice in the middle of it
        plan("fade-long", 27, 2, 2, 200, [1] * 8 + [1, 3, 9] + [1] * 4, {0: 0, 8: 4}),
        # sweep-1 through two fades (the in-place run of test_gpu_eq_phases.py)
        plan("sweep-1 fades", 27, 2, 2, 200, [1] * 66, {0: 0, 33: 4}),
        # the largest buffers
        plan("big", 864, 8, 8, 700, [1, 3, 1], {0: 0, 1: 4}),
    ]
    # a set in the first step behind a fade's end; R < 2 has no fade at all and R = 2 one of a single sample: sets in consecutive steps
    for R in (0, 1, 2):
        out.append(plan(f"fade-sets R={R}", 27, 2, 2, R, [1, 1, 1, 3, 1, 1], {0: 0, 1: 4, 2: 7, 4: 2}))
    # R = 28 ends ON the step edge: the next set comes in the step right behind the fade
    out.append(plan("fade-sets R=28", 27, 2, 2, 28, [1, 1, 1, 3, 1, 1], {0: 0, 1: 4, 2: 7, 4: 2}))
    return out


PLANS = _sweeps() + _batches() + _fades() + _others()
BY_NAME = {p["name"]: p for p in PLANS}
assert len(BY_NAME) == len(PLANS)


def steps(pl):
    """the clock of the header, step by step: a set takes effect at the next step's first sample and To's grid starts there; From
    keeps its own grid; n_fade = min(n, t_set + R - 1 - t) while t - t_set + 1 < R.  Yields dicts t, n, to = (k0, n), frm = (k0,
    n_fade) or None.  A set while a fade runs is refused by the engine: a plan that asks for one is wrong"""
    t, t_set, t_set_from, have_from, R = 0, 0, 0, False, pl["R"]
    assert not set(pl["sets"]) - set(range(len(pl["cuts"]))), pl["name"]
    for k, nb in enumerate(pl["cuts"]):
        n = nb * pl["frames"]
        assert n > 0
        if k in pl["sets"]:
            assert not (have_from and t - t_set + 1 < R), (pl["name"], k, "a set during a fade")
            t_set_from, t_set, have_from = t_set, t, True
        fading = have_from and t - t_set + 1 < R
        n_fade = min(n, t_set + R - 1 - t) if fading else 0
        yield dict(step=k, t=t, n=n, to=((t - t_set) % P, n), frm=((t - t_set_from) % P, n_fade) if n_fade else None)
        t += n


def phases(pl):
    """every launch of a cascade: (which, k0, n)"""
    for s in steps(pl):
        yield ("to",) + s["to"]
        if s["frm"]:
            yield ("from",) + s["frm"]


def whole_blocks(k0, n):
    """G: the whole blocks of the step behind its first block (the one sample t lies in)"""
    return max(0, (k0 + n) // P - 1)


def classes(k0, n):
    """the cases of one cascade's step of n samples from phase k0, by the block definition: a block's last two outputs (the pair,
    samples P - 2 and P - 1) are what the next block depends on"""
    assert 0 <= k0 < P and n > 0
    end = k0 + n                                          # in samples from the first block's origin
    out = set()
    if k0 == P - 1:
        out.add("first_from_history")                     # the first block's sample P - 2 belongs to the step before
    if end <= P - 2:
        out.add("no_pair")                                # the step ends before its first block's pair
    if end == P - 1:
        out.add("only_first_of_pair")
    if end >= 2 * P - 1 and end % P == P - 1:
        out.add("tail_first_of_pair")                     # a later, unfinished block's sample P - 2 is the step's last
    if end % P == 0:
        out.add("ends_on_block")
    if whole_blocks(k0, n) in BATCH_G:
        out.add(f"G={whole_blocks(k0, n)}")
    if end % 256 in (0, 1):
        out.add(f"grid_edge_{end % 256}")                 # positions are worked on in groups of 256 from the first block's origin
    if n < H:
        out.add("shorter_than_history")
    return out


CLASSES = ["first_from_history", "no_pair", "only_first_of_pair", "tail_first_of_pair", "ends_on_block"] + [f"G={g}" for g in BATCH_G] + \
    ["grid_edge_0", "grid_edge_1", "shorter_than_history"]
FROM_CLASSES = [c for c in CLASSES if not (c.startswith("G=") and int(c[2:]) >= 63)]


def coverage(plans=None):
    """{which: {class: {plan name: launches}}}"""
    table = {w: {c: {} for c in CLASSES} for w in ("to", "from")}
    for pl in PLANS if plans is None else plans:
        for which, k0, n in phases(pl):
            for c in classes(k0, n):
                table[which][c][pl["name"]] = table[which][c].get(pl["name"], 0) + 1
    return table


def coverage_text(table):
    lines = []
    for which in ("to", "from"):
        for c in CLASSES:
            by = table[which][c]
            some = ", ".join(f"{k}: {v}" for k, v in list(by.items())[:4]) + (f", ... ({len(by)} plans)" if len(by) > 4 else "")
            lines.append(f"{which:4s} {c:22s} {sum(by.values()):5d}  {some}")
    return "\n".join(lines)


def total_buffers(pl):
    return sum(pl["cuts"])


def signal(pl):
    """the plan's input [C][n] f32: seeded noise, the seed from the plan's name"""
    rng = np.random.default_rng(zlib.crc32(pl["name"].encode()))
    return rng.standard_normal((pl["C"], total_buffers(pl) * pl["frames"])).astype(np.float32)


def bank_entry(c, s, shift):
    return BANK[(shift + 3 * c + s) % len(BANK)]


def coefficients(Cn, S, shift=0):
    """[C][S][5] as tests/test_gpu_eq.py's coefficients(), by the model's design(): every channel its own sections of BANK"""
    return np.array([[em.design(bank_entry(c, s, shift)[0], RATE, *bank_entry(c, s, shift)[1:]) for s in range(S)] for c in range(Cn)])


def run_model(pl, cuts=None, x=None):
    """the model alone over a plan -> out [C][n] f32.  cuts: other step lengths in buffers over the same samples (plans with one
    set, before step 0)"""
    x = signal(pl) if x is None else x
    if cuts is not None:
        assert set(pl["sets"]) == {0} and sum(cuts) == total_buffers(pl)
    model = em.Model(pl["C"], pl["S"], pl["R"])
    outs, at = [], 0
    for k, nb in enumerate(pl["cuts"] if cuts is None else cuts):
        n = nb * pl["frames"]
        if k in pl["sets"]:
            model.set(coefficients(pl["C"], pl["S"], pl["sets"][k]))
        outs.append(model.process(x[:, at:at + n]))
        at += n
    assert at == x.shape[1] == model.t
    return np.concatenate(outs, axis=1)
