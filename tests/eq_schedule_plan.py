"""The EQ bus's schedule plans (no GPU, no engine library): runs with coefficient sets at absolute samples, chosen so that every
branch of a scheduled step is reached (include/openpbso_amd.h "The EQ bus's SCHEDULE"; openpbso_amd/csrc/eq_schedule.h).  A set cuts
its predecessor's block at offset (t_set - t_prev) mod P; its fade keeps the predecessor running for R - 1 samples more; a step
works on positions in groups of 256 from its first sample and walks its blocks 64 at a time.  reach() names what a plan reaches
from those definitions alone; tests/test_eq_schedule_plan.py proves the coverage with the model alone, tests/test_gpu_eq_schedule.py
runs the plans on the device against the model, bit for bit.

A plan: frames per buffer, C channels, S sections, R cross-fade samples, cuts = the step lengths in buffers, sets = {t_set: shift}:
the coefficient set eq_phase_plan.coefficients(C, S, shift) takes effect at the absolute sample t_set."""
import zlib

import numpy as np

from tests import eq_model as em
from tests import eq_phase_plan as pp

P = em.P
H = P + 2


def plan(name, frames, Cn, S, R, cuts, t_sets):
    t_sets = sorted(t_sets)
    return dict(name=name, frames=frames, C=Cn, S=S, R=R, cuts=list(cuts), sets={t: (3 * i + 1) % 10 for i, t in enumerate(t_sets)})


def _offsets():
    """the gap to the predecessor walks through every residue mod P: the predecessor's block is cut at offset 0 .. 63"""
    out = []
    for R, base in ((0, P), (3, P), (67, 2 * P)):
        t, ts = max(R - 1, 0) + 5, []
        for off in range(P):
            ts.append(t)
            t += base + off + 1
        ts.append(t)                                      # (gap base + 64: offset 0)
        nb = -(-(t + 100) // 27)
        out.append(plan(f"offsets R={R}", 27, 2, 2, R, [nb], ts))
    return out


def _spacing():
    """sets 1 apart (R <= 2) and exactly R - 1 apart, for every R; the first one as early as the identity allows"""
    out = []
    for R in (0, 1, 2, 3, 64, 67, 200):
        gap = max(R - 1, 1)
        first = max(R - 1, 0)
        ts = [first + gap * j for j in range(6)]
        ts += [ts[-1] + gap + 40 + gap * j for j in range(3)]
        nb = -(-(ts[-1] + gap + 60) // 27)
        out.append(plan(f"spacing R={R}", 27, 2, 2, R, [nb // 2, nb - nb // 2], ts))
    return out


def _runs():
    """70 sets one sample apart whose last one is the last sample of a step (d = 0), the sample before (d = -1), the first sample
    of the next step (d = +1): the history behind the step holds values of more than EQ_HIST sets"""
    out = []
    for R in (0, 2):
        for d in (-1, 0, 1):
            end = 10 * 27
            out.append(plan(f"run70 R={R} d={d}", 27, 2, 2, R, [10, 2, 1], [end - 70 + j + d for j in range(70)]))
    return out


def _edges():
    out = [
        # a set on the first and on the last sample of a step
        plan("first-last R=64", 513, 2, 2, 64, [1, 1, 1], [513, 2 * 513 - 1]),
        plan("first-last R=0", 27, 2, 2, 0, [2, 1, 1], [54, 80]),
        # t_set at offsets 255, 256, 257 of a step's positions
        plan("group-edge R=0", 513, 2, 2, 0, [1, 2], [513 + 255, 513 + 256, 513 + 257]),
        plan("group-edge R=3", 513, 2, 2, 3, [1, 2], [513 + 255, 513 + 257, 513 + 511, 513 + 513]),
        # a set in a step of one buffer of 27 < EQ_HIST samples, the fade across many such steps
        plan("short-steps R=200", 27, 2, 2, 200, [1] * 40, [200, 200 + 199, 200 + 199 + 230]),
        plan("short-steps R=3", 27, 2, 2, 3, [1] * 12, [26, 28, 54, 81, 83, 107]),
    ]
    # a tail that ends on the last sample of a step (d = 0), one before it and one behind it
    for R in (3, 64, 200):
        for d in (-1, 0, 1):
            end = 20 * 27
            out.append(plan(f"tail-end R={R} d={d}", 27, 2, 2, R, [20, 1, 8], [end - (R - 1) + d]))
    # the chain walks 64 blocks at a time: sets at the blocks 63, 64, 65 of a step (the first set makes the grid start with the step)
    t0 = 10 * 27
    out.append(plan("batch-edge V", 27, 2, 2, 0, [10, 200], [t0, t0 + 63 * P, t0 + 63 * P + 10, t0 + 64 * P, t0 + 64 * P + 1, t0 + 65 * P + 63]))
    # ... and the tails' list: 199 samples are four blocks, so the seventeenth tail crosses the batch edge
    out.append(plan("batch-edge F R=200", 27, 2, 2, 200, [8, 160], [199 + 199 * j for j in range(21)]))
    return out


PLANS = _offsets() + _spacing() + _runs() + _edges()
BY_NAME = {p["name"]: p for p in PLANS}
assert len(BY_NAME) == len(PLANS)


def total(pl):
    return sum(pl["cuts"]) * pl["frames"]


def signal(pl):
    rng = np.random.default_rng(zlib.crc32(pl["name"].encode()))
    return rng.standard_normal((pl["C"], total(pl))).astype(np.float32)


def coefficients(pl, t_set):
    if "coef" in pl:                                      # (a plan with coefficients of its own: a function of the shift)
        return pl["coef"](pl["sets"][t_set])
    return pp.coefficients(pl["C"], pl["S"], pl["sets"][t_set])


def step_edges(pl, cuts=None):
    e, at = [0], 0
    for nb in (pl["cuts"] if cuts is None else cuts):
        at += nb * pl["frames"]
        e.append(at)
    return e


def other_cuts(pl):
    """the same samples cut into other steps, in buffers: one step, and one buffer per step"""
    nb = sum(pl["cuts"])
    return {"one step": [nb], "one buffer per step": [1] * nb}


def run_model(pl, x=None, tables=None):
    """the model alone: the input cut at every t_set and at every step edge, with set() before the piece that begins at a t_set.
    tables: {t_set: [C][S][5][P]} to use in place of the reference's own"""
    x = signal(pl) if x is None else x
    model = em.Model(pl["C"], pl["S"], pl["R"])
    edges = sorted(set(step_edges(pl)) | set(pl["sets"]))
    outs = []
    for a, b in zip(edges[:-1], edges[1:]):
        if a in pl["sets"]:
            if tables is None:
                model.set(coefficients(pl, a))
            else:
                model.set(tables_=tables[a])
        outs.append(model.process(x[:, a:b]))
    assert model.t == x.shape[1]
    return np.concatenate(outs, axis=1)


def vblocks(pl, t, n, t_to):
    """the blocks of the timeline in force in the step [t, t + n): (origin, length, t_set of the set), by the definition: a set's
    blocks start at its t_set, and a block ends where the next set begins or the step ends"""
    ts = [t_to] + [s for s in sorted(pl["sets"]) if t <= s < t + n]
    out = []
    for g, s in enumerate(ts):
        lo, hi = max(s, t), (ts[g + 1] if g + 1 < len(ts) else t + n)
        if hi <= lo:
            continue
        o = lo - (lo - s) % P
        while o < hi:
            out.append((o, min(P, hi - o), s))
            o += P
    return out


def reach(pl, cuts=None):
    """what the plan reaches, as a set of names"""
    out, R = set(), pl["R"]
    ts = sorted(pl["sets"])
    edges = step_edges(pl, cuts)
    out.add(f"R={R}")
    for a, b in zip([0] + ts[:-1], ts):
        out.add(f"offset={(b - a) % P}")
        if b - a == 1:
            out.add("gap=1")
        if R >= 2 and b - a == R - 1:
            out.add("gap=R-1")
    if pl["frames"] < H and any(nb == 1 for nb in (pl["cuts"] if cuts is None else cuts)):
        out.add("n<H")
    for a, b in zip(edges[:-1], edges[1:]):
        inside = [s for s in ts if a <= s < b]
        if not inside:
            continue
        for s in inside:
            if s == a:
                out.add("first sample")
            if s == b - 1:
                out.add("last sample")
            if s - a in (255, 256, 257):
                out.add(f"group offset {s - a}")
            if R >= 2 and s + R - 2 - (b - 1) in (-1, 0, 1):
                out.add(f"tail end {s + R - 2 - (b - 1):+d}")
        # a run of 70 one-sample sets against the step end
        for d in (-1, 0, 1):
            want = [b - 70 + j + d for j in range(70)]
            if set(want) <= set(ts):
                out.add(f"run70 {d:+d}")
        t_to = max([s for s in ts if s < a], default=0)
        blk = vblocks(pl, a, b - a, t_to)
        for i, (o, L, s) in enumerate(blk):
            if s in inside and o == s and i in (63, 64, 65):
                out.add(f"V batch block {i}")
        # the tails' blocks: every set's predecessor for R - 1 samples on the predecessor's grid
        if R >= 2:
            nf, prev = 0, t_to
            for s in inside:
                lo, hi = s, min(s + R - 1, b)
                o = lo - (lo - prev) % P
                first = nf
                while o < hi:
                    nf += 1
                    o += P
                if first < 64 < nf or first == 64:
                    out.add("F batch edge")
                prev = s
    return out


REQUIRED = [f"offset={k}" for k in range(P)] + [f"R={R}" for R in (0, 1, 2, 3, 64, 67, 200)] + \
    ["gap=1", "gap=R-1", "n<H", "first sample", "last sample", "group offset 255", "group offset 256", "group offset 257",
     "tail end -1", "tail end +0", "tail end +1", "run70 -1", "run70 +0", "run70 +1", "V batch block 63", "V batch block 64",
     "V batch block 65", "F batch edge"]
