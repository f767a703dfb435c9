"""The master bus's window plan (no GPU, no engine library): look-aheads and holds chosen so that every class of the sliding minimum
of kernels_master.hip is reached, and an input on which a wrong minimum shows.  With W = L + H + 1 and 2^k <= W < 2^(k+1) the header
comment of that file builds a(e) = min r[e - W + 1 .. e] in three parts: min(k, 10) doubling levels in LDS on strips of 1024 samples
of E = history ++ step (e = 2 L + H + q for the step's sample q), k - 10 further passes over all of E that ping-pong between two
arrays, and a(e) = min(M[e], M[e - D]), D = W - 2^k.  The gain then runs in strips of 64 samples, or of 1024 once a step has 16384.
classes() names these from that comment alone; nothing built is imported.  tests/test_master_window_plan.py proves the coverage
and runs the model over every case; tests/test_gpu_master_windows.py runs the cases on the device against the model, bit for bit.

A case: name, W, L, H, C channels, seed.  The input of a case is a staircase (staircase()): noise far below the ceiling, so that
r = 1 between peaks, and eight isolated peaks that rotate over the channels, four of descending magnitude and then four of
ascending magnitude behind the last exit of the first four.  In the descending run the oldest peak in the window sets the minimum,
so a(t) rises at the exact sample p + W at which the peak at p has left; in the ascending run a(t) falls at every entry p.  The
peaks are placed so that, of the exits and of the entries alike, one sits at e mod 1024 = 1023 and one at e mod 1024 = 0 of the
single-step run (the borders of the minimum's strips), one on the last sample of a step of the uneven cut and one on the first.
Eight placed events have to fit into about 0.4 W, so the peaks are W / 24 apart, two of each run next to each other."""
import numpy as np

B = 513                                  # frames per buffer of every case
T = 0.7                                  # the ceiling of every case
NOISE = 0.05
LDS_LEVELS, MIN_STRIP = 10, 1024         # kernels_master.hip: MS_LEVELS, MS_STRIP
WIDE_FROM, WIDE_STRIP, NARROW_STRIP = 16384, 1024, 64
MAX_L, MAX_H = 4096, 65536               # include/openpbso_amd.h: MASTER_MAX_LOOKAHEAD, MASTER_MAX_HOLD
# the uneven cut, in buffers: a one-buffer step right behind the first; 31 buffers are the longest step of the narrow gain launch
CUT_HEAD, CUT_CYCLE = (2, 1, 3, 1, 4), (31, 5, 2, 9, 1, 13, 4, 7)
DESC = (6.0, 4.9, 3.8, 2.7)              # |peak| of the descending run and of the ascending one; all above T, all r distinct
ASC = (1.4, 2.3, 3.2, 4.1)
KINDS = ("strip-last", "strip-first", "step-last", "step-first")


def classes(L, H, n):
    """what launch_master does for a step of n samples, from the header comment of kernels_master.hip"""
    W = L + H + 1
    k = W.bit_length() - 1                               # 2^k <= W < 2^(k+1)
    lds = min(k, LDS_LEVELS)
    wide = n >= WIDE_FROM
    strip = WIDE_STRIP if wide else NARROW_STRIP
    return dict(W=W, k=k, lds_levels=lds, passes=k - lds, D=W - (1 << k), wide=wide, gain_strips=-(-n // strip),
                ragged=n % strip != 0, last_in="M1" if (k - lds) % 2 else "M0")


def _shape(W, look):
    """(L, H) of a window of W samples: look = 1: L = 1 (w = [1]: g shows a(t) directly) or the least L that the largest hold
    leaves; look = 0: H = 0, the gain kernel's halo is the window"""
    if look == 0:
        return W - 1, 0
    L = max(1, W - 1 - MAX_H)
    if L > 1:
        L = 1 << (L - 1).bit_length()                    # 67584: L = 2048; 69633: L = 4096, the largest there is
    return L, W - 1 - L


def windows():
    """every W of the plan: 2^k - 1, 2^k, 2^k + 1 for k = 1 .. 16, the largest there is, and one with D in mid range for each of the
    pass counts 1 .. 6 (3 * 2^(k-1); at k = 16 no W reaches that: 2^16 + 2048)"""
    ws = {W for k in range(1, 17) for W in ((1 << k) - 1, 1 << k, (1 << k) + 1) if W >= 2}
    ws |= {MAX_L + MAX_H + 1}
    ws |= {3 << (k - 1) for k in range(11, 16)} | {(1 << 16) + 2048}
    return sorted(ws)


def cases():
    out = []
    for W in windows():
        for look in (1, 0):
            if look == 0 and (W > MAX_L + 1 or W == 2):  # (W = 2 with H = 0 is L = 1 again)
                continue
            L, H = _shape(W, look)
            assert 1 <= L <= MAX_L and 0 <= H <= MAX_H and L + H + 1 == W
            i = len(out)
            out.append(dict(name=f"W={W} L={L} H={H}", W=W, L=L, H=H, C=(1, 3, 8)[i % 3], seed=1000 + i))
    return out


def boundaries(limit):
    """the first samples of the steps of the uneven cut, up to limit"""
    out, at, i = [], 0, 0
    while at <= limit:
        out.append(at)
        at += B * (CUT_HEAD[i] if i < len(CUT_HEAD) else CUT_CYCLE[(i - len(CUT_HEAD)) % len(CUT_CYCLE)])
        i += 1
    return out


def cuts(nb):
    """the two cuts of nb buffers: one step, and the uneven steps of at most 31 buffers (the last one cut short)"""
    uneven, i = [], 0
    while sum(uneven) < nb:
        s = CUT_HEAD[i] if i < len(CUT_HEAD) else CUT_CYCLE[(i - len(CUT_HEAD)) % len(CUT_CYCLE)]
        uneven.append(min(s, nb - sum(uneven)))
        i += 1
    return [nb], uneven


def _place(cursor, kind, shift, HL, starts):
    """the least peak position p >= cursor whose event sample p + shift is of the kind"""
    x = cursor + shift
    if kind == "strip-last":
        x += (1023 - (HL + x)) % 1024
    elif kind == "strip-first":
        x += (-(HL + x)) % 1024
    elif kind == "step-last":
        x = min(s for s in starts if s - 1 >= x) - 1
    else:
        x = min(s for s in starts if s >= x)
    return x - shift


def layout(case):
    """the peaks of a case: [(position, channel, value)], the placed exits and entries {kind: sample}, and n"""
    W, HL = case["W"], 2 * case["L"] + case["H"]
    gap = max(1, W // 24)
    starts = boundaries(3 * W + 40 * B)[1:]
    peaks, exits, entries, cursor = [], {}, {}, 1
    for run, mags, shift, events in ((0, DESC, W, exits), (1, ASC, 0, entries)):
        for i, kind in enumerate(KINDS):
            p = _place(cursor, kind, shift, HL, starts)
            j = len(peaks)
            peaks.append((p, j % case["C"], mags[i] * (-1) ** j))
            events[kind] = p + shift
            cursor = p + (1 if kind == "step-last" else gap)
        cursor = peaks[-1][0] + W + gap                  # the ascending run starts behind the last exit of the descending one
    n = -(-(peaks[-1][0] + 2) // B) * B
    return dict(peaks=peaks, exits=exits, entries=entries, n=n)


def staircase(case):
    """x [C][n] float32 of a case, and its layout"""
    lay = layout(case)
    rng = np.random.default_rng(case["seed"])
    x = (rng.standard_normal((case["C"], lay["n"])) * NOISE).astype(np.float32)
    assert np.abs(x).max() < 0.5 * T
    for p, c, v in lay["peaks"]:
        x[c, p] = v
    return x, lay


def dense(case, n):
    """dense noise of scale 1: nearly every sample is limited"""
    return np.random.default_rng(case["seed"] + 7).standard_normal((case["C"], n)).astype(np.float32)


def ratios(x, ceiling=T):
    """r(t) of an input at gain 1: the header's line, in numpy f32"""
    pk = np.abs(np.asarray(x, dtype=np.float32)).max(axis=0)
    t = np.float32(ceiling)
    with np.errstate(divide="ignore"):
        return np.where(pk > t, t / pk, np.float32(1)).astype(np.float32)


def window_minimum(r, W):
    """a(t) = min r[t - W + 1 .. t] (1 before t = 0) by the doubling scheme of the header comment, in numpy: k levels, then D"""
    k = W.bit_length() - 1
    m = np.asarray(r, dtype=np.float32).copy()

    def back(a, d):
        return np.concatenate([np.ones(min(d, a.size), dtype=np.float32), a[:max(a.size - d, 0)]])

    for j in range(k):
        m = np.minimum(m, back(m, 1 << j))
    return np.minimum(m, back(m, W - (1 << k)))
