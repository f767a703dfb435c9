"""K5's scan (kernels_scan.hip: iir_scan_kernel, iir_scan_seg_kernel, dense_increment_kernel) at its batch, group and hit-window
borders: the 150-buffer scene of tests/scan_border_scene.py (anchored without a GPU by tests/test_scan_border_scene.py) against the fp64
oracle, in the serial scan at chunk lengths and launch cuts that move every border over the lanes, in runs that END on a border (the
state a launch hands on is the scan's own product), in the segmented scan with chunks longer than its batches, and with launches of a
handful of dense rows.  Every run says through info() which path it took; the builds reached:

    iir_scan_kernel<DIRECT, DENSE>      direct_hits = 0 / -1  x  dense / plain scene: test_serial_scan_in_its_four_builds (and all others)
    iir_scan_seg_kernel<DIRECT, DENSE>  the same four: test_segmented_scan_with_chunks_longer_than_a_batch
    dense_increment_kernel              every dense-scene case (total_dense_increment_launches)

DENSE is the build of a launch with dense rows (launch_iir_scan: vinc != nullptr, counted by total_dense_increment_launches), DIRECT the
build of an engine whose vertex hits are projected by the bank (direct_hits >= 0).

The bars are the project's stated ones (tests/test_gpu_time_chunks.py::_check): audio max|d| <= 5e-4 peak and relative
L2 <= 1e-3 per object, qnorm rows <= 5e-4 row peak + 2e-6 audio peak, state atol 5e-4 max|state|, `emitted` equal -- and the audio bar
buffer by buffer against the object's run peak, so that a failure names the first bad buffer: the border that broke.
"""
import numpy as np
import pytest

from openpbso_amd import capi
from tests import scan_border_scene as S
from tests.scenarios import B, rel_errors, run_engine, run_oracle

pytestmark = pytest.mark.gpu

NB = S.NB
PREFIXES = (63, 64, 65, 80, 128, 129)
DENSE_IDS = {True: "dense", False: "plain"}
BLOCK = dict(form=capi.FORM_BLOCK, bank_kernel=capi.BANK_BLOCK, chunk_buffers=NB)
HIT_CUTS = [cut for cut, *_ in S.HIT_CUTS if sum(cut) == NB and len(cut) > 1]                   # [30, 120], [14, 136]: 33 and 17 hits in one batch
CUTS = [[NB], [1, 149], [2, 148], [63, 87], [64, 86], [65, 85], [7, 9, 16, 33, 85]] + HIT_CUTS + ["default"]      # "default": the engine's chunk_buffers, 128 + 22
# launches of exactly 4, 4, 5, 3 and 1 dense rows (INC_RB = 4 rows per wave of dense_increment_kernel: one wave full, one row more,
# one less, a single row), between launches of none and a tail of 20
DENSE_ROW_CUT = [60, 3, 2, 5, 56, 3, 1, 20]


@pytest.fixture(scope="module")
def scenes():
    """per variant: the objects, the events, the script's reading and the oracle's run -- computed once, never changed"""
    out = {}
    for dense in (True, False):
        objs, evs = S.build(dense)
        want = run_oracle(objs, evs, NB)
        for v in want.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        out[dense] = dict(objs=objs, evs=evs, kind=S.script_rows(evs), want=want, runs={})
    return out


@pytest.fixture(scope="module")
def prefix_oracles(scenes):
    return {(dense, k): run_oracle(sc["objs"], [e for e in sc["evs"] if e["t"] < k], k) for dense, sc in scenes.items() for k in PREFIXES}


def launches_of(cut):
    return [128, NB - 128] if cut == "default" else list(cut)


def run(sc, cut=None, n_buffers=NB, **kw):
    settings = dict(BLOCK)
    if cut == "default":
        del settings["chunk_buffers"]
        cut = None
    settings.update(kw)
    evs = sc["evs"] if n_buffers == NB else [e for e in sc["evs"] if e["t"] < n_buffers]
    return run_engine(sc["objs"], evs, n_buffers, split=cut, **settings)


def check_path(got, sc, launches, cb, segmented):
    """the path the run names is the one that ran: every launch cut in time on the block kernel, none on the per-sample kernel, the
    dense increments for exactly the launches that have dense rows, the segmented scan for exactly the launches it fits"""
    info = got["info"]
    edges = np.concatenate([[0], np.cumsum(launches)])
    n_dense = sum(S.dense_rows(sc["kind"], lo, hi) > 0 for lo, hi in zip(edges[:-1], edges[1:]))
    n_seg = sum(2 <= -(-n // min(cb, n)) <= 8 for n in launches) if segmented else 0
    counters = {k: info[k] for k in ("total_time_chunk_launches", "total_block_launches", "total_sample_launches", "total_split_launches",
                                     "total_dense_increment_launches", "total_segmented_scans")}
    assert counters == dict(total_time_chunk_launches=len(launches), total_block_launches=len(launches), total_sample_launches=0,
                            total_split_launches=0, total_dense_increment_launches=n_dense, total_segmented_scans=n_seg), counters


def check(got, want, label, qnorm=True, n_buffers=NB):
    """the stated bars; returns the figures (audio max / peak, relative L2, qnorm row excess / bar, state max / peak)"""
    assert np.isfinite(got["audio"]).all(), label
    assert np.array_equal(got["emitted"], want["emitted"]), label
    n_obj = want["audio"].shape[0]
    peak = np.abs(want["audio"]).max(axis=1)
    err = np.abs(got["audio"].astype(np.float64) - want["audio"]).reshape(n_obj, n_buffers, B).max(axis=2) / peak[:, None]
    bad = np.argwhere(err > 5e-4)
    assert not len(bad), f"{label}: first bad (object, buffer) {tuple(int(v) for v in bad[np.argmin(bad[:, 1])])} of {len(bad)}; per-buffer max {err.max():.2e} of peak"
    mx, l2 = rel_errors(got["audio"], want["audio"])
    assert (mx <= 5e-4).all() and (l2 <= 1e-3).all(), (label, mx.max(), l2.max())
    fig_q = fig_qrow = 0.0
    if qnorm:
        assert set(got["qnorm"]) >= set(want["qnorm"])
        for key, w in want["qnorm"].items():
            bar = 5e-4 * max(np.abs(w).max(), 1e-30) + 2e-6 * peak[key[0]]
            d = np.abs(got["qnorm"][key] - w).max()
            assert d <= bar, (label, key, d, bar)
            fig_q, fig_qrow = max(fig_q, d / bar), max(fig_qrow, d / max(np.abs(w).max(), 1e-30))
    fig_s = 0.0
    for i, (g, w) in enumerate(zip(got["state"], want["state"])):
        for c in (0, 1):
            top = max(np.abs(w[c]).max(), 1e-30)
            np.testing.assert_allclose(g[c], w[c], rtol=0, atol=5e-4 * top, err_msg=f"{label}: state {c} of object {i}")
            fig_s = max(fig_s, np.abs(g[c] - w[c]).max() / top)
    print(f"FIG {label}: audio {mx.max():.2e} l2 {l2.max():.2e} qnorm/bar {fig_q:.2e} qnorm/rowpeak {fig_qrow:.2e} state {fig_s:.2e}")
    return mx.max()


def same_bits(a, b, label):
    assert np.array_equal(a["audio"], b["audio"]) and np.array_equal(a["emitted"], b["emitted"]), label
    assert set(a["qnorm"]) == set(b["qnorm"])
    for key in a["qnorm"]:
        assert np.array_equal(a["qnorm"][key], b["qnorm"][key]), (label, key)
    for x, y in zip(a["state"], b["state"]):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1]), label


def uncut(sc, time_chunks):
    """the serial scan of the whole run in one launch, kept per chunk length: what the cuts and the segmented scan are compared with"""
    key = ("serial", time_chunks)
    if key not in sc["runs"]:
        sc["runs"][key] = run(sc, scan_kernel=1, time_chunks=time_chunks)
    return sc["runs"][key]


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
@pytest.mark.parametrize("time_chunks", [1, 3, 8, 63, 64, 65])
def test_serial_scan_marks_at_every_lane(scenes, time_chunks, dense):
    """chunk starts on every lane (1), in every position of a group (3), on lane 0 of every group and of batches 1 and 2 (8: 64 and
    128), a chunk that is exactly a batch (64), one buffer less (63: the marks on lane 63 and on lane 62 of batch 1) and one more"""
    sc = scenes[dense]
    got = uncut(sc, time_chunks)
    check_path(got, sc, [NB], time_chunks, segmented=False)
    assert got["info"]["last_time_chunk_buffers"] == time_chunks
    check(got, sc["want"], f"serial tc={time_chunks} {DENSE_IDS[dense]}")


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
@pytest.mark.parametrize("cut", CUTS, ids=lambda c: c if isinstance(c, str) else "+".join(map(str, c)))
def test_serial_scan_is_bit_identical_for_every_cut(scenes, cut, dense):
    """time_chunks = 1: the cuts move the same absolute buffer over other lanes, groups and batches -- 63 | 64 to lanes 62 | 63 behind
    [1, 149], to lane 0 of a launch behind [64, 86]; the 40 hits of [64, 104) into windows of 16 + 16 + 8 (uncut), 16 + 16 + 1 and
    16 + 1 (the hit-count cuts); behind [2, 148] batch 1 (66 .. 129) has no listener move of its own and the chunk starts of batch 2 take the
    row that batch 0 set -- and the serial scan claims not to depend on any of it: audio, qnorm rows and state bit for bit"""
    sc = scenes[dense]
    got = run(sc, cut=None if cut == [NB] else cut, scan_kernel=1, time_chunks=1)
    check_path(got, sc, launches_of(cut), 1, segmented=False)
    check(got, sc["want"], f"serial tc=1 cut={cut} {DENSE_IDS[dense]}")
    same_bits(got, uncut(sc, 1), cut)


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
@pytest.mark.parametrize("direct_hits", [0, -1])
@pytest.mark.parametrize("qnorm", [capi.QNORM_ALL, capi.QNORM_OFF])
def test_serial_scan_in_its_four_builds(scenes, qnorm, direct_hits, dense):
    """iir_scan_kernel<DIRECT = (direct_hits == 0), DENSE = dense>, with and without qnorm rows, chunks of 8 and of 1 behind a cut"""
    sc = scenes[dense]
    for tc, cut in ((8, None), (1, [63, 87])):
        got = run(sc, cut=cut, scan_kernel=1, time_chunks=tc, qnorm=qnorm, direct_hits=direct_hits)
        check_path(got, sc, cut or [NB], tc, segmented=False)
        check(got, sc["want"], f"serial build direct={direct_hits} {DENSE_IDS[dense]} qnorm={qnorm} tc={tc}", qnorm=qnorm != capi.QNORM_OFF)


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
def test_serial_scan_with_the_split_bf16_projection(scenes, dense):
    sc = scenes[dense]
    for tc, cut in ((8, None), (1, [64, 86])):
        got = run(sc, cut=cut, scan_kernel=1, time_chunks=tc, form=capi.FORM_BLOCK_BF16)
        check_path(got, sc, cut or [NB], tc, segmented=False)
        check(got, sc["want"], f"serial bf16 {DENSE_IDS[dense]} tc={tc}")


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
@pytest.mark.parametrize("k", PREFIXES)
def test_a_run_that_ends_on_a_border_leaves_the_oracles_state(scenes, prefix_oracles, k, dense):
    """k buffers in one launch: the state behind the last lane of batch 0 (63 buffers: the batch's tail, 64: a full batch), behind
    lane 0 of batch 1 (65), behind exactly one hit window in batch 1 (80), behind two full batches and behind lane 0 of batch 2 --
    what the next launch would start from, and the audio"""
    sc = scenes[dense]
    for tc in (1, 8):
        got = run(sc, n_buffers=k, scan_kernel=1, time_chunks=tc)
        info = got["info"]
        assert info["total_time_chunk_launches"] == info["total_block_launches"] == 1 and info["total_sample_launches"] == 0
        assert info["total_dense_increment_launches"] == (S.dense_rows(sc["kind"], 0, k) > 0) and info["total_segmented_scans"] == 0
        check(got, prefix_oracles[(dense, k)], f"prefix {k} tc={tc} {DENSE_IDS[dense]}", n_buffers=k)


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
@pytest.mark.parametrize("direct_hits", [0, -1])
@pytest.mark.parametrize("cb", [19, 30, 33, 75, 149])
def test_segmented_scan_with_chunks_longer_than_a_batch(scenes, cb, direct_hits, dense):
    """iir_scan_seg_kernel<DIRECT, DENSE>: 8, 5, 5, 2 and 2 chunks, each longer than the DENSE build's batch of 16, at 33 and 75 longer
    than the plain build's 32, at 149 a last chunk of one buffer; at 19 chunk 4 is the all-clear stretch [76, 95) of object 2
    (n_stepped = 0: the identity) and chunks 4 and 5 have no listener move between chunks that have one.  Against the oracle, and
    against the serial scan of the same settings at the bar the 16-buffer test holds (2e-5 of peak)."""
    sc = scenes[dense]
    assert [-(-NB // c) for c in (19, 30, 33, 75, 149)] == [8, 5, 5, 2, 2]
    for cut in (None, [64, 86]):
        seg = run(sc, cut=cut, scan_kernel=2, time_chunks=cb, direct_hits=direct_hits)
        check_path(seg, sc, cut or [NB], cb, segmented=True)
        if cut is None:
            assert seg["info"]["total_segmented_scans"] == 1
        check(seg, sc["want"], f"segmented cb={cb} cut={cut} direct={direct_hits} {DENSE_IDS[dense]}")
        ser = run(sc, cut=cut, scan_kernel=1, time_chunks=cb, direct_hits=direct_hits) if cut or direct_hits else uncut(sc, cb)
        check_path(ser, sc, cut or [NB], cb, segmented=False)
        check(ser, sc["want"], f"serial cb={cb} cut={cut} direct={direct_hits} {DENSE_IDS[dense]}")
        mx, _ = rel_errors(seg["audio"], ser["audio"])
        print(f"FIG segmented against serial cb={cb} cut={cut} direct={direct_hits} {DENSE_IDS[dense]}: {mx.max():.2e}")
        assert mx.max() <= 2e-5, mx.max()


@pytest.mark.parametrize("dense", [True, False], ids=DENSE_IDS.get)
def test_nine_chunks_keep_the_serial_scan(scenes, dense):
    """17 buffers per chunk are 9 chunks, one more than a workgroup of the segmented form has waves: the serial scan, also when the
    segmented one is asked for -- the same bits"""
    sc = scenes[dense]
    got = run(sc, scan_kernel=2, time_chunks=17)
    check_path(got, sc, [NB], 17, segmented=True)
    assert got["info"]["total_segmented_scans"] == 0
    check(got, sc["want"], f"nine chunks {DENSE_IDS[dense]}")
    same_bits(got, uncut(sc, 17), "scan_kernel 2 against 1 at nine chunks")


def test_launches_of_a_handful_of_dense_rows(scenes):
    """dense_increment_kernel takes INC_RB = 4 rows per wave: launches of 4, 4, 5, 3 and 1 rows (and of none), bit-identical at one
    buffer per chunk to the uncut run, whose single launch evaluates all 37"""
    sc = scenes[True]
    edges = np.concatenate([[0], np.cumsum(DENSE_ROW_CUT)])
    rows = [S.dense_rows(sc["kind"], lo, hi) for lo, hi in zip(edges[:-1], edges[1:])]
    assert rows == [0, 4, 4, 5, 0, 3, 1, 20] and sum(rows) == 37
    got = run(sc, cut=DENSE_ROW_CUT, scan_kernel=1, time_chunks=1)
    check_path(got, sc, DENSE_ROW_CUT, 1, segmented=False)
    assert got["info"]["total_dense_increment_launches"] == 6
    check(got, sc["want"], "dense row cut tc=1")
    same_bits(got, uncut(sc, 1), DENSE_ROW_CUT)
    got = run(sc, cut=DENSE_ROW_CUT, scan_kernel=1, time_chunks=4)
    check_path(got, sc, DENSE_ROW_CUT, 4, segmented=False)
    check(got, sc["want"], "dense row cut tc=4")


@pytest.mark.parametrize("shape", [1, 2, 4])
def test_dense_borders_at_every_team_shape(scenes, shape):
    """the whole dense run -- dense rows on both sides of 63 | 64 and 127 | 128 -- at one, two and four modes per lane"""
    sc = scenes[True]
    for tc in (8, 1):
        got = run(sc, scan_kernel=1, time_chunks=tc, time_chunk_shape=shape)
        check_path(got, sc, [NB], tc, segmented=False)
        assert got["info"]["total_dense_increment_launches"] == 1 and got["info"]["last_time_chunk_shape"] == shape
        check(got, sc["want"], f"dense shape={shape} tc={tc}")
