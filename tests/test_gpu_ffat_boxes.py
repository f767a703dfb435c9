"""K4 (kernels_exact.hip) on box-shaped FFAT maps and at edge listener positions.

Every other GPU test of the lookup feeds it synth.uniform_cube_geometry's cube -- Nx == Ny on every face, strides f * dim^2,
center3 == center -- and listeners outside the box with no zero component of centre - p.  Here the maps lie over the boxes of
tests/ffat_boxes.py (a different (Nx, Ny) on each pair of faces, faces one cell wide, center3 off the centre, more cells than
the batch kernel's LDS window) and the listeners stand along the axes, on diagonals through the box's edges and corners, over
cell centres and borders, and inside the box.  All of it through each lookup kernel -- ffat_lookup_kernel,
ffat_lookup_runs_kernel, ffat_lookup_shared_kernel, both branches of ffat_batch_kernel -- and the host's transposition
(build_ffat_shared), bit for bit against the C oracle, which tests/test_oracle_ffat_boxes.py holds bit for bit to an
independent numpy restatement on the same boxes and positions.  The one undefined position, the map's centre, is in no test."""
import functools
import os

import numpy as np
import pytest

from openpbso_amd import ForceMessage, capi, synth
from openpbso_amd.solver import Engine
from oracle import oracle_py as orc
from tests import ffat_boxes as fb
from tests.scenarios import ObjSpec, _oracle_maps, force_ev, run_engine, run_oracle

pytestmark = pytest.mark.gpu


def _oracle_rows(lam, omaps, pos, n_modes=None):
    """computeTransfer(pos, T*) of the oracle for every position: [n_pos][n_maps]"""
    s = orc.Solver(lam, synth.RHO, synth.ALPHA, synth.BETA, n_modes=n_modes)
    s.read_ffat_maps(omaps)
    rows = []
    for p in pos:
        rc, row = s.compute_transfer_out(p, s.n)
        assert rc == 1
        rows.append(row)
    s.close()
    return np.array(rows)


# ---------------------------------------------------------------------------------------------------------------------------
# compute_transfer_batch
BATCH_MODES = {"A": 48, "B": 48, "C": 48, "D": 48, "E": 5, "F": 5}


@functools.lru_cache(maxsize=None)
def _batch_case(name):
    n = BATCH_MODES[name]
    lam = synth.eigenvalues(n, 300 + ord(name))
    maps = fb.named_box_maps(name, lam, 310 + ord(name))
    pos = np.concatenate([fb.edge_positions(maps[0]), fb.random_positions(maps[0], 200, 320 + ord(name))])
    want = _oracle_rows(lam, _oracle_maps(maps), pos)
    want.setflags(write=False)
    return lam, maps, pos, want


@pytest.mark.parametrize("shared", ["1", "0"])
@pytest.mark.parametrize("name", sorted(BATCH_MODES))
def test_transfer_batch_on_boxes_is_bit_exact(monkeypatch, name, shared):
    """PBSO_FFAT_SHARED=1: ffat_lookup_shared_kernel over the transposed maps; 0: ffat_batch_kernel, box E (7 440 cells) read in
    place, F (7 136) and the others staged in LDS"""
    monkeypatch.setenv("PBSO_FFAT_SHARED", shared)
    lam, maps, pos, want = _batch_case(name)
    assert (fb.n_cells(maps[0]) > 7168) == (name == "E")
    with Engine() as eng:
        oid = eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA)
        eng.set_ffat_maps(oid, maps)
        eng.finalize()
        ok, got = eng.compute_transfer_batch(oid, pos, len(lam))
    assert ok
    assert np.isfinite(got).all() and (want > 0).all()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, shared, len(bad), pos[bad[0][0]].tolist(), int(bad[0][1]), got[tuple(bad[0])], want[tuple(bad[0])])


# ---------------------------------------------------------------------------------------------------------------------------
# lookups inside a step
SIZES = [300, 65, 130, 2, 17, 1]
N_POS = 84                                  # positions per object: 84 one-buffer steps, or 7 steps of 12


def _box_at(name, center):
    extent, cell, _ = fb.BOXES[name]
    return fb.box_geometry(center, cell, extent, fb.SHIFT)


@functools.lru_cache(maxsize=None)
def _scene():
    """0: 300 modes on box A (a second 256-mode tile of the shared kernel, pitch 304); 1: 65 on B; 2: 130 on D; 3: 2 on C (the
    smallest shared object); 4: 17 modes over three boxes in turn (A, and B's and D's shapes about A's centre): the general
    kernels; 5: one mode: nothing to share.  Positions: fb.step_positions of the object's box (object 4: of its three, in turn)."""
    lams = [synth.eigenvalues(n, 400 + i) for i, n in enumerate(SIZES)]
    maps = [fb.named_box_maps(name, lams[i], 410 + i) for i, name in enumerate("ABDC")]
    ca = fb.BOXES["A"][2]
    three = [_box_at("A", ca), _box_at("B", ca), _box_at("D", ca)]
    m4 = fb.named_box_maps("A", lams[4], 414)
    for m in m4:
        m.update(three[m["mode_id"] % 3])
        m["psi"] = np.resize(m["psi"], fb.n_cells(m))                # (box A's 62 values cut or repeated to the box's cell count)
    maps.append(m4)
    maps.append(fb.named_box_maps("D", lams[5], 415))
    pos = [fb.step_positions(maps[i][0], N_POS) for i in range(4)]
    each = [fb.step_positions(g, N_POS, seed=5 + j) for j, g in enumerate(three)]
    pos.append(np.array([each[t % 3][t] for t in range(N_POS)]))
    pos.append(fb.step_positions(maps[5][0], N_POS))
    want = [_oracle_rows(lams[i], _oracle_maps(maps[i]), pos[i]) for i in range(len(SIZES))]
    for w in want:
        w.setflags(write=False)
    return lams, maps, pos, want


def _run_scene(monkeypatch, shared, steps, **select):
    monkeypatch.setenv("PBSO_FFAT_SHARED", "1" if shared else "0")
    lams, maps, pos, _ = _scene()
    total = sum(steps)
    assert total == N_POS
    with Engine(**select) as eng:
        for i, n in enumerate(SIZES):
            eng.add_object(lams[i], synth.RHO, synth.ALPHA, synth.BETA)
            eng.set_ffat_maps(i, maps[i])
        eng.finalize()
        rng = np.random.default_rng(5)
        for i, n in enumerate(SIZES):
            assert eng.enqueue_force(i, ForceMessage(data=rng.standard_normal(n) * 1e-3), 0)
            assert eng.compute_transfer_path(np.full(total, i, dtype=np.int32), pos[i], np.arange(total, dtype=np.int64)).all()
        audio, latest = [], []
        for nb in steps:
            eng.step(nb)
            audio.append(eng.audio().copy())
            latest.append([eng.latest_transfer(i).copy() for i in range(len(SIZES))])
        return audio, latest, eng.info()


def _check_scene(monkeypatch, steps, select):
    _, _, pos, want = _scene()
    a_audio, a_latest, a_info = _run_scene(monkeypatch, True, steps, **select)
    b_audio, b_latest, b_info = _run_scene(monkeypatch, False, steps, **select)
    # objects 0..3 through the shared kernel, 4 and 5 through the general ones -- in the same launches; or all six through the general ones
    assert a_info["total_ffat_shared_events"] == 4 * N_POS and a_info["total_ffat_general_events"] == 2 * N_POS
    assert b_info["total_ffat_shared_events"] == 0 and b_info["total_ffat_general_events"] == 6 * N_POS
    done = 0
    for k, nb in enumerate(steps):
        done += nb
        assert np.isfinite(a_audio[k]).all()
        assert np.array_equal(a_audio[k], b_audio[k]), k
        for i, n in enumerate(SIZES):
            assert np.array_equal(a_latest[k][i], b_latest[k][i]), (k, i)
            assert np.array_equal(a_latest[k][i][:n], want[i][done - 1]), (k, i, pos[i][done - 1].tolist())      # bit for bit
    assert max(np.abs(a).max() for a in a_audio) > 0


@pytest.mark.parametrize("select", [{}, dict(time_chunks=-1), dict(bank_kernel=2)])
def test_one_listener_event_per_object_and_step(monkeypatch, select):
    """84 one-buffer steps, every object's listener at another edge position in each: the shared kernel and ffat_lookup_kernel
    (one event per run), then everything through ffat_lookup_kernel; rows against the oracle after every step"""
    _check_scene(monkeypatch, [1] * N_POS, select)


@pytest.mark.parametrize("select", [{}, dict(time_chunks=-1), dict(bank_kernel=2)])
def test_a_path_of_twelve_positions_per_object_in_one_step(monkeypatch, select):
    """7 steps of 12 buffers, a position per buffer: runs of 12 events per object, so ffat_lookup_runs_kernel for the general
    objects (and for all six with PBSO_FFAT_SHARED=0).  The rows in force at the end of each step -- an axis-aligned listener at
    the end of the first six -- against the oracle; the rows in between through the audio, equal between the two kernels."""
    _check_scene(monkeypatch, [12] * (N_POS // 12), select)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["1", "0"])
@pytest.mark.parametrize("later", ["same", "other"])
def test_a_replaced_map(monkeypatch, later, shared):
    """mode 3 twice in the list handed to set_ffat_maps, over two different boxes: the later entry wins (std::map), its Psi behind
    every other map's in the object's pool and the first one's left there unused.  later == "same": the entry that wins lies
    over the box of the other modes, so the object shares one geometry; "other": it does not, so the general kernels."""
    monkeypatch.setenv("PBSO_FFAT_SHARED", shared)
    n = 20
    lam = synth.eigenvalues(n, 500)
    maps = fb.named_box_maps("A", lam, 501)
    odd = dict(fb.named_box_maps("D", lam, 502)[3], **_box_at("D", fb.BOXES["A"][2]))
    if later == "same":
        listed = maps[:3] + [odd] + maps[4:] + [maps[3]]
    else:
        listed = maps + [odd]
    assert [m["mode_id"] for m in listed].count(3) == 2 and len(listed) == n + 1
    pos = np.concatenate([fb.step_positions(maps[0], N_POS), fb.step_positions(odd, N_POS)])
    want = _oracle_rows(lam, _oracle_maps(listed), pos)
    final = maps[3] if later == "same" else odd
    alone = np.array([abs(orc.ffat_get_map_val(orc.ffat_map(final), p)) for p in pos])
    assert np.array_equal(want[:, 3], alone) and want.shape == (len(pos), n)
    with Engine() as eng:
        oid = eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA)
        eng.set_ffat_maps(oid, listed)
        eng.finalize()
        assert eng.n_maps(oid) == n
        ok, got = eng.compute_transfer_batch(oid, pos, n)
        assert ok and np.array_equal(got, want)
        latest = []
        for t in range(8):
            eng.compute_transfer(oid, pos[11 * t], t)
            eng.step(1)
            latest.append(eng.latest_transfer(oid).copy())
        info = eng.info()
    is_shared = later == "same" and shared == "1"
    assert info["total_ffat_shared_events"] == (8 if is_shared else 0) and info["total_ffat_general_events"] == (0 if is_shared else 8)
    for t in range(8):
        assert np.array_equal(latest[t], want[11 * t]), t


# ---------------------------------------------------------------------------------------------------------------------------
def test_mix_listeners_on_a_box_with_axis_aligned_listeners():
    """pbso_mix_listeners: one 130-mode object on box D heard by 5 listeners, two of them straight along an axis from the map's
    centre; test_gpu_listener_mix_edges.py's tolerance (5e-4 of the listener's peak), and nothing but finite samples"""
    from tests.test_gpu_listener_mix_edges import _oracle_per_listener
    n_modes, nb = 130, 4
    lam = synth.eigenvalues(n_modes, 600)
    maps = fb.named_box_maps("D", lam, 601)
    two, _ = fb.axis_positions(maps[0])
    rng = np.random.default_rng(6)
    d = rng.standard_normal((3, 3))
    pos = np.concatenate([np.asarray(maps[0]["center"]) + 0.4 * d / np.linalg.norm(d, axis=1, keepdims=True), two[[4, 3]]])      # +z, -y
    hits = {0: rng.standard_normal(n_modes) * 1e-3, 2: rng.standard_normal(n_modes) * 1e-3}
    with Engine(form=capi.FORM_BLOCK) as eng:
        oid = eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA)
        eng.set_ffat_maps(oid, maps)
        eng.finalize()
        eng.listeners_enable(oid)
        eng.compute_transfer(oid, pos[3], 0)
        for b, data in hits.items():
            assert eng.enqueue_force(oid, ForceMessage(data=data), b)
        eng.step(nb)
        single = eng.audio()[oid].astype(np.float64)
        mix = eng.mix_listeners(oid, pos).astype(np.float64)
    want = _oracle_per_listener(lam, _oracle_maps(maps), pos, nb, hits)
    assert np.isfinite(mix).all() and np.isfinite(single).all() and np.isfinite(want).all()
    for l in range(len(pos)):
        assert np.abs(want[l]).max() > 0
        assert np.abs(mix[l] - want[l]).max() <= 5e-4 * np.abs(want[l]).max(), l
    assert np.abs(single - want[3]).max() <= 5e-4 * np.abs(want[3]).max()


# ---------------------------------------------------------------------------------------------------------------------------
def test_end_to_end_audio_with_a_listener_crossing_an_axis_and_an_edge_diagonal():
    """4 objects x 64 modes on boxes A, B, D and a cube, 12 buffers of Poisson hits, the listener of each moving every buffer on
    an arc about the map's centre that stands exactly on the +z axis in buffer 5 and on the diagonal through the box's own
    +x+y edge in buffer 9 (outside the boxes throughout: the transfer stays in the scaled-state range).  The parity tests'
    tolerance on the audio, the transfer rows bit for bit."""
    from tests.test_gpu_parity import _check
    nb, n_modes = 12, 64
    objs, evs = [], []
    for i, name in enumerate(["A", "B", "D", None]):
        seed = 700 + i
        lam = synth.eigenvalues(n_modes, seed)
        maps = fb.named_box_maps(name, lam, seed) if name else synth.ffat_maps(lam, seed, dim=6, cell_size=0.012, center=(0.2, 0.1, -0.1))
        objs.append(ObjSpec(lam, shapes=synth.mode_shapes(n_modes, seed), maps=maps))
        vns = synth.unit_normals(nb, seed)
        for b, vid in enumerate(synth.poisson_hits(nb, seed, p=0.4)):
            if vid >= 0:
                evs.append(force_ev(b, i, vid=int(vid), vn=vns[b]))
        c = np.asarray(maps[0]["center"], dtype=np.float64)
        half = (np.asarray(maps[0]["bbox_top"]) - np.asarray(maps[0]["bbox_low"])) / 2
        for b in range(nb):
            a = 0.2 * (b - 5)
            off = 0.45 * np.array([np.sin(a), 0.3 * np.sin(a), np.cos(a)])
            if b == 9:
                off = 3 * half * np.array([1.0, 1.0, 0.0])
            p = c + off
            assert (np.abs(p - c) > half).any()
            if b == 5:
                assert p[0] == c[0] and p[1] == c[1] and p[2] > c[2]
            evs.append(dict(t=b, obj=i, kind="listener", pos=p))
    assert sum(e["kind"] == "force" for e in evs) >= 8
    got = run_engine(objs, evs, nb)
    want = run_oracle(objs, evs, nb)
    _check(got, want)
    assert np.abs(want["audio"]).max(axis=1).min() > 0
    for i in range(len(objs)):
        assert np.array_equal(got["latest"][i], want["latest"][i]), i


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", ["1", "0"])
def test_box_maps_from_fatcube_files(monkeypatch, tmp_path, shared):
    """a data directory whose <name>_ffat_maps/ holds box-A .fatcube files, through pbso_add_object_from_files; the oracle gets
    or_fatcube_parse of the same bytes"""
    monkeypatch.setenv("PBSO_FFAT_SHARED", shared)
    from tests.fatcube_codec import encode_fatcube, proto_classes
    from tests.test_headless_cli import make_data_dir
    d = tmp_path / "data"
    d.mkdir()
    lam, _ = make_data_dir(d, thr=20000.0)                       # (every mode audible: as many maps as modes)
    cls = proto_classes()
    maps = fb.named_box_maps("A", lam, 800)
    files = sorted(f for f in os.listdir(d / "bowl_ffat_maps") if f.endswith(".fatcube"))
    assert len(files) == len(maps)
    omaps = []
    for m in maps:
        data = encode_fatcube(cls, m)
        (d / "bowl_ffat_maps" / f"mode_{m['mode_id']:03d}.fatcube").write_bytes(data)
        rc, om = orc.fatcube_parse(data)
        assert rc == 0
        omaps.append(om)
    assert sorted(f for f in os.listdir(d / "bowl_ffat_maps") if f.endswith(".fatcube")) == files
    pos = np.concatenate([fb.edge_positions(maps[0]), fb.random_positions(maps[0], 100, 801)])
    want = _oracle_rows(lam, omaps, pos)
    with Engine() as eng:
        oid, naud = eng.add_object_from_files(str(d / "bowl_surf.modes"), str(d / "bowl_material.txt"), str(d / "bowl_ffat_maps"))
        assert naud == len(lam)
        eng.finalize()
        assert eng.n_maps(oid) == len(maps)
        ok, got = eng.compute_transfer_batch(oid, pos)
    assert ok and got.shape == want.shape
    assert np.array_equal(got, want)
