"""FFAT lookups (A7) on box-shaped maps and at edge listener positions, on the CPU: the C oracle's or_ffat_get_map_val against
the independent numpy restatement of test_oracle_crosschecks.py, bit for bit (a == b, no tolerance: every operation of
GetMapVal is a single IEEE double operation in both, in the same order), over tests/ffat_boxes.py's boxes and positions; the
helpers themselves against the committed non-uniform fixture; oracle_py.ffat_map against uniform_cube and the .fatcube codecs."""
import json
import os

import numpy as np
import pytest

from openpbso_amd import synth
from tests import ffat_boxes as fb
from tests.scenarios import is_uniform_cube, oracle_map
from tests.test_oracle_crosschecks import ffat_numpy

G = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GEOM_FIELDS = ["cell_size", "center3", "center", "bbox_low", "bbox_top", "low_corners", "n_elements", "strides"]


def _positions(geom, seed):
    return np.concatenate([fb.edge_positions(geom), fb.random_positions(geom, 300, seed)])


def test_box_geometry_reproduces_the_golden_nonuniform_map():
    want = json.load(open(os.path.join(G, "fatcubes.json")))["fat_nonuniform_mode7.fatcube"]
    extent, cell, center = fb.BOXES["A"]
    got = fb.box_geometry(center, cell, extent, center3_shift=0.001)
    for f in GEOM_FIELDS:
        assert np.array_equal(np.asarray(got[f], dtype=np.float64), np.asarray(want[f], dtype=np.float64)), f
    assert fb.n_cells(got) == len(want["psi"])
    # and the uniform cube is the special case: an even cube of the box helper is the synthetic generator's cube
    cube = synth.uniform_cube_geometry((0.1, -0.2, 0.3), 0.01, 6)
    box = fb.box_geometry((0.1, -0.2, 0.3), 0.01, (6, 6, 6))
    for f in GEOM_FIELDS:
        assert np.array_equal(np.asarray(box[f], dtype=np.float64), np.asarray(cube[f], dtype=np.float64)), f


@pytest.mark.parametrize("name", sorted(fb.BOXES))
def test_edge_positions_cover_what_they_claim(name):
    extent, cell, center = fb.BOXES[name]
    g = fb.box_geometry(center, cell, extent, fb.SHIFT)
    c = np.asarray(center)
    half = np.asarray(extent) * cell / 2
    two, one = fb.axis_positions(g)
    assert ((two - c == 0).sum(axis=1) == 2).all() and len(two) == 6
    assert ((one - c == 0).sum(axis=1) == 1).all() and len(one) == 12
    inside = fb.inside_positions(g)
    assert len(inside) == 60 and (np.abs(inside - c) <= 0.95 * half).all()
    pos = fb.edge_positions(g)
    assert not (pos == c).all(axis=1).any()
    # the lattice listeners: every face is entered, and on each face both clamp branches, tx == 0 and the interior occur
    m = dict(g, mode_id=0, k=1.0, psi=np.arange(fb.n_cells(g), dtype=np.float64) + 1.0)
    seen = {}
    for p in fb.lattice_positions(g):
        face, xf, yf = _locate(m, p)
        seen.setdefault(face, []).append((xf, yf))
    assert sorted(seen) == [0, 1, 2, 3, 4, 5]
    for face, pts in seen.items():
        nx, ny = g["n_elements"][face]
        for vals, n in ((np.array([v[0] for v in pts]), nx), (np.array([v[1] for v in pts]), ny)):
            assert (np.floor(vals) < 0).any() and (np.floor(vals) >= n - 1).any(), (face, n)
            frac = np.abs(vals - np.round(vals))
            assert (frac < 1e-6).any()                                        # a cell centre: tx or ty 0 (to rounding)
            if n > 1:
                inner = (np.floor(vals) >= 0) & (np.floor(vals) < n - 1)
                assert inner.any() and (frac[inner] > 0.4).any()              # a cell border between two cells


def _locate(m, p):
    """the face and the fractional cell coordinates of ffat_numpy, restated for the coverage check above"""
    low, top = np.asarray(m["bbox_low"]), np.asarray(m["bbox_top"])
    d = np.asarray(m["center"]) - p
    with np.errstate(divide="ignore", invalid="ignore"):
        t_en = np.minimum((low - p) / d, (top - p) / d).max()
    surf = p + t_en * d
    best, face = np.inf, -1
    for dd in range(3):
        for cand, f in ((abs(low[dd] - surf[dd]), 2 * dd + 1), (abs(top[dd] - surf[dd]), 2 * dd)):
            if cand < best:
                best, face = cand, f
    dk = face // 2
    di, dj = (dk + 1) % 3, (dk + 2) % 3
    h = m["cell_size"]
    lc = np.asarray(m["low_corners"][face])
    return face, (surf[di] - (lc[di] + 0.5 * h)) / h, (surf[dj] - (lc[dj] + 0.5 * h)) / h


@pytest.mark.parametrize("name", sorted(fb.BOXES))
def test_ffat_lookup_oracle_vs_numpy_restatement_on_boxes(oracle, name):
    """bit equality, and a finite value, at every edge position and 300 seeded random ones"""
    lam = synth.eigenvalues(2, 50 + ord(name))
    for m in fb.named_box_maps(name, lam, 60 + ord(name)):
        assert not is_uniform_cube(m)
        om = oracle.ffat_map(m)
        for p in _positions(m, 70 + ord(name) + m["mode_id"]):
            a = oracle.ffat_get_map_val(om, p)
            b = ffat_numpy(m, p)
            assert np.isfinite(a) and a == b, (name, m["mode_id"], p.tolist(), a, b)


def test_box_lookup_tells_nx_from_ny_and_face_from_face(oracle):
    """Psi = the cell's own flat index + 1: at a cell centre the lookup returns exactly that cell (weights 1, 0, 0, 0), so the
    test's own restatement is anchored to the layout psi[stride[f] + x * Ny + y] and not only to the oracle"""
    extent, cell, center = fb.BOXES["D"]
    g = fb.box_geometry(center, cell, extent)                    # (center3 == center: r is the distance to the centre)
    m = dict(g, mode_id=0, k=1.0, psi=np.arange(fb.n_cells(g), dtype=np.float64) + 1.0)
    om = oracle.ffat_map(m)
    c = np.asarray(center)
    for face in range(6):
        dk = face // 2
        di, dj = (dk + 1) % 3, (dk + 2) % 3
        nx, ny = g["n_elements"][face]
        assert (nx, ny) == (extent[di], extent[dj]) and nx != ny
        for x in range(nx):
            for y in range(ny):
                q = np.zeros(3)
                q[dk] = g["low_corners"][face][dk]
                q[di] = g["low_corners"][face][di] + (x + 0.5) * cell
                q[dj] = g["low_corners"][face][dj] + (y + 0.5) * cell
                p = c + 2.5 * (q - c)
                want = (g["strides"][face] + x * ny + y + 1.0) / np.linalg.norm(p - c)
                for val in (oracle.ffat_get_map_val(om, p), ffat_numpy(m, p)):
                    assert abs(val - want) <= 1e-9 * want, (face, x, y, val, want)


def test_ffat_map_of_a_uniform_cube_equals_uniform_cube(oracle):
    lam = synth.eigenvalues(3, 81)
    for m in synth.ffat_maps(lam, 81, dim=6, cell_size=0.012, center=(0.02, -0.01, 0.03)):
        assert is_uniform_cube(m)
        a = oracle.ffat_map(m)
        b = oracle.uniform_cube(m["mode_id"], m["k"], m["center"], m["cell_size"], 6, m["psi"])
        for name, _ in oracle.OrFfatMap._fields_:
            if name == "psi":
                assert np.array_equal(oracle.map_psi(a), oracle.map_psi(b))
            elif name in ("low_corners", "n_elements"):
                assert [list(r) for r in getattr(a, name)] == [list(r) for r in getattr(b, name)], name
            elif name in ("center3", "center", "bbox_low", "bbox_top", "strides"):
                assert list(getattr(a, name)) == list(getattr(b, name)), name
            else:
                assert getattr(a, name) == getattr(b, name), name
        for p in _positions(m, 82):
            assert oracle.ffat_get_map_val(a, p) == oracle.ffat_get_map_val(b, p) == oracle.ffat_get_map_val(oracle_map(m), p)


def test_box_map_through_the_fatcube_codecs(oracle):
    """encode_fatcube -> or_fatcube_parse gives the values of ffat_map(m); the engine's parse_fatcube returns the same fields"""
    from openpbso_amd import capi
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    from openpbso_amd import loaders
    from tests.fatcube_codec import encode_fatcube, proto_classes
    cls = proto_classes()
    lam = synth.eigenvalues(3, 91)
    for m in fb.named_box_maps("A", lam, 91):
        data = encode_fatcube(cls, m)
        rc, parsed = oracle.fatcube_parse(data)
        assert rc == 0
        direct = oracle.ffat_map(m)
        for p in _positions(m, 92):
            assert oracle.ffat_get_map_val(parsed, p) == oracle.ffat_get_map_val(direct, p)
        got = loaders.parse_fatcube(data)
        assert got["mode_id"] == m["mode_id"] and got["k"] == m["k"]
        for f in GEOM_FIELDS + ["psi"]:
            assert np.array_equal(np.asarray(got[f], dtype=np.float64), np.asarray(m[f], dtype=np.float64)), f
