"""FFAT maps over a BOX (test infrastructure only): the reference's ordinary map constructor (ffat_solver.h:406-437) lays a box
around the object with its own (first, second) cell count on each pair of faces -- what a plate's or a glass's .fatcube files
hold.  synth.uniform_cube_geometry is its special case (ResampleToUniformCube): Nx == Ny on every face, strides f * dim^2, a box
symmetric about its centre and center3 == center, under which a swapped Nx / Ny, a swapped di / dj, the wrong face's n_elements
or stride and the wrong clamp bound all go unseen.  Here: the box geometry, maps over it, and the listener positions at which
the lookup's arithmetic is IEEE-defined but unusual (zero direction components, ties, cell borders, the inside of the box)."""
import numpy as np

from openpbso_amd import synth

# the boxes of the tests: extent in cells (x, y, z), cell size, centre; each used with center3 = center + SHIFT
SHIFT = 0.0007
BOXES = {
    "A": ((5, 3, 2), 0.02, (0.1, -0.2, 0.05)),        # the shape of tests/golden/fat_nonuniform_mode7.fatcube
    "B": ((5, 3, 1), 0.02, (0.1, -0.2, 0.05)),        # faces one cell wide: one axis always clamps (Nx - 1 == 0)
    "C": ((1, 1, 1), 0.05, (0.0, 0.0, 0.0)),          # six single-cell faces
    "D": ((2, 7, 4), 0.013, (-1.0, 2.0, 0.5)),        # every Nx != Ny
    "E": ((40, 36, 30), 0.004, (0.3, 0.1, -0.2)),     # 7 440 cells: over the batch kernel's LDS window of 7 168 doubles
    "F": ((40, 36, 28), 0.004, (0.3, 0.1, -0.2)),     # 7 136 cells: just under it
}
DIAGONALS = ((1, 1, 0), (1, -1, 0), (0, 1, 1), (1, 0, -1), (1, 1, 1), (-1, -1, -1), (1, -1, 1), (-1, 1, 1))


def box_geometry(center, cell_size, extent_xyz, center3_shift=0.0):
    """The runtime fields of a map over a box of extent_xyz cells around `center`, as the reference's constructor lays them out:
    face dd (normal axis dk = dd // 2, + side for even dd) has n_elements (extent[di], extent[dj]) with di = (dk + 1) % 3 and
    dj = (dk + 2) % 3, its low corner at center - half with component dk moved to +-half[dk], strides the running sum of
    Nx * Ny, and bbox_low / bbox_top the min / max of the corners.  center3 (FFAT_Map<T,3>::_center, the origin of the 1 / r
    decay) = center + center3_shift."""
    center = np.asarray(center, dtype=np.float64)
    extent = np.asarray(extent_xyz, dtype=np.int64)
    half = extent * cell_size / 2
    ne = np.zeros((6, 2), dtype=np.int32)
    low = np.zeros((6, 3))
    for dd in range(6):
        dk = dd // 2
        di, dj = (dk + 1) % 3, (dk + 2) % 3
        ne[dd] = (extent[di], extent[dj])
        low[dd] = center - half
        low[dd, dk] = center[dk] + (half[dk] if dd % 2 == 0 else -half[dk])
    cells = ne[:, 0].astype(np.int64) * ne[:, 1]
    return {
        "cell_size": cell_size, "low_corners": low, "n_elements": ne,
        "strides": np.concatenate([[0], np.cumsum(cells)[:-1]]).astype(np.int32), "center": center.copy(),
        "center3": center + center3_shift, "bbox_low": low.min(axis=0), "bbox_top": low.max(axis=0),
    }


def n_cells(geom):
    ne = np.asarray(geom["n_elements"], dtype=np.int64)
    return int((ne[:, 0] * ne[:, 1]).sum())


def box_maps(lam, seed, extent_xyz=(5, 3, 2), cell_size=0.02, center=(0.1, -0.2, 0.05), center3_shift=SHIFT):
    """One map per mode over the same box (synth.ffat_maps' counterpart, the same Psi scale: |N(0,1)| * 1e7 * k * 0.5)."""
    rng = np.random.default_rng(seed + 32452843)
    omega = np.sqrt(np.asarray(lam) / synth.RHO)
    maps = []
    for m, om in enumerate(omega):
        g = box_geometry(center, cell_size, extent_xyz, center3_shift)
        g["mode_id"] = m
        g["k"] = om / synth.SPEED_OF_SOUND
        g["psi"] = np.abs(rng.standard_normal(n_cells(g))) * 1e7 * g["k"] * 0.5
        maps.append(g)
    return maps


def named_box_maps(name, lam, seed):
    extent, cell, center = BOXES[name]
    return box_maps(lam, seed, extent, cell, center)


def axis_positions(geom):
    """listeners straight along an axis from the map's centre (two zero components of centre - p: +-inf lanes that the max over
    the three entry parameters discards), and the same with one further component off the axis (one zero component)"""
    c = np.asarray(geom["center"], dtype=np.float64)
    half = (np.asarray(geom["bbox_top"]) - np.asarray(geom["bbox_low"])) / 2
    two, one = [], []
    for a in range(3):
        for sign in (1.0, -1.0):
            p = c.copy()
            p[a] = c[a] + sign * (3 * half[a] + 0.1)
            two.append(p)
            for b in range(3):
                if b != a:
                    q = p.copy()
                    q[b] = c[b] + 0.37 * half[b]
                    one.append(q)
    return np.array(two), np.array(one)


def diagonal_positions(geom):
    """face and body diagonals: centre + 3 s * half sends the ray through the box's own edges and corners, centre + 0.4 s along
    the unit diagonals; both tie in t_enter and in the nearest-plane pick"""
    c = np.asarray(geom["center"], dtype=np.float64)
    half = (np.asarray(geom["bbox_top"]) - np.asarray(geom["bbox_low"])) / 2
    s = np.array(DIAGONALS, dtype=np.float64)
    return np.concatenate([c + s * half * 3, c + 0.4 * s])


LATTICE_FULL = 100         # faces with at most this many half-cell lattice points get all of them


def lattice_positions(geom):
    """For every face, listeners at centre + 2.5 q for surface points q (relative to the centre) on the face's half-cell lattice
    (even steps: cell borders, odd steps: cell centres, where tx or ty is 0).  A small face gets the whole lattice; a large one a
    walk, step t at half-cell t along di and half-cell 2 t + 1 along dj (both wrap; 2 is coprime to the odd lattice length, so
    either axis sees every centre and border).  The lattice's outermost points lie on the box's edges, where the nearest-plane
    pick ties and hands them to the neighbouring face, so each face also gets four points a quarter cell inside its borders:
    the first and the last half cell of either axis -- both clamp branches -- on the face itself."""
    out = []
    for dd in range(6):
        nx, ny = (int(v) for v in geom["n_elements"][dd])
        lx, ly = 2 * nx + 1, 2 * ny + 1
        if lx * ly <= LATTICE_FULL:
            steps = [(0.5 * i, 0.5 * j) for i in range(lx) for j in range(ly)]
        else:
            steps = [(0.5 * (t % lx), 0.5 * ((2 * t + 1) % ly)) for t in range(max(lx, ly))]
        out += [_through(geom, dd, u, v) for u, v in steps]
    return np.concatenate([np.array(out), border_positions(geom)])


def _through(geom, dd, u, v):
    """the listener at centre + 2.5 q for the point q of face dd that lies u cells along di and v cells along dj from its corner"""
    c = np.asarray(geom["center"], dtype=np.float64)
    h = float(geom["cell_size"])
    dk = dd // 2
    lc = np.asarray(geom["low_corners"][dd], dtype=np.float64)
    q = np.zeros(3)
    q[dk] = lc[dk]
    q[(dk + 1) % 3] = lc[(dk + 1) % 3] + h * u
    q[(dk + 2) % 3] = lc[(dk + 2) % 3] + h * v
    return c + 2.5 * (q - c)


def border_positions(geom):
    """four listeners per face through points a quarter cell inside its four borders, halfway along the other axis: on every
    face, for either axis, the branch x < 0 and the branch x >= Nx - 1 of Interpolate"""
    out = []
    for dd in range(6):
        nx, ny = (int(v) for v in geom["n_elements"][dd])
        mx, my = nx // 2 + 0.5, ny // 2 + 0.5
        out += [_through(geom, dd, u, v) for u, v in ((0.25, my), (nx - 0.25, my), (mx, 0.25), (mx, ny - 0.25))]
    return np.array(out)


def step_positions(geom, n, seed=3):
    """n >= 72 edge positions for tests that spend a launch per position: the 6 + 12 axis-aligned ones, the 16 diagonals, the 24
    border points (every face, both clamp branches of either axis), 6 points inside the box and a seeded choice from the
    lattice for the rest.  The two-zero axis positions stand at indices 11, 23, ..., 71 (the last of a run of twelve)."""
    two, one = axis_positions(geom)
    lat = lattice_positions(geom)[:-24]
    rng = np.random.default_rng(seed)
    assert n >= 72
    fill = lat[rng.choice(len(lat), n - 64, replace=len(lat) < n - 64)]
    rest = list(np.concatenate([one, diagonal_positions(geom), border_positions(geom), inside_positions(geom)[:6], fill]))
    out = []
    for t in two:
        out += rest[:11] + [t]
        rest = rest[11:]
    return np.array(out + rest)


def inside_positions(geom, n=60, seed=9):
    c = np.asarray(geom["center"], dtype=np.float64)
    half = (np.asarray(geom["bbox_top"]) - np.asarray(geom["bbox_low"])) / 2
    rng = np.random.default_rng(seed)
    return c + 0.95 * half * rng.uniform(-1.0, 1.0, (n, 3))


def edge_positions(geom):
    """The listener positions the rest of the suite steers clear of, all with IEEE-defined arithmetic in GetMapVal: axis-aligned
    (axis_positions), diagonals (diagonal_positions), cell centres and borders (lattice_positions) and 60 seeded points inside
    the box (within 0.95 of the half-extents).

    Never the map's centre itself: there centre - p is zero in all three lanes, t_enter is -inf, the surface point NaN and
    (int)floor(NaN) undefined in C -- the one position the reference leaves undefined, and out of every test."""
    two, one = axis_positions(geom)
    pos = np.concatenate([two, one, diagonal_positions(geom), lattice_positions(geom), inside_positions(geom)])
    assert not (pos == np.asarray(geom["center"], dtype=np.float64)).all(axis=1).any()
    return pos


def random_positions(geom, n, seed):
    """seeded positions around the box, a normal cloud two half-diagonals wide: inside and outside alike (never the centre)"""
    c = np.asarray(geom["center"], dtype=np.float64)
    half = (np.asarray(geom["bbox_top"]) - np.asarray(geom["bbox_low"])) / 2
    rng = np.random.default_rng(seed)
    return c + rng.standard_normal((n, 3)) * 2 * np.linalg.norm(half)
