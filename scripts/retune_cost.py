"""What one pbso_set_material over ALL objects of an engine costs, beside the only other way to the same tables: destroy the engine,
add every object again, finalize.

Shapes: 1024 x 512 modes with 256-vertex mode shapes (the g32 rebuild dominates: 12 B per (dof, mode)), and 128 x 512 without shapes
(the tables kernel alone).  Per shape: the wall time of the call (median of --reps), the HIP-event time of each kernel (the library
records them with PBSO_RETUNE_TIMING=1 and reports them on stderr), retune_g32_kernel's time beside its byte bound at --hbm-gbs, and the
wall time of create + add + finalize at the same shape.

    python scripts/retune_cost.py [--reps 5] [--hbm-gbs 8000] [--out profiles/retune.txt]
"""
import argparse
import os
import re
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1024, 512, 256), (128, 512, 0)]


def child(n_obj, n_modes, n_verts, reps):
    sys.path.insert(0, ROOT)
    import numpy as np
    from openpbso_amd import Engine, capi, synth
    lams = [synth.eigenvalues(n_modes, 9000 + i) for i in range(n_obj)]
    shape = synth.mode_shapes(n_modes, 9000, n_verts) if n_verts else None      # (one array for all objects: the upload is what counts)

    def build():
        eng = Engine(form=capi.FORM_BLOCK, qnorm=capi.QNORM_OFF)
        for lam in lams:
            eng.add_object(lam, synth.RHO, synth.ALPHA, synth.BETA, mode_shapes=shape)
        eng.finalize()
        eng.sync()
        return eng

    t0 = time.perf_counter()
    eng = build()
    first_build = time.perf_counter() - t0
    ids = list(range(n_obj))
    walls = []
    for r in range(reps + 1):                                # (the first call grows the upload buffers: not timed)
        eng.step(1)
        eng.sync()
        t0 = time.perf_counter()
        eng.set_material(ids, 1900.0 + r, 25.0, 3e-7)
        walls.append(time.perf_counter() - t0)
    stats = eng.material_stats()
    m_pad = eng.info()["modes_padded"]
    rebuilds = []
    for _ in range(max(1, min(reps, 2))):
        t0 = time.perf_counter()
        eng.close()
        eng = build()
        rebuilds.append(time.perf_counter() - t0)
    eng.close()
    print(f"RESULT wall_ms {1e3 * float(np.median(walls[1:])):.4f} rebuild_ms {1e3 * float(np.median(rebuilds)):.3f} first_build_ms {1e3 * first_build:.3f} "
          f"m_pad {m_pad} g32_elems {stats[3] // stats[0] if stats[0] else 0}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hbm-gbs", type=float, default=8000.0, help="the HBM rate the byte bound is priced at (GB/s)")
    ap.add_argument("--out", default="")
    ap.add_argument("--child", nargs=3, type=int)
    a = ap.parse_args()
    if a.child:
        child(*a.child, a.reps)
        return
    lines = []
    for n_obj, n_modes, n_verts in SHAPES:
        # a fresh process per shape: the kernels' HIP-event times come back on its stderr
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--reps", str(a.reps), "--child", str(n_obj), str(n_modes), str(n_verts)],
                           capture_output=True, text=True, env=dict(os.environ, PBSO_RETUNE_TIMING="1"), timeout=900)
        if r.returncode != 0:
            sys.exit(r.stdout + r.stderr)
        res = dict(zip(*[iter(re.search(r"RESULT (.*)", r.stdout).group(1).split())] * 2))
        ev = re.findall(r"pbso retune: tables kernel ([0-9.]+) ms, g32 kernel ([0-9.]+) ms", r.stderr)[1:]
        tables = sorted(float(x) for x, _ in ev)[len(ev) // 2]
        g32 = sorted(float(y) for _, y in ev)[len(ev) // 2]
        elems = int(res["g32_elems"])
        bound_ms = 12.0 * elems / (a.hbm_gbs * 1e9) * 1e3
        lines.append(f"{n_obj} x {n_modes} modes, {n_verts} vertices (m_pad {res['m_pad']}): pbso_set_material over all objects "
                     f"{float(res['wall_ms']):.3f} ms wall | retune_tables_kernel {tables:.4f} ms (latency-bound chain, no roof) | "
                     f"retune_g32_kernel {g32:.4f} ms for {12.0 * elems / 1e9:.3f} GB, bound {bound_ms:.4f} ms at {a.hbm_gbs:.0f} GB/s"
                     + (f" ({100.0 * bound_ms / g32:.0f} % of it)" if g32 > 0 and elems else "")
                     + f" | destroy + add + finalize {float(res['rebuild_ms']):.1f} ms wall")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
