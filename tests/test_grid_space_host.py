"""The grid space (tests/grid_cases.py) on the CPU: every case's conditions hold on the oracle's output alone, and
the device state machine run through the host simulator equals the oracle bit for bit on every case -- records, film,
debug counters, no walk-table lookup outside the padded table -- so a GPU comparison on these inputs
(tests/test_gpu_grid_space.py) compares non-trivial work with a reference the shared __host__ __device__ code already
meets.  For the extra subset also the pixel-RNG mode.

On the density (and temperature) grids with a non-zero background or denormal values: the direct-addressed stencil
pool's host expansion (tests/native/dense_pool_host.cpp) checks itself against cell_at / fetch_stencil over the whole
table, and bricks it dumps are compared with hostsim's probe() voxel by voxel.  The coverage pass's host march
(tests/alpha_lib.py) runs every case's frame at sub 1: tau finite and >= 0, alpha = 1 - exp(-tau).  Its float64
restatements of the optical depth (tests/analytic_anchor.py: cube_od, optical_depth) know the constant cube and the
sparse anchor grid only and take no other grid, so that comparison is not made here.
"""
import subprocess

import numpy as np
import pytest

import alpha_lib as AL
import dense_pool_lib as DP
import grid_cases as GC
import hostsim_lib as HS
from volume_path_tracer_amd import capi


@pytest.mark.parametrize("case_id", GC.IDS)
def test_case_conditions_hold_on_the_oracle(case_id):
    GC.check_case(case_id)


@pytest.mark.parametrize("case_id", GC.IDS)
def test_host_simulator_equals_the_oracle(case_id):
    ref = GC.check_case(case_id)
    HS.walk_outside(reset=True)
    f_h, r_h, c_h = HS.render_jobs(ref.cfg, ref.dens, ref.temp, 0, ref.jobs, records=True)
    assert r_h.tobytes() == ref.rec.tobytes(), "per-sample radiance differs"
    assert f_h.tobytes() == ref.film.tobytes()
    for k in GC.DEBUG_COUNTERS + (("temp_stencils",) if ref.temp is not None else ()):
        assert c_h[k] == ref.counters[k], (k, c_h[k], ref.counters[k])
    assert HS.walk_outside() == 0


@pytest.mark.parametrize("case_id", GC.EXTRA_IDS)
def test_host_simulator_pixel_rng_mode_equals_the_oracle(case_id):
    ref = GC.check_case(case_id)
    f_o, r_o = ref.pixel_mode()
    f_h, r_h, c_h = HS.render_jobs(ref.cfg, ref.dens, ref.temp, 0, ref.jobs, records=True, rng_mode=capi.VPT_RNG_PIXEL)
    assert r_h.tobytes() == r_o.tobytes()
    assert r_o.tobytes() != ref.rec.tobytes() or case_id == "tiles_only"  # (another RNG stream: other samples)
    assert f_h.tobytes() == f_o.tobytes()
    assert c_h["samples"] == ref.counters["samples"]


# ---- the dense pool's host expansion -------------------------------------------------------------------------
def _pool_grids():
    """(name, grid) of every grid of the table with a non-zero background or denormal values."""
    out = []
    for cid in GC.IDS:
        _, dens, temp = GC.BY_ID[cid].build()
        for which, g in (("density", dens), ("temperature", temp)):
            if g is None:
                continue
            v = np.abs(g.leaf_values)
            tiny = ((v > 0) & (v < GC.DENORMAL_MIN_NORMAL)).any()
            if g.desc.background != 0.0 or tiny:
                out.append((f"{cid}/{which}", g))
    return out


def _table(g):
    """(origin, (nx, ny, nz) in cells) of the cells8 table: the bounding box of the grid's lower nodes."""
    org = [g.leaf_origin]
    if g.tile_origin is not None:
        org.append(g.tile_origin[np.asarray(g.tile_level) == 1])
    lower = np.concatenate(org) >> 7
    return lower.min(0) * 128, (lower.max(0) - lower.min(0) + 1) * 16


def test_dense_pool_host_expansion_on_backgrounds_and_denormals(tmp_path):
    """dense_pool_host's own check over every cell and voxel (the dense stencil against fetch_stencil through
    cell_at, uint32), then dumped bricks against probe(): the table's first and last cell (cells without a leaf: the
    background, and the apron past the table), a cell in the cloud's middle, one in the denormal slab and the cell of
    the lower-node tile at (64, 0, 0) where the table holds one.  A brick is [y 8][z 8][x 9][4]: corner q of voxel
    (x, y, z) is the value at (x, y + (q >> 1), z + (q & 1))."""
    grids = _pool_grids()
    names = [n for n, _ in grids]
    assert {"background=+0.05/density", "background=-0.05/density", "bbox_loose+background/density",
            "root_edge+background/density", "denormal:40/density", "denormal:5000/density", "denormal:max/density",
            "temp:background/temperature"} == set(names), names
    exe = DP.build_program()
    files = [DP.write_grid(tmp_path / f"g{n}.grid", g) for n, (_, g) in enumerate(grids)]
    r = subprocess.run([str(exe), *map(str, files)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "dense_pool_host ok" in r.stdout and "FAIL" not in r.stdout
    y, z, x, q = np.meshgrid(np.arange(8), np.arange(8), np.arange(9), np.arange(4), indexing="ij")
    offsets = np.stack([x, y + (q >> 1), z + (q & 1)], -1).reshape(-1, 3)
    background_seen = denormal_seen = 0
    for (name, g), f in zip(grids, files):
        org, (nx, ny, nz) = _table(g)
        cells = [(0, 0, 0), (nx - 1, ny - 1, nz - 1), (4, 4, 4), (1, 4, 4)]
        if g.tile_origin is not None:
            cells.append(tuple((np.array([64, 0, 0]) - org) >> 3))
        for a, b, c in cells:
            brick = DP.host_bricks(f, int((a * ny + b) * nz + c), 1, tmp_path).ravel()
            want, _, _ = HS.probe(g, org + 8 * np.array([a, b, c]) + offsets)
            assert brick.tobytes() == want.tobytes(), (name, (a, b, c), int((brick.view(np.uint32) != want.view(np.uint32)).sum()))
            background_seen += int(g.desc.background != 0.0 and (brick == np.float32(g.desc.background)).all())
            denormal_seen += int(((brick > 0) & (brick < GC.DENORMAL_MIN_NORMAL)).any())
    assert background_seen >= 8 and denormal_seen >= 6, (background_seen, denormal_seen)


# ---- the coverage pass's host march --------------------------------------------------------------------------
@pytest.mark.parametrize("case_id", GC.IDS)
def test_alpha_host_march_on_every_grid(case_id):
    """sub 1 on the case's frame: every pixel written, tau finite and >= +0, alpha = 1 - exp(-tau) within expf's
    error; the volume covers part of the frame.  (No float64 optical depth: see the module docstring.)"""
    wl, dens, _ = GC.BY_ID[case_id].build()
    alpha, tau = AL.render(wl.cfg, dens, 1, fill=np.nan)
    assert np.isfinite(tau).all() and (tau >= 0).all() and not np.signbit(tau).any()
    assert np.isfinite(alpha).all() and (alpha >= 0).all() and (alpha <= 1).all()
    assert np.abs(alpha + np.expm1(-tau.astype(np.float64))).max() <= 2.0 ** -22
    assert (tau > 0).any()
    if case_id == "inactive_half":  # the march reads values, not active bits
        assert tau.tobytes() == AL.render(wl.cfg, GC.reference("cloud").dens, 1)[1].tobytes()
    if case_id == "background=+0.05":  # the background is read between the leaves and the box
        assert tau.tobytes() != AL.render(wl.cfg, GC.reference("cloud").dens, 1)[1].tobytes()
