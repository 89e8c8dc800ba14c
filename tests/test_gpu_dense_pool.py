"""The direct-addressed stencil pool on the GPU (vpt_gpu_set_pool_layout): every kernel gives the oracle's bytes with
the dense pool on and off, on frames small enough to run in a second -- 24x16, 2 waves, 64^3 grids for the density
(c3) and the density + temperature (c4) kernels, and the sparse anchor grid of tests/grids.py at 24x24, the smallest
frames on which every tree level and both grids are reached.  The layout never changes a value a lane reads, so
everything here is compared as bytes.  Then the policy: VPT_POOL_AUTO's fallback under a cap, the refusal while a feed
is open, the info call's byte counts, and the device pool itself against the host expansion
(tests/native/dense_pool_host.cpp)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

import alpha_lib as AL
import dense_pool_lib as DP
import grids as G
import oracle_lib as O
import param_cases as P
from test_gpu_param_space import _check_production, _check_records, _first_diff, _fused_uniform, _records
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SPARSE, DENSE, AUTO = capi.VPT_POOL_SPARSE, capi.VPT_POOL_DENSE, capi.VPT_POOL_AUTO
BRICK_BYTES = 9216
VPT_E_STATE = 6


def _anchor():
    wl = workload("c3", width=24, height=24, spp=P.WAVES)
    G.look_at(wl.cfg, (-40.0, -90.0, -700.0), (-40.0, -90.0, 10.0))
    wl.cfg.camera_parameters.vfov_deg = 50.0
    return wl, G.sparse_grid(), None


def _shifted():
    wl = workload("c4", width=24, height=16, spp=P.WAVES, grid_n=64)
    dens, temp = G.temperature_pair("shifted")
    return wl, dens, temp


SCENES = {"c3": P._c3, "c4": P._c4, "anchor": _anchor}
_REF = {}


def scene(name):
    if name not in _REF:
        _REF[name] = P.Reference(SCENES[name])
        P.check_common(_REF[name])
    return _REF[name]


def _integrator(ref):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(ref.cfg, ref.dens, ref.temp, device=0)


def table_cells(grid) -> int:
    """Cells of the cells8 table: 16^3 per lower node of the bounding box of the grid's lower nodes (leaves' and
    lower-node tiles' parents)."""
    org = [grid.leaf_origin]
    if grid.tile_origin is not None:
        org.append(grid.tile_origin[np.asarray(grid.tile_level) == 1])
    lower = np.concatenate(org) >> 7
    return int(np.prod((lower.max(0) - lower.min(0) + 1) * 16))


def tile_mask(cfg, tiles):
    """bool [H][W]: the pixels of the listed tiles."""
    W, H = cfg.width, cfg.height
    tw, th = int(cfg.tile_size[0]), int(cfg.tile_size[1])
    ntx = -(-W // tw)
    m = np.zeros((H, W), bool)
    for t in tiles:
        x0, y0 = (t % ntx) * tw, (t // ntx) * th
        m[y0:y0 + th, x0:x0 + tw] = True
    return m


def every_kernel(fails, what, it, ref, gang=True):
    """The records kernel, the throughput and latency production kernels (the run-skipping variant too without a
    temperature grid), a tile-list launch, the gang kernel and the alpha pass's tau plane against the oracle.
    Returns the bytes of everything rendered, for the comparison between the layouts."""
    out = []
    got = _records(it, ref)
    _check_records(fails, f"{what}: records kernel", got, ref, ref.rec, ref.film, ref.counters)
    out += [got[0].tobytes(), got[1].tobytes()]
    for lat in (0, 1):
        it.set_latency_kernel(lat)
        _check_production(fails, f"{what}: production kernel lat={lat}", it, ref)
    it.set_latency_kernel(-1)
    if ref.temp is None:
        it.set_run_skipping(1)
        _check_production(fails, f"{what}: run-skipping kernel", it, ref)
        it.set_run_skipping(-1)
    # a tile-list launch of every other tile, both waves: those tiles' pixels of the oracle's film, nothing else
    tiles = list(range(0, ref.T, 2))
    film = torch.zeros_like(it.film)
    it.counters(reset=True)
    it.render_tile_list(tiles, 1, P.WAVES, film=film)
    torch.cuda.synchronize()
    f = film.cpu().numpy()
    want = np.where(tile_mask(ref.cfg, tiles)[..., None], ref.film, np.float32(0.0))
    d = _first_diff(f, want)
    if d:
        fails.append(f"{what}: tile-list launch: {d}")
    out.append(f.tobytes())
    if gang:
        f_g, waves = _fused_uniform(it, 4)
        d = _first_diff(f_g, ref.film4())
        if d or not (waves == 4).all():
            fails.append(f"{what}: gang kernel: {d} waves {np.unique(waves).tolist()}")
        out.append(f_g.tobytes())
    _, tau = it.render_alpha(sub=2, tau=True)
    if not hasattr(ref, "host_tau"):
        ref.host_tau = AL.render(ref.cfg, ref.dens, 2)[1]
    h_tau = ref.host_tau
    if tau.tobytes() != h_tau.tobytes():
        fails.append(f"{what}: alpha pass: tau differs from the host march in {int((tau != h_tau).sum())} pixels")
    out.append(tau.tobytes())
    return out


@pytest.mark.parametrize("name", list(SCENES))
def test_parity_dense_on_and_off(name):
    """Throughput, latency, run-skipping and gang kernels, a tile-list launch, the records kernel (records, debug
    counters) and the alpha pass's tau plane: the oracle's bytes with the dense pool and without, on one context."""
    ref = scene(name)
    it = _integrator(ref)
    fails, outs = [], {}
    if not os.environ.get("VPT_POOL_LAYOUT"):  # AUTO's choice on these grids
        info = it.pool_info()
        assert info["layout"] == DENSE and info["policy"] == AUTO, info
    for layout in (DENSE, SPARSE, DENSE):
        it.set_pool_layout(layout)
        assert it.pool_info()["layout"] == layout
        got = every_kernel(fails, f"layout {layout}", it, ref)
        outs.setdefault(layout, got)
        if got != outs[layout]:
            fails.append(f"layout {layout}: a second pass over the kernels rendered other bytes")
    if outs[DENSE] != outs[SPARSE]:
        fails.append("dense and sparse rendered different bytes")
    if name == "anchor":  # the grid holds every tree level: leaves, lower / upper / root tiles and empty space
        dims = {O.OracleGrid(ref.dens).get_dim(*p) for p in ((3, 3, 3), (64, 0, 0), (128, 0, 0), (4096, 0, 0), (-300, 0, 0))}
        assert {8, 128, 4096} <= dims, dims
    assert not fails, f"{name}:\n  " + "\n  ".join(fails)


PARAM_IDS = ["inside", "away", "voxel=2^26", "top-rows", "sigma=(50,50)"]


@pytest.mark.parametrize("case_id", PARAM_IDS + ["shifted-temperature"])
def test_param_cases_with_the_dense_pool(case_id):
    """A handful of tests/param_cases.py cases with the dense pool on: a camera inside the volume and one looking
    away, voxel size 2^26, the blackbody table's top rows, a dense medium; and a temperature grid shifted against the
    density's, whose lookups fall in other cells and partly outside its table."""
    if case_id == "shifted-temperature":
        ref = _REF.setdefault(case_id, P.Reference(_shifted))
        P.check_common(ref)
        assert ref.counters["temp_stencils"] > 100
    else:
        ref = P.check_case(case_id)
    it = _integrator(ref)
    it.set_pool_layout(DENSE)
    info = it.pool_info()
    assert info["layout"] == DENSE and info["dense_bytes"][0] == table_cells(ref.dens) * BRICK_BYTES
    fails = []
    _check_records(fails, "records kernel", _records(it, ref), ref, ref.rec, ref.film, ref.counters)
    for lat in (0, 1):
        it.set_latency_kernel(lat)
        _check_production(fails, f"production kernel lat={lat}", it, ref)
    assert not fails, f"{case_id}:\n  " + "\n  ".join(fails)


def test_auto_falls_back_under_a_cap_and_says_so():
    """VPT_POOL_AUTO with a cap one byte below the dense size stays sparse without an error and reports it; at the
    size it goes dense; the cap is the sum over both grids."""
    ref = scene("c4")
    it = _integrator(ref)
    need = (table_cells(ref.dens) + table_cells(ref.temp)) * BRICK_BYTES
    it.set_pool_layout(AUTO, cap_bytes=need - 1)
    info = it.pool_info()
    assert info["layout"] == SPARSE and info["policy"] == AUTO and info["dense_bytes"] == (0, 0)
    fails = []
    _check_production(fails, "sparse after the fallback", it, ref)
    it.set_pool_layout(AUTO, cap_bytes=need)
    info = it.pool_info()
    assert info["layout"] == DENSE and sum(info["dense_bytes"]) == need and info["expand_ms"] > 0.0
    _check_production(fails, "dense at the cap", it, ref)
    it.set_pool_layout(AUTO, cap_bytes=0)  # the default cap: 1/8 of the device's memory
    assert it.pool_info()["layout"] == DENSE
    assert not fails, "\n  ".join(fails)


def test_info_bytes():
    """Both pools' bytes: table cells x 9216 per grid dense, leaves x 9216 sparse; the sparse pool stays resident."""
    for name in ("c4", "anchor"):
        ref = scene(name)
        it = _integrator(ref)
        grids = [ref.dens] + ([ref.temp] if ref.temp is not None else [])
        want_dense = tuple(table_cells(g) * BRICK_BYTES for g in grids) + (0,) * (2 - len(grids))
        want_sparse = tuple(g.leaf_count * BRICK_BYTES for g in grids) + (0,) * (2 - len(grids))
        it.set_pool_layout(DENSE)
        info = it.pool_info()
        assert info["dense_bytes"] == want_dense and info["sparse_bytes"] == want_sparse, info
        it.set_pool_layout(SPARSE)
        info = it.pool_info()
        assert info["dense_bytes"] == (0, 0) and info["sparse_bytes"] == want_sparse and info["policy"] == SPARSE
    assert table_cells(scene("anchor").dens) == 80 * 80 * 48


def test_setter_refuses_while_a_feed_is_open():
    """While a feed of the context is launched and not closed the setter returns VPT_E_STATE at once and changes
    nothing; after the close it works, and the feed's film is the oracle's."""
    wl = workload("c3", width=64, height=48, spp=16, grid_n=64)
    from volume_path_tracer_amd.render import Integrator

    it = Integrator(wl.cfg, SynthGrid(1, 64).grid(), None, device=0)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    film = torch.zeros_like(it.film)
    torch.cuda.synchronize()
    before = it.pool_info()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(16 * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    t0 = time.monotonic()
    for layout in (SPARSE, DENSE, AUTO):
        assert L.vpt_gpu_set_pool_layout(it.h, layout) == VPT_E_STATE and b"feed" in L.vpt_last_error()
    assert time.monotonic() - t0 < 5.0
    assert it.pool_info() == before
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    np.testing.assert_array_equal(film.cpu().numpy()[..., 3], 16)
    it.set_pool_layout(SPARSE)
    assert it.pool_info()["layout"] == SPARSE
    assert L.vpt_gpu_set_pool_layout(it.h, 3) == 1 and L.vpt_gpu_set_pool_layout(None, DENSE) == 1  # VPT_E_INVALID


def test_device_pool_equals_the_host_expansion(tmp_path):
    """vpt_gpu_debug_read_pool on the anchor grid: the table's first and last cells (aprons past the table), runs
    across a lower node with leaves and its lower-node tiles, and one in the gap with the upper-node tile -- the host
    expansion's bytes.  A few bricks also against the oracle's getValue, voxel by voxel."""
    ref = scene("anchor")
    it = _integrator(ref)
    it.set_pool_layout(DENSE)
    cells = table_cells(ref.dens)
    grid_file = DP.write_grid(tmp_path / "anchor.grid", ref.dens)
    nz, ny = 48, 80
    org = np.array([-256, -384, 0])

    def cell_of(i, j, k):
        a, b, c = (np.array([i, j, k]) - org) >> 3
        return int((a * ny + b) * nz + c)

    runs = [(0, 96), (cells - 96, 96), (cell_of(64, 64, 0), 48), (cell_of(64, 56, 0), 48), (cell_of(64, 0, 0) - 8, 32),
            (cell_of(0, 72, 64) - 4, 16), (cell_of(128, 0, 0), 32), (cell_of(120, 120, 0), 48)]
    leaf_cells = 0
    for begin, count in runs:
        dev = it.debug_read_pool(0, begin, count)
        host = DP.host_bricks(grid_file, begin, count, tmp_path)
        assert dev.tobytes() == host.tobytes(), (begin, count, int((dev.view(np.uint32) != host.view(np.uint32)).sum()))
        leaf_cells += int((np.abs(dev).max(axis=1) > 0.3).sum())
    assert leaf_cells > 10
    og = O.OracleGrid(ref.dens)
    for cell in (cell_of(64, 64, 64), cell_of(64, 8, 0), cells - 1):  # a leaf, a lower tile, the table's last cell
        brick = it.debug_read_pool(0, cell, 1).reshape(8, 8, 9, 4)
        a, rem = divmod(cell, ny * nz)
        b, c = divmod(rem, nz)
        o = org + 8 * np.array([a, b, c])
        for y, z, x in ((0, 0, 0), (7, 7, 8), (3, 7, 5), (7, 2, 8)):
            for q in range(4):
                want = np.float32(og.get_value(int(o[0] + x), int(o[1] + y + (q >> 1)), int(o[2] + z + (q & 1))))
                assert brick[y, z, x, q].view(np.uint32) == want.view(np.uint32), (cell, x, y, z, q)
    with pytest.raises(Exception):
        it.debug_read_pool(0, cells, 1)
    it.set_pool_layout(SPARSE)
    assert capi.lib().vpt_gpu_debug_read_pool(it.h, 0, 0, 1, np.zeros(2304, np.float32).ctypes.data_as(
        C.POINTER(C.c_float))) == VPT_E_STATE
