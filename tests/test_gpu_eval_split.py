"""The split density evaluation on the GPU: the density-only production kernels of the throughput family (plain,
run-skipping, band, gang) issue a collision's stencil loads at the top of lane_iteration (eval_issue) and finish the
evaluation in front of the ray block (eval_finish), with the finish, fetch and pixel blocks in between and NEE
completion behind it.  The split only moves work inside
an iteration: a lane's own order of operations and draws is the one it was, so every film here equals the oracle's
(tests/oracle_lib.py render_jobs) BIT FOR BIT and the counters `samples`, `stencils` and `dda_steps` are the oracle's.

Full launches at small sizes are forced with set_tuning(grid_blocks=1), as in tests/test_gpu_full_tuning.py (a grid
set by the caller is never moved to the latency kernel).  kernel_variant(last_launch=True) tells whether the launch
just made ran a split instantiation.

The axes: the full-launch gates (1, 1, 1, 1) -- eval_issue with a single lane --, the defaults, and (64, 1, 64, 1) --
eval_issue with every lane, and no rare block between the halves; the pool layout, dense (every lane carries loads),
sparse (every lane takes eval_finish's lookup path) and the anchor grid's dense pool, whose table does not hold every
voxel a ray samples (lanes of both kinds in one wavefront; the library's pool is dense or sparse for both grids of a
scene, so a cap cannot leave one of two grids sparse: this mixed wavefront is the case such a cap would make); the
job order; and the other kernels: the run-skipping one on a small cube, a band and a gang launch of the base case, and
the temperature kernel, which evaluates whole."""
import ctypes as C
import functools

import numpy as np
import pytest

import grids as G
import oracle_lib as O
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

COUNTERS = ("samples", "stencils", "dda_steps")
BASE = ("c3", 96, 64, 64, 67)     # T = 96 tiles, 6 432 jobs on one block (4 wavefronts): a full launch
RAGGED = ("c3", 37, 29, 128, 66)  # ragged tiles on both edges, the 128^3 cloud
CUBE = ("c2", 48, 40, 64, 12)     # the constant cube: the run-skipping kernel
FIRE = ("c4", 40, 32, 64, 70)     # the temperature kernel
GATES = [(1, 1, 1, 1), None, (64, 1, 64, 1)]  # (gate_min, gate_idle, gate_eval, gate_walk); None: the library's


class Ref:
    """A scene, its grids and the oracle's film and counters of `waves` whole waves: computed once, never written."""

    def __init__(self, wl, dens, temp, waves):
        self.wl, self.cfg, self.dens, self.temp, self.waves = wl, wl.cfg, dens, temp, waves
        self.T = wl.cfg.jobs_per_wave()
        od = O.OracleGrid(dens, fix_majorants=True)
        ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
        self.film, _, self.counters = O.render_jobs(wl.cfg, od, ot, 0, waves * self.T)
        self.film.setflags(write=False)


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, n, waves):
    wl = workload(name, width=w, height=h, spp=waves, grid_n=n)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    return Ref(wl, dens, temp, waves)


@functools.lru_cache(maxsize=None)
def _anchor_ref():
    """tests/grids.py's sparse anchor grid (leaves, lower / upper / root tiles, empty space between its lower nodes)
    at 24x24, 12 waves: 108 jobs per wave."""
    wl = workload("c3", width=24, height=24, spp=12)
    G.look_at(wl.cfg, (-40.0, -90.0, -700.0), (-40.0, -90.0, 10.0))
    wl.cfg.camera_parameters.vfov_deg = 50.0
    return Ref(wl, G.sparse_grid(), None, 12)


def _integrator(ref):
    from volume_path_tracer_amd.render import Integrator

    it = Integrator(ref.cfg, ref.dens, ref.temp, device=0)
    it.set_tuning(grid_blocks=1)
    return it


def _check(it, ref, film, what, split=True):
    torch.cuda.synchronize()
    f_g = film.cpu().numpy()
    kv = it.kernel_variant(last_launch=True)
    assert kv["eval_split"] is split, f"{what}: {kv}"
    c = it.counters()
    for k in COUNTERS:
        assert c[k] == ref.counters[k], f"{what}: counter {k}: {c[k]}, the oracle's {ref.counters[k]}"
    np.testing.assert_array_equal(f_g[..., 3], float(ref.waves))
    diff = (f_g.view(np.uint32) != ref.film.view(np.uint32)).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ"


def _render_and_check(it, ref, what, split=True):
    it.counters(reset=True)
    film = torch.zeros_like(it.film)
    it.render_jobs(0, ref.waves * ref.T, film=film)
    _check(it, ref, film, what, split)


def test_variant_before_the_first_launch():
    it = _integrator(_ref(*BASE))
    assert set(it.kernel_variant()) == {"has_temperature", "run_skipping"}  # (as before without the argument)
    assert it.kernel_variant(last_launch=True)["eval_split"] is None


@pytest.mark.parametrize("gates", GATES, ids=["gates-1", "gates-default", "gates-64"])
@pytest.mark.parametrize("case", [BASE, RAGGED], ids=["base", "ragged"])
def test_full_launch_gates(case, gates):
    ref = _ref(*case)
    it = _integrator(ref)
    it.set_run_skipping(0)  # the plain kernel (small grids choose the run-skipping one: test_run_skipping_kernel)
    if gates is not None:
        it.set_full_tuning(*gates)
        assert it.gate_info(capi.VPT_GATES_FULL)[0] == gates
    assert it.pool_info()["layout"] == capi.VPT_POOL_DENSE
    _render_and_check(it, ref, f"gates {gates}")
    assert it.gate_info(capi.VPT_GATES_FULL)[1] == capi.VPT_GATES_FULL


@pytest.mark.parametrize("gates", GATES, ids=["gates-1", "gates-default", "gates-64"])
def test_sparse_pool_takes_the_lookup_path(gates):
    """Without the direct-addressed pool no lane carries loads: every evaluation finishes on the lookup path."""
    ref = _ref(*BASE)
    it = _integrator(ref)
    it.set_pool_layout(capi.VPT_POOL_SPARSE)
    assert it.pool_info()["layout"] == capi.VPT_POOL_SPARSE
    if gates is not None:
        it.set_full_tuning(*gates)
    _render_and_check(it, ref, f"sparse pool, gates {gates}")


@pytest.mark.parametrize("layout", [capi.VPT_POOL_DENSE, capi.VPT_POOL_SPARSE], ids=["dense", "sparse"])
def test_dense_table_that_misses_voxels(layout):
    """The anchor grid: rays sample tiles and background outside the dense pool's table, so a wavefront holds lanes
    with loads in flight and lanes without; and the same frame sparse."""
    ref = _anchor_ref()
    assert ref.counters["stencils"] > 1000
    it = _integrator(ref)
    it.set_pool_layout(layout)
    assert it.pool_info()["layout"] == layout
    for gates in ((1, 1, 1, 1), None):
        if gates is not None:
            it.set_full_tuning(*gates)
        else:
            it.set_full_tuning(6, 4, 36, 4)
        _render_and_check(it, ref, f"anchor grid, layout {layout}, gates {gates}")


def test_job_orders():
    ref = _ref(*BASE)
    it = _integrator(ref)
    for mode in (capi.VPT_ORDER_COST_SAME_TILE, capi.VPT_ORDER_COST_TAIL, capi.VPT_ORDER_JID):
        it.set_job_order(mode)
        _render_and_check(it, ref, f"order {mode}")


def test_run_skipping_kernel():
    ref = _ref(*CUBE)
    it = _integrator(ref)
    it.set_run_skipping(1)
    assert it.kernel_variant()["run_skipping"]
    for gates in GATES:
        if gates is not None:
            it.set_full_tuning(*gates)
        _render_and_check(it, ref, f"cube, gates {gates}")


def test_band_launch():
    ref = _ref(*BASE)
    it = _integrator(ref)
    it.counters(reset=True)
    film = torch.zeros_like(it.film)
    it.render_tiles(0, ref.T, 1, ref.waves, film=film)
    _check(it, ref, film, "band launch")


def test_gang_launch():
    """The fused adaptive driver with target 0: every tile runs to max_waves, the uniform frame."""
    ref = _ref(*BASE)
    it = _integrator(ref)
    it.counters(reset=True)
    film = torch.zeros_like(it.film)
    m2 = torch.zeros((ref.cfg.height, ref.cfg.width), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    p = capi.AdaptiveParams(0.0, 1e-3, 3, 16, ref.waves)
    res = capi.AdaptiveResult()
    w, err = np.zeros(ref.T, np.uint32), np.zeros(ref.T, np.float32)
    capi.check(capi.lib().vpt_gpu_render_adaptive_fused(
        it.h, C.byref(p), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
        w.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res),
        C.c_void_p(it.stream_handle())), "vpt_gpu_render_adaptive_fused")
    assert (w == ref.waves).all()
    _check(it, ref, film, "gang launch")


def test_temperature_kernel_evaluates_whole():
    """The temperature kernel keeps the evaluation in one piece (80 VGPRs at 6 waves leave the stencil no registers
    across the rare blocks): the launch says so, and renders the oracle's film as before."""
    ref = _ref(*FIRE)
    it = _integrator(ref)
    _render_and_check(it, ref, "temperature kernel", split=False)
    assert ref.counters["temp_stencils"] > 0 and it.counters()["temp_stencils"] == ref.counters["temp_stencils"]
