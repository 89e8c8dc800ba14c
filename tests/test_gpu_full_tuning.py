"""The full-launch gate set (vpt_gpu_set_full_tuning): production launches of the throughput kernel read gates of
their own; partly filled launches, latency launches, feeds and debug launches keep the context's.

Gates only choose when a block of the lane state machine runs, never what a lane computes: every film here equals
the oracle's (tests/oracle_lib.py render_jobs) BIT FOR BIT.  The film cannot show a job that ran twice -- its count
channel comes from the film pass, and a job's samples are plain stores to the job's own slots -- so every case also
checks the kernel's sample counter against jobs x pixels per tile.

Full launches at small sizes are forced with set_tuning(grid_blocks=1), as in tests/test_gpu_film_order.py.
"""
import functools

import numpy as np
import pytest

import oracle_lib as O
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VPT_E_INVALID = 1  # include/vpt_gpu.h


@functools.lru_cache(maxsize=None)
def _ref(name, w, h, n, spp):
    """The workload, its grids and the oracle's film of `spp` whole waves: computed once, shared, never written."""
    wl = workload(name, width=w, height=h, spp=spp, grid_n=n)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
    f_o, _, _ = O.render_jobs(wl.cfg, od, ot, 0, spp * wl.cfg.jobs_per_wave())
    f_o.setflags(write=False)
    return wl, dens, temp, f_o


def _integrator(ref):
    from volume_path_tracer_amd.render import Integrator

    wl, dens, temp, _ = ref
    return Integrator(wl.cfg, dens, temp, device=0)


def _samples_expected(cfg, spp):
    """jobs x pixels per tile, tile by tile (8x8 tiles clipped at the right and bottom edges)."""
    tw = th = 8
    total = 0
    for y0 in range(0, cfg.height, th):
        for x0 in range(0, cfg.width, tw):
            total += spp * min(tw, cfg.width - x0) * min(th, cfg.height - y0)
    return total


def _render_and_check(it, ref, spp, what, gate_set=None):
    wl, _, _, f_o = ref
    it.counters(reset=True)
    film = torch.zeros_like(it.film)
    it.render_jobs(0, spp * wl.cfg.jobs_per_wave(), film=film)
    torch.cuda.synchronize()
    f_g = film.cpu().numpy()
    if gate_set is not None:
        assert it.gate_info(gate_set)[1] == gate_set, f"{what}: the launch read gate set {it.gate_info(gate_set)[1]}"
    samples = it.counters()["samples"]
    assert samples == _samples_expected(wl.cfg, spp), f"{what}: {samples} samples traced"
    np.testing.assert_array_equal(f_g[..., 3], float(spp))
    diff = (f_g.view(np.uint32) != f_o.view(np.uint32)).any(axis=-1)
    assert not diff.any(), f"{what}: {int(diff.sum())} of {diff.size} pixels differ"


FULL = [
    # (workload, width, height, grid_n, waves): one block (4 wavefronts) makes each a full launch
    ("c3", 96, 64, 64, 67),    # T = 96 tiles, 6 432 jobs
    ("c4", 40, 32, 64, 70),    # temperature kernel
    ("c3", 37, 29, 128, 66),   # ragged tiles on both edges
]


def test_tile_size_assumed():
    """(_samples_expected restates the reference's 8x8 tiles)"""
    assert _ref(*FULL[0])[0].cfg.jobs_per_wave() == 96
    assert _samples_expected(_ref(*FULL[2])[0].cfg, 66) == 66 * 37 * 29


@pytest.mark.parametrize("gate_idle", [None, 2, 1])
@pytest.mark.parametrize("name,w,h,n,waves", FULL)
def test_full_launch_with_its_own_gates(name, w, h, n, waves, gate_idle):
    """A full launch on the library's full-launch gates (None) and on gate_idle 2 / 1 set for full launches alone
    (the context's set stays as created) equals the oracle."""
    ref = _ref(name, w, h, n, waves)
    it = _integrator(ref)
    it.set_tuning(grid_blocks=1)
    if gate_idle is not None:
        it.set_full_tuning(gate_idle=gate_idle)
    _render_and_check(it, ref, waves, f"{name} full gate_idle {gate_idle}", capi.VPT_GATES_FULL)
    assert it.gate_info(capi.VPT_GATES_FULL)[0][1] == (gate_idle or (1 if name == "c4" else 4))
    assert it.gate_info(capi.VPT_GATES_CONTEXT)[0][1] == (1 if name == "c4" else 8)


def test_job_orders_on_the_full_launch_gates():
    """The three job orders on a full launch that reads gate_idle 2 from the full-launch set: the same film."""
    ref = _ref(*FULL[0])
    it = _integrator(ref)
    it.set_tuning(grid_blocks=1)
    it.set_full_tuning(gate_min=4, gate_idle=2, gate_eval=24, gate_walk=2)
    for mode in (capi.VPT_ORDER_COST_SAME_TILE, capi.VPT_ORDER_COST_TAIL, capi.VPT_ORDER_JID):
        it.set_job_order(mode)
        _render_and_check(it, ref, 67, f"order {mode}")


def test_set_tuning_then_full_tuning():
    """set_tuning writes both sets, set_full_tuning then overrides the full-launch one: still the oracle's film."""
    ref = _ref(*FULL[0])
    it = _integrator(ref)
    assert it.gate_info(capi.VPT_GATES_CONTEXT) == ((6, 8, 36, 4), -1)  # the density kernel's defaults
    assert it.gate_info(capi.VPT_GATES_FULL)[0] == (6, 4, 36, 4)
    lat = it.gate_info(capi.VPT_GATES_LATENCY)[0]
    it.set_tuning(gate_min=3, gate_idle=16, grid_blocks=1, gate_eval=20, gate_walk=1)
    assert it.gate_info(capi.VPT_GATES_CONTEXT)[0] == it.gate_info(capi.VPT_GATES_FULL)[0] == (3, 16, 20, 1)
    _render_and_check(it, ref, 67, "set_tuning", capi.VPT_GATES_FULL)
    it.set_full_tuning(gate_idle=2)  # the other values keep
    assert it.gate_info(capi.VPT_GATES_FULL)[0] == (3, 2, 20, 1)
    assert it.gate_info(capi.VPT_GATES_CONTEXT)[0] == (3, 16, 20, 1) and it.gate_info(capi.VPT_GATES_LATENCY)[0] == lat
    _render_and_check(it, ref, 67, "set_tuning + set_full_tuning", capi.VPT_GATES_FULL)
    it.set_tuning(gate_walk=0)  # (only gate_walk: 0 is a value for it)
    assert it.gate_info(capi.VPT_GATES_FULL)[0] == (3, 2, 20, 0) and it.gate_info(capi.VPT_GATES_CONTEXT)[0] == (3, 16, 20, 0)


def test_bad_arguments():
    ref = _ref("c3", 48, 40, 64, 6)
    it = _integrator(ref)
    L = capi.lib()
    assert L.vpt_gpu_set_full_tuning(it.h, 0, 0, 0, -1) == VPT_E_INVALID  # gate_idle 0 could stall a wavefront
    assert L.vpt_gpu_set_full_tuning(None, 0, 2, 0, -1) == VPT_E_INVALID
    assert L.vpt_gpu_set_full_tuning(it.h, 0, 2, 0, -1) == capi.VPT_OK
    with pytest.raises(RuntimeError):
        it.set_full_tuning(gate_idle=0)
    assert L.vpt_gpu_gate_info(it.h, 3, None, None) == VPT_E_INVALID
    assert it.gate_info(capi.VPT_GATES_FULL)[0][1] == 2


# test_gpu_film_order.py's test_multi_wave_film_bit_identical shapes: (workload, width, height, grid_n, run_skipping, waves)
SMALL = [
    ("c3", 48, 40, 64, 0, 6),
    ("c3", 37, 29, 128, 0, 5),
    ("c2", 64, 48, 128, 1, 5),
    ("c4", 40, 32, 64, -1, 5),
]


@pytest.mark.parametrize("name,w,h,n,runs,waves", SMALL)
def test_full_tuning_leaves_other_launches_alone(name, w, h, n, runs, waves):
    """After set_full_tuning(gate_idle=2), launches on the latency kernel (latency-bound and partly filled ones:
    the `lat` 1 cases of test_multi_wave_film_bit_identical) render the oracle's film as before."""
    ref = _ref(name, w, h, n, waves)
    it = _integrator(ref)
    it.set_full_tuning(gate_idle=2)
    it.set_latency_kernel(1)
    if runs >= 0:
        it.set_run_skipping(runs)
    _render_and_check(it, ref, waves, f"{name} lat 1", capi.VPT_GATES_LATENCY)  # (latency-bound: few jobs per wavefront)
    # 4 blocks = 16 wavefronts, more than 6 jobs per wavefront: partly filled, on the latency kernel with the context's gates
    assert waves * ref[0].cfg.jobs_per_wave() > 6 * 16
    it.set_tuning(grid_blocks=4)
    _render_and_check(it, ref, waves, f"{name} lat 1, partly filled", capi.VPT_GATES_CONTEXT)


def test_debug_launch_reads_the_context_gates():
    """A launch with per-sample records (the debug kernel) on a full grid keeps the context's gates; its records
    hold every sample."""
    ref = _ref("c3", 48, 40, 64, 6)
    wl = ref[0]
    it = _integrator(ref)
    it.set_tuning(grid_blocks=1)
    jobs = 6 * wl.cfg.jobs_per_wave()
    rec = torch.full((jobs * 64, 3), float("nan"), device="cuda:0")
    it.counters(reset=True)
    it.render_jobs(0, jobs, records=rec)
    torch.cuda.synchronize()
    assert it.gate_info(capi.VPT_GATES_CONTEXT)[1] == capi.VPT_GATES_CONTEXT
    assert it.counters()["samples"] == _samples_expected(wl.cfg, 6)
    assert not torch.isnan(rec).any()
