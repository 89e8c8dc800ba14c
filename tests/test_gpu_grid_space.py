"""Every HIP kernel against the oracle across the grid space (tests/grid_cases.py).

tests/test_gpu_param_space.py moves the scene's parameters over the plain cloud; here the grid moves: backgrounds,
index boxes that cut leaves or reach into empty root space and onto root tiles, leaves across lower / upper / root
node boundaries, index coordinates up to 2^22, inactive voxels with values, denormal values and majorants, the
hand-built grids of every HDDA level, non-identity maps, temperature grids of another map or topology.  What runs
only on a device on these inputs -- the 24-bit multiply-add indexing with large table origins, the hardware rcp /
log / rsq sequences on denormal majorants, the dense pool's expansion kernel over a background, the LDS tables, the
gates -- has no CPU twin: tests/test_grid_space_host.py holds the host build of the shared code to the oracle on the
same table and checks the conditions that make each case mean something.

Per case, one context (plus the coverage pass's own, and one at 96x72 for the compacting kernel, as set_scene does
not resize a frame):
  a. the records kernel: records, sample counts, debug counters;
  b. the throughput and the latency production kernel: the ordered 2-wave film and the production counters;
  c. density-only cases: the run-skipping instantiation, forced;
  d. the throughput film under each stencil pool layout, forced (sparse, dense);
  e. the coverage pass: tau byte-equal to the host march, alpha within EXPF_TOL;
and for GC.EXTRA_IDS:
  f. the gang kernel of the fused adaptive driver: the uniform 4-wave frame;
  g. the pixel-RNG kernel: records and sample counts;
  h. the band kernel: two uneven bands into one film;
  i. the compacting latency kernel at 96x72 (T = 108): each wave's film, the counters, `exchanged` > 0;
  j. the feed kernel: the case's 2 T jobs in two uneven pushes through a staged feed, closed and collected.  A feed
     adds with film atomics in completion order; with two samples per pixel that film is still the oracle's bit for
     bit (0 + a + b == 0 + b + a in fp32), so this comparison is on bits too: no tolerance, and none of the drop-in's
     ordered-frame machinery.
Every film and record comparison is on bit patterns (uint32 views); the one tolerance of the module is the coverage
pass's EXPF_TOL on the alpha plane, inside test_gpu_alpha.check_parity.
"""
import numpy as np
import pytest

import grid_cases as GC
import oracle_lib as O
from test_gpu_alpha import check_parity
from test_gpu_param_space import _check_production, _check_records, _first_diff, _fused_uniform, _records
from volume_path_tracer_amd import capi

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

LAYOUTS = (("sparse", capi.VPT_POOL_SPARSE), ("dense", capi.VPT_POOL_DENSE))


def _integrator(ref):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(ref.cfg, ref.dens, ref.temp, device=0)


def _check_film(fails, what, got, want):
    d = _first_diff(got, want)
    if d:
        fails.append(f"{what}: film: {d}")


def _pool_layouts(fails, notes, it, ref):
    """d. The throughput film under each layout the context accepts; a refused layout goes into `notes`."""
    it.set_latency_kernel(0)
    for name, layout in LAYOUTS:
        try:
            it.set_pool_layout(layout)
        except RuntimeError as e:
            notes.append(f"pool layout {name}: skipped, the context refused it ({e})")
            continue
        got = it.pool_info()["layout"]
        if got != layout:
            fails.append(f"pool layout {name}: pool_info reports layout {got}")
            continue
        _check_production(fails, f"throughput kernel, {name} pool", it, ref)
    it.set_pool_layout(capi.VPT_POOL_AUTO)


def _bands(fails, it, ref):
    """h. Tiles [0, 2) and [2, T) as two band launches into one film."""
    film = torch.zeros_like(it.film)
    it.render_tiles(0, 2, 1, GC.WAVES, film=film)
    it.render_tiles(2, ref.T, 1, GC.WAVES, film=film)
    torch.cuda.synchronize()
    _check_film(fails, "band kernel", film.cpu().numpy(), ref.film)


def _compaction(fails, case_id):
    """i. The compacting latency kernel on the case's scene at 96x72, a wave per launch."""
    from volume_path_tracer_amd.render import Integrator

    big = GC.reference_compact(case_id)
    assert big.T == 108
    it = Integrator(big.cfg, big.dens, big.temp, device=0)
    it.set_latency_kernel(1, 0)
    it.set_tuning(grid_blocks=4)
    it.set_compaction(4)
    it.counters(reset=True)
    for w in range(GC.WAVES):
        film = torch.zeros_like(it.film)
        it.render_jobs(w * big.T, big.T, film=film)
        torch.cuda.synchronize()
        _check_film(fails, f"compacting latency kernel, wave {w + 1}", film.cpu().numpy(), big.wave_films[w])
    c = it.counters()
    for k in GC.PRODUCTION_COUNTERS:
        if c[k] != big.counters[k]:
            fails.append(f"compacting latency kernel: counter {k}: got {c[k]} want {big.counters[k]}")
    if not c["exchanged"] > 0:
        fails.append("compacting latency kernel: no path was exchanged")


def _feed(fails, it, ref):
    """j. The case's jobs through a staged feed: 5 jids, then the rest, close, collect."""
    from volume_path_tracer_amd.render import Feed

    dev_film = torch.zeros_like(it.film)
    torch.cuda.synchronize()
    feed = Feed(it, dev_film, torch.cuda.Stream(device=it.dev), 1024, staged=True)
    host = np.zeros((ref.cfg.height, ref.cfg.width, 4), np.float32)
    try:
        jids = np.arange(ref.jobs, dtype=np.uint64)
        feed.push(jids[:5])
        feed.push(jids[5:])
        feed.close()
        feed.collect(host)
    finally:
        feed.destroy()
    _check_film(fails, "feed kernel", host, ref.film)


@pytest.mark.parametrize("case_id", GC.IDS)
def test_every_kernel_equals_the_oracle(case_id):
    """Steps a-e for every case and f-j for GC.EXTRA_IDS (the module docstring lists them).  Every mismatch of the
    case is collected and reported with its first differing row, after a preamble of what was skipped."""
    ref = GC.check_case(case_id)
    it = _integrator(ref)
    fails, notes = [], []
    _check_records(fails, "records kernel", _records(it, ref), ref, ref.rec, ref.film, ref.counters)
    for lat in (0, 1):
        it.set_latency_kernel(lat)
        _check_production(fails, f"production kernel lat={lat}", it, ref)
    if ref.temp is None:
        it.set_latency_kernel(0)
        it.set_run_skipping(1)
        assert it.kernel_variant()["run_skipping"] is True
        _check_production(fails, "production kernel with run skipping", it, ref)
        it.set_run_skipping(-1)
    _pool_layouts(fails, notes, it, ref)
    try:
        check_parity(ref.cfg, ref.dens, ref.temp, 2)
    except AssertionError as e:
        fails.append(f"coverage pass: {e}")
    if case_id in GC.EXTRA_IDS:
        it.set_latency_kernel(-1)
        f_g, waves = _fused_uniform(it, 4)
        if not (waves == 4).all():
            fails.append(f"gang kernel: waves {np.unique(waves).tolist()}")
        _check_film(fails, "gang kernel", f_g, ref.film4())
        it.set_rng_mode(capi.VPT_RNG_PIXEL)
        f_p, r_p = ref.pixel_mode()
        _check_records(fails, "pixel-RNG kernel", _records(it, ref), ref, r_p, f_p)
        it.set_rng_mode(capi.VPT_RNG_REFERENCE)
        _bands(fails, it, ref)
        _feed(fails, it, ref)
        _compaction(fails, case_id)
    for n in notes:
        print(f"{case_id}: {n}")
    assert not fails, f"{case_id}:\n  " + "\n  ".join(notes + fails)


# ---- the majorant trace ------------------------------------------------------------------------------------------
TRACE_IDS = [i for i in GC.DENSITY_IDS if i != "sparse"]   # tests/test_traces.py traces the sparse grid
DIRECTIONS = [(0.05, -0.02, 1.0), (-1.0, 0.3, 0.2), (0.4, 0.8, -0.45), (-0.6, -0.7, -0.4)]
INSIDE = [(0.03, 0.05, 0.04), (0.96, 0.1, 0.9), (0.5, 0.93, 0.07), (0.35, 0.45, 0.6)]   # fractions of the index box


def _trace_rays(grid):
    """8 world rays: 4 through the centre of the grid's index box from 3 box diagonals outside it, 4 that start
    inside the box (near its faces and corners: in empty root space where the box is loose)."""
    d = grid.desc
    m, vec = np.asarray(d.map_mat[:], np.float64).reshape(3, 3), np.asarray(d.map_vec[:], np.float64)
    lo, hi = np.asarray(d.index_bbox_min[:], np.float64), np.asarray(d.index_bbox_max[:], np.float64) + 1.0
    centre = m @ ((lo + hi) / 2) + vec
    diagonal = np.linalg.norm(m @ (hi - lo))
    rays = []
    for k, direction in enumerate(DIRECTIONS):
        u = np.asarray(direction, np.float32)
        u = (u / np.float32(np.linalg.norm(u))).astype(np.float32)
        rays.append(((centre - 3.0 * diagonal * u.astype(np.float64)).astype(np.float32), u))
        start = m @ (lo + np.asarray(INSIDE[k]) * (hi - lo)) + vec
        rays.append((start.astype(np.float32), u))
    return rays


@pytest.mark.parametrize("case_id", TRACE_IDS)
def test_majorant_trace_on_the_new_grids(case_id):
    """vpt_majorant_trace_kernel's rows against the oracle's restatement of Volume::log_majorant_trace, byte for
    byte as tests/test_traces.py compares them, where rays start in empty root space, cross the 4096 boundaries, run
    2^22 voxels from the origin or through denormal majorants."""
    ref = GC.reference(case_id)
    it = _integrator(ref)
    rows = 0
    for o, d in _trace_rays(ref.dens):
        g, r = it.majorant_trace(o, d), O.majorant_trace(ref.od, o, d)
        assert g.shape == r.shape and g.tobytes() == r.tobytes(), (case_id, o.tolist(), d.tolist(), g.shape, r.shape)
        rows += len(r)
    assert rows > 8, rows
