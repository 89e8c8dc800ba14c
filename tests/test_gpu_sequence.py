"""Sequences on one context (vpt_gpu_set_scene / vpt_gpu_set_grids, Integrator.set_scene / set_camera / set_volume,
render.render_sequence, the command line's --frames): a frame rendered after an update equals, byte for byte, the
frame of a context created fresh with that configuration and those grids.

The oracle's bytes come from tests/param_cases.py (P.reference / P.check_case): its 24x16 cases on the plain 64^3
cloud are 29 configurations that differ in one scene parameter each -- the sequence walked here -- and its nine
temperature-grid cases the second one.  Every frame is 24x16, 2 waves (4 for the gang kernel) on 64^3 grids (128^3
where tests/grids.py builds that); a launch takes milliseconds.
"""
import ctypes as C

import numpy as np
import pytest

import grids as G
import param_cases as P
from volume_path_tracer_amd import capi, image
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, orbit, read_configuration, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6


def _integrator(cfg, dens, temp=None):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(cfg, dens, temp, device=0)


def _film(it, jobs=None, first=0):
    """One production launch of `jobs` jobs (default: the configuration's) from zero -> (film, counters)."""
    film = torch.zeros_like(it.film)
    it.counters(reset=True)
    it.render_jobs(first, it.total_jobs if jobs is None else jobs, film=film)
    torch.cuda.synchronize()
    return film.cpu().numpy(), it.counters()


def _records(it, ref):
    rec = torch.full((ref.jobs * 64, 3), float("nan"), dtype=torch.float32, device=it.dev)
    film = torch.zeros_like(it.film)
    it.counters(reset=True)
    it.render_jobs(0, ref.jobs, film=film, records=rec)
    torch.cuda.synchronize()
    return film.cpu().numpy(), rec.cpu().numpy(), it.counters()


def _diff(a, b):
    """'n of N rows differ; first: ...' for two float32 arrays compared as bits, or None."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    if a.shape != b.shape:
        return f"shapes {a.shape} and {b.shape}"
    a, b = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
    bad = (a.view(np.uint32) != b.view(np.uint32)).any(axis=1)
    if not bad.any():
        return None
    i = int(np.flatnonzero(bad)[0])
    return f"{int(bad.sum())} of {bad.size} rows differ; first: row {i} got {a[i].tolist()} want {b[i].tolist()}"


def _check_stop(fails, what, it, ref, records=True):
    """The context, as it stands, against the oracle's outputs of `ref`: the ordered film and the production counters
    through the full (lat 0) and the latency (lat 1) scene copies, the records launch through the context copy."""
    for lat in (0, 1):
        it.set_latency_kernel(lat)
        f, c = _film(it, ref.jobs)
        d = _diff(f, ref.film)
        if d:
            fails.append(f"{what}: lat={lat}: film: {d}")
        for k in P.PRODUCTION_COUNTERS:
            if c[k] != ref.counters[k]:
                fails.append(f"{what}: lat={lat}: counter {k}: got {c[k]} want {ref.counters[k]}")
    it.set_latency_kernel(-1)
    if records:
        f, r, c = _records(it, ref)
        d = _diff(r, ref.rec)
        if d:
            fails.append(f"{what}: records: {d}")
        if not np.array_equal(f[..., 3], ref.film[..., 3]):
            fails.append(f"{what}: records launch: sample-count channel differs")
        for k in P.DEBUG_COUNTERS + (("temp_stencils",) if ref.temp is not None else ()):
            if c[k] != ref.counters[k]:
                fails.append(f"{what}: records launch: counter {k}: got {c[k]} want {ref.counters[k]}")


def _small(case_id):
    cfg = P.reference(case_id).cfg
    return (cfg.width, cfg.height) == (24, 16)


def _walk_ids(plain_c3):
    if plain_c3:
        return [c.id for c in P.CASES if c.plain_c3 and _small(c.id)]
    return [c.id for c in P.CASES if P.reference(c.id).temp is not None and _small(c.id)]


# max_depth = 1 and 2 both allow one scatter (max_scatters = ceil(max_depth / 2)): the table itself asserts that their
# records are the same bytes (param_cases._depth_1_2_3), so no output can tell an update between them from a no-op.
SAME_OUTPUT = {frozenset(("max_depth=1", "max_depth=2"))}


def _assert_every_step_shows(ids):
    """A condition on the inputs: consecutive stops' oracle films differ as bytes, or their counters do -- a set_scene
    that did nothing would then fail at the next stop.  (SAME_OUTPUT: the one pair the table declares identical.)"""
    for a, b in zip(ids, ids[1:]):
        ra, rb = P.reference(a), P.reference(b)
        if frozenset((a, b)) in SAME_OUTPUT:
            assert ra.rec.tobytes() == rb.rec.tobytes()
            continue
        assert ra.film.tobytes() != rb.film.tobytes() or ra.counters != rb.counters, (a, b)
        assert ra.rec.tobytes() != rb.rec.tobytes(), (a, b)


def _fused_uniform(it, waves):
    T = it.cfg.jobs_per_wave()
    film = torch.zeros_like(it.film)
    m2 = torch.zeros((it.cfg.height, it.cfg.width), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    p = capi.AdaptiveParams(0.0, 1e-3, 2, 2, waves)
    res = capi.AdaptiveResult()
    w, err = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    capi.check(capi.lib().vpt_gpu_render_adaptive_fused(
        it.h, C.byref(p), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
        w.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res),
        C.c_void_p(it.stream_handle())), "vpt_gpu_render_adaptive_fused")
    return film.cpu().numpy(), w


# ------------------------------------------------------------------------------------------------ 1. the c3 walk

def test_c3_walk_equals_the_oracle_at_every_stop():
    """One context, created on the first 24x16 plain-cloud case, moved by set_scene through all 29 in table order and
    back: at every stop both production kernels' films and counters and the records launch are the oracle's."""
    ids = _walk_ids(True)
    assert len(ids) == 29 and ids[0] == "g=0"
    for i in ids:
        P.check_case(i)
    _assert_every_step_shows(ids)
    first = P.reference(ids[0])
    it = _integrator(first.cfg, first.dens)
    fails = []
    _check_stop(fails, f"created on {ids[0]}", it, first)
    for n, i in enumerate(ids[1:] + ids[-2::-1]):
        ref = P.reference(i)
        it.set_scene(ref.cfg)
        assert bytes(it.cfg) == bytes(ref.cfg) and it.total_jobs == ref.jobs
        _check_stop(fails, f"stop {n + 1} ({i})", it, ref)
    assert not fails, "\n  ".join(fails[:20])


# ------------------------------------------------------------------------------------------------ 2. the c4 walk

def test_c4_walk_equals_the_oracle_at_every_stop():
    """The same over the nine temperature-grid cases; the walk passes lds-under -> lds-over -> lds-under, so the LDS
    copy of the blackbody table is allowed, refused and allowed again (bb_lds_ok).  The gang kernel's uniform 4-wave
    frame and the pixel-RNG kernel at the stops in P.EXTRA_KERNEL_IDS."""
    ids = _walk_ids(False)
    assert len(ids) == 9
    order = ids[1:] + ids[-2::-1]
    steps = list(zip(order, order[1:]))   # the rule flips both ways: off on the way out, on again on the way back
    assert steps.index(("lds-under", "lds-over")) < steps.index(("lds-over", "lds-under"))
    lo, hi = (P.temperature_range(P.reference(i))[1] for i in ("lds-under", "lds-over"))
    assert lo < P.LDS_RULE <= hi
    for i in ids:
        P.check_case(i)
    _assert_every_step_shows(ids)
    first = P.reference(ids[0])
    it = _integrator(first.cfg, first.dens, first.temp)
    fails = []
    extras = 0
    for n, i in enumerate([ids[0]] + order):
        ref = P.reference(i)
        if n:
            it.set_scene(ref.cfg)
        _check_stop(fails, f"stop {n} ({i})", it, ref)
        if i in P.EXTRA_KERNEL_IDS:
            extras += 1
            f, waves = _fused_uniform(it, 4)
            if not (waves == 4).all():
                fails.append(f"stop {n} ({i}): gang kernel: waves {np.unique(waves).tolist()}")
            d = _diff(f, ref.film4())
            if d:
                fails.append(f"stop {n} ({i}): gang kernel: film: {d}")
            it.set_rng_mode(capi.VPT_RNG_PIXEL)
            f_p, r_p = ref.pixel_mode()
            f, r, _ = _records(it, ref)
            d = _diff(r, r_p)
            if d:
                fails.append(f"stop {n} ({i}): pixel-RNG kernel: records: {d}")
            if not np.array_equal(f[..., 3], f_p[..., 3]):
                fails.append(f"stop {n} ({i}): pixel-RNG kernel: sample counts differ")
            it.set_rng_mode(capi.VPT_RNG_REFERENCE)
    assert extras >= 2
    assert not fails, "\n  ".join(fails[:20])


# ------------------------------------------------------------------------------------------------ 3. derived state

def _derived(it):
    """Everything a context derives from its scene besides the frame: the matte's planes, the tile costs and ranks, a
    band launch, a list launch with a moment plane and the tile errors of that."""
    out = {}
    out["alpha"], out["tau"] = it.render_alpha(tau=True)
    out["cost"], rank = it.tile_costs()
    out["rank"] = rank.astype(np.float32)
    T = it.jobs_per_wave
    band = torch.zeros_like(it.film)
    it.render_tiles(1, T - 1, 1, 2, film=band)
    torch.cuda.synchronize()
    out["band"] = band.cpu().numpy()
    lst = torch.zeros_like(it.film)
    m2 = torch.zeros((it.cfg.height, it.cfg.width), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    it.set_film_moments(m2)
    try:
        it.render_tile_list([0, 2, 3, T - 1], 1, 2, film=lst)
        torch.cuda.synchronize()
    finally:
        it.set_film_moments(None)
    out["list"], out["m2"] = lst.cpu().numpy(), m2.cpu().numpy()
    out["err"] = it.tile_errors(m2, film=lst)
    return out


def test_derived_state_follows_the_scene():
    """g=0 -> inside -> sigma=(50,50): the updated context's matte, tile costs and ranks, band launch, list launch
    with a moment plane and tile errors are a fresh context's of the same case, bytes for bytes -- with all of them
    computed before each update, so stale costs, ranks, band ranks or list ranks would show."""
    ids = ["g=0", "inside", "sigma=(50,50)"]
    refs = [P.reference(i) for i in ids]
    it = _integrator(refs[0].cfg, refs[0].dens)
    prev = _derived(it)
    for i, ref in zip(ids[1:], refs[1:]):
        it.set_scene(ref.cfg)
        got = _derived(it)
        want = _derived(_integrator(ref.cfg, ref.dens))
        for k in want:
            d = _diff(np.atleast_2d(got[k]), np.atleast_2d(want[k]))
            assert d is None, f"{i}: {k}: {d}"
        # the inputs: the scene change moves the costs and the matte (a stale copy would differ)
        assert got["cost"].tobytes() != prev["cost"].tobytes(), i
        assert got["tau"].tobytes() != prev["tau"].tobytes(), i
        prev = got


# ------------------------------------------------------------------------------------------------ 4. overrides

def _tune(it):
    it.set_tuning(gate_min=5, gate_idle=7, grid_blocks=96, gate_eval=30, gate_walk=3)
    it.set_full_tuning(gate_idle=3, gate_eval=20)
    it.set_latency_tuning(wave_lanes=2, gate_min=2, gate_idle=9)
    it.set_rng_mode(capi.VPT_RNG_PIXEL)
    it.set_pool_layout(capi.VPT_POOL_SPARSE)
    it.set_job_order(capi.VPT_ORDER_COST_TAIL)
    it.set_job_order_tail(1)
    it.set_film_order(capi.VPT_FILM_ATOMIC)


def _settings(it):
    pool = it.pool_info()
    pool.pop("expand_ms")
    return {"gates": [it.gate_info(s)[0] for s in (capi.VPT_GATES_CONTEXT, capi.VPT_GATES_LATENCY, capi.VPT_GATES_FULL)],
            "pool": pool, "film_order": it.film_order_info(), "launch": it.launch_info(),
            "latency": it.latency_kernel_info(), "variant": it.kernel_variant()}


def test_overrides_survive_a_scene_update():
    """Tuning, RNG mode, pool layout, job order and film order set before a set_scene are what they were after it, and
    the frame is a fresh context's with the same settings; the tile costs set by hand are gone (the scene's own are
    computed again) and so is the explicit job permutation (vpt_gpu_job_permutation_info), as documented."""
    a, b = P.reference("g=0"), P.reference("inside")
    it = _integrator(a.cfg, a.dens)
    _tune(it)
    T = it.jobs_per_wave
    it.set_tile_costs(np.arange(T, dtype=np.float32))
    it.set_job_permutation(np.arange(a.jobs, dtype=np.uint32)[::-1])
    assert it.tile_costs()[0].tolist() == list(range(T))
    assert it.job_permutation_size() == a.jobs
    _film(it)
    before = _settings(it)
    it.set_scene(b.cfg)
    assert _settings(it) == before
    assert it.job_permutation_size() == 0
    assert before["gates"] == [(5, 7, 30, 3), (2, 9, 1, 1), (5, 3, 20, 3)] and before["launch"][0] == 96
    assert before["pool"]["layout"] == capi.VPT_POOL_SPARSE and before["film_order"]["mode"] == capi.VPT_FILM_ATOMIC
    fresh = _integrator(b.cfg, b.dens)
    _tune(fresh)
    got, want = _film(it), _film(fresh)
    d = _diff(got[0], want[0])
    assert d is None, d
    assert got[1] == want[1]
    assert (want[0][..., 3] == P.WAVES).all() and want[0].tobytes() != b.film.tobytes()   # (the pixel mode's samples)
    cost, rank = it.tile_costs()
    cost_f, rank_f = fresh.tile_costs()
    assert cost.tobytes() == cost_f.tobytes() and rank.tolist() == rank_f.tolist()
    assert cost.tolist() != list(range(T))
    # and back in the reference mode the frame is the oracle's
    for x in (it, fresh):
        x.set_rng_mode(capi.VPT_RNG_REFERENCE)
        x.set_film_order(capi.VPT_FILM_ORDERED)
    d = _diff(_film(it)[0], b.film)
    assert d is None, d


# ------------------------------------------------------------------------------------------------ 5. refusals

def test_refused_updates_leave_the_scene():
    """Another output_size or tile_size is VPT_E_INVALID naming the field; an open feed is VPT_E_STATE; null grids and a
    temperature grid for a density-only context are VPT_E_INVALID.  After each the context renders its case's oracle
    film exactly."""
    L = capi.lib()
    ref, other = P.reference("g=-0.4"), P.reference("inside")
    it = _integrator(ref.cfg, ref.dens)
    it.set_tuning(grid_blocks=1)   # 256 lanes: a feed launches once 256 jobs are pushed
    fails = []

    def still(what):
        assert bytes(it.cfg) == bytes(ref.cfg)
        _check_stop(fails, what, it, ref, records=False)

    for field, msg in (("output_size", b"output_size"), ("tile_size", b"tile_size")):
        for axis in (0, 1):
            c = other.cfg.copy()
            getattr(c, field)[axis] += 1
            assert L.vpt_gpu_set_scene(it.h, C.byref(c)) == VPT_E_INVALID
            assert msg in L.vpt_last_error()
            with pytest.raises(RuntimeError, match=field):
                it.set_scene(c)
        still(f"after a refused {field}")
    c = other.cfg.copy()
    c.tile_size[0] = 0   # (an invalid configuration whose sizes also differ)
    assert L.vpt_gpu_set_scene(it.h, C.byref(c)) == VPT_E_INVALID
    # an open feed
    feed_film = torch.zeros_like(it.film)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(256, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    c = other.cfg.copy()
    rc_scene = L.vpt_gpu_set_scene(it.h, C.byref(c))
    msg_scene = L.vpt_last_error()
    g = C.c_void_p()
    capi.check(L.vpt_grids_flatten(C.byref(ref.dens.desc), None, C.byref(g)), "flatten")
    rc_grids = L.vpt_gpu_set_grids(it.h, g)
    msg_grids = L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    assert rc_scene == VPT_E_STATE and b"feed" in msg_scene
    assert rc_grids == VPT_E_STATE and b"feed" in msg_grids
    still("after an open feed refused the updates")
    # the volume: null grids, and a presence mismatch
    assert L.vpt_gpu_set_grids(it.h, None) == VPT_E_INVALID
    L.vpt_grids_free(g)
    dens, temp = G.temperature_pair("same")
    with pytest.raises(RuntimeError, match="temperature"):
        it.set_volume(dens, temp)
    still("after a refused volume")
    assert not fails, "\n  ".join(fails)
    # and the updates work afterwards
    it.set_scene(other.cfg)
    d = _diff(_film(it)[0], other.film)
    assert d is None, d


# ------------------------------------------------------------------------------------------------ 6. num_waves

def test_num_waves_follows():
    import oracle_lib as O

    ref = P.reference("g=0.95")
    it = _integrator(ref.cfg, ref.dens)
    T = it.jobs_per_wave
    assert it.total_jobs == 2 * T
    c = ref.cfg.copy()
    c.num_waves = 5
    it.set_scene(c)
    jpw, tot = C.c_uint64(), C.c_uint64()
    capi.check(capi.lib().vpt_gpu_job_space(it.h, C.byref(jpw), C.byref(tot)), "job_space")
    assert (jpw.value, tot.value) == (T, 5 * T) and (it.jobs_per_wave, it.total_jobs) == (T, 5 * T)
    film = torch.zeros_like(it.film)
    it.render_waves(5, 1, film=film)
    torch.cuda.synchronize()
    want = O.render_jobs(c, ref.od, None, 4 * T, T)[0]
    d = _diff(film.cpu().numpy(), want)
    assert d is None, d
    # the whole frame of the new job space
    d = _diff(_film(it)[0], O.render_jobs(c, ref.od, None, 0, 5 * T)[0])
    assert d is None, d


# ------------------------------------------------------------------------------------------------ 7. volume swap

def _c3_cfg():
    return P.reference("g=0").cfg.copy()


def _density_stops():
    """(name, cfg, density, table case or None) of the density-only walk."""
    sparse_cfg = _c3_cfg()
    G.look_at(sparse_cfg, (-40.0, -90.0, -700.0), (-40.0, -90.0, 10.0))
    sparse_cfg.camera_parameters.vfov_deg = 50.0
    tiles_cfg = _c3_cfg()
    G.look_at(tiles_cfg, (-500.0, 30.0, -300.0), (500.0, 30.0, 60.0))
    cloud = P.reference("g=0").dens
    cloud128 = SynthGrid(1, 128).grid()   # (the 64^3 cloud's runs are long enough for run skipping; the 128^3 one's are not)
    small, large = P.reference("voxel=2^-20"), P.reference("voxel=2^26")
    return [("cloud", _c3_cfg(), cloud, "g=0"),
            ("signed", _c3_cfg(), G.signed_grid(), None),
            ("voxel=2^-20", small.cfg.copy(), small.dens, "voxel=2^-20"),
            ("voxel=2^26", large.cfg.copy(), large.dens, "voxel=2^26"),
            ("sparse", sparse_cfg, G.sparse_grid(), None),
            ("tiles-only", tiles_cfg, G.tiles_only_grid(), None),
            ("cloud 128", _c3_cfg(), cloud128, None),
            ("cube", _c3_cfg(), SynthGrid(0, 128).grid(), None),
            ("cloud 128 again", _c3_cfg(), cloud128, None),
            ("cloud again", _c3_cfg(), cloud, "g=0")]


def _volume_state(it):
    pool = it.pool_info()
    return {"variant": it.kernel_variant(), "layout": pool["layout"], "policy": pool["policy"],
            "sparse_bytes": pool["sparse_bytes"], "dense_bytes": pool["dense_bytes"], "launch": it.launch_info(),
            "latency": it.latency_kernel_info()}


@pytest.mark.parametrize("forced", ["auto", "sparse-pool", "no-run-skipping"])
def test_volume_swap_density(forced):
    """One density-only context through the cloud, the signed grid, two extreme voxel sizes, the sparse grid of every
    HDDA level, a grid of tiles alone, the 128^3 cloud, the constant cube, the 128^3 cloud and the first cloud again --
    each stop one set_volume and one
    set_scene: the film, the counters, the kernel variant, the pool's layout and byte counts and the grid are a fresh
    context's (with the same setter applied), and the oracle's film where the table has the case.  Auto run skipping
    is off for the 128^3 cloud, turns on for the cube and off again for the 128^3 cloud (the 64^3 cloud itself takes
    the run-skipping variant, as a fresh context on it does); a forced 0 stays; a forced sparse pool stays."""
    def force(x):
        if forced == "sparse-pool":
            x.set_pool_layout(capi.VPT_POOL_SPARSE)
        elif forced == "no-run-skipping":
            x.set_run_skipping(0)

    stops = _density_stops()
    it = _integrator(stops[0][1], stops[0][2])
    force(it)
    fails, runs, prev = [], {}, None
    for n, (name, cfg, dens, case) in enumerate(stops):
        if n:
            it.set_volume(dens)
            it.set_scene(cfg)
        fresh = _integrator(cfg, dens)
        force(fresh)
        got, want = _film(it), _film(fresh)
        d = _diff(got[0], want[0])
        if d:
            fails.append(f"{name}: film vs a fresh context: {d}")
        if got[1] != want[1]:
            fails.append(f"{name}: counters {got[1]} vs a fresh context's {want[1]}")
        if _volume_state(it) != _volume_state(fresh):
            fails.append(f"{name}: {_volume_state(it)} vs a fresh context's {_volume_state(fresh)}")
        if case is not None:
            d = _diff(got[0], P.reference(case).film)
            if d:
                fails.append(f"{name}: film vs the oracle: {d}")
        assert want[1]["samples"] == 24 * 16 * 2
        if prev is not None:
            assert want[0].tobytes() != prev, f"{name}: the stop's frame is the previous stop's (a no-op would pass)"
        prev = want[0].tobytes()
        runs[name] = it.kernel_variant()["run_skipping"]
        if forced == "sparse-pool":
            assert it.pool_info()["layout"] == capi.VPT_POOL_SPARSE and it.pool_info()["dense_bytes"] == (0, 0)
    if forced == "no-run-skipping":
        assert not any(runs.values()), runs
    else:
        assert not runs["cloud 128"] and runs["cube"] and not runs["cloud 128 again"], runs
    assert not fails, "\n  ".join(fails)


@pytest.mark.parametrize("forced", ["auto", "sparse-pool", "no-run-skipping"])
def test_volume_swap_temperature(forced):
    """One temperature context through temperature_pair("same") -> ("shifted") -> ("half_voxels"), the configuration
    alternating between two of the table's temperature cases (either side of the LDS-rows rule for these grids' value
    range); a density-only volume is refused and the previous frame still reproduced.  Repeated with the sparse pool
    forced (the layout of two grids is applied again at every swap) and with run skipping forced off."""
    def force(x):
        if forced == "sparse-pool":
            x.set_pool_layout(capi.VPT_POOL_SPARSE)
        elif forced == "no-run-skipping":
            x.set_run_skipping(0)

    cfgs = [P.reference(i).cfg.copy() for i in ("lds-under", "lds-over", "knots")]
    it = None
    prev = None
    for kind, cfg in zip(("same", "shifted", "half_voxels"), cfgs):
        dens, temp = G.temperature_pair(kind)
        if it is None:
            it = _integrator(cfg, dens, temp)
            force(it)
        else:
            it.set_volume(dens, temp)
            it.set_scene(cfg)
        fresh = _integrator(cfg, dens, temp)
        force(fresh)
        if forced == "sparse-pool":
            assert it.pool_info()["layout"] == capi.VPT_POOL_SPARSE and it.pool_info()["dense_bytes"] == (0, 0)
        else:
            assert it.pool_info()["layout"] == capi.VPT_POOL_DENSE and all(it.pool_info()["dense_bytes"])
        got, want = _film(it), _film(fresh)
        d = _diff(got[0], want[0])
        assert d is None, f"{kind}: {d}"
        assert got[1] == want[1] and want[1]["temp_stencils"] > 0, kind
        assert _volume_state(it) == _volume_state(fresh), kind
        assert want[0].tobytes() != prev
        prev = want[0].tobytes()
        if kind == "same":
            d = _diff(got[0], P.reference("lds-under").film)
            assert d is None, f"same: vs the oracle: {d}"
    with pytest.raises(RuntimeError, match="temperature"):
        it.set_volume(G.temperature_pair("same")[0], None)
    assert _film(it)[0].tobytes() == prev


# ------------------------------------------------------------------------------------------------ 7b. a failed swap

VPT_E_NOMEM = 5


@pytest.mark.parametrize("nth", [1, 2])
def test_failed_volume_swap_leaves_no_volume(nth):
    """A vpt_gpu_set_grids that fails after the old volume was freed (vpt_gpu_debug_fail_upload: the density's upload
    of a density-only context; the temperature's, after the density's succeeded, of a two-grid context) returns
    VPT_E_NOMEM saying that the context has no volume; every call that launches, computes or takes tile costs, or
    derives a scene then returns VPT_E_STATE and writes nothing; settings and queries still work; a later good swap
    and set_scene render the oracle's film; and a context without a volume can be destroyed."""
    L = capi.lib()
    ref = P.reference("g=0" if nth == 1 else "lds-under")
    other = P.reference("inside" if nth == 1 else "knots")
    it = _integrator(ref.cfg, ref.dens, ref.temp)
    T = it.jobs_per_wave
    it.set_tile_costs(np.arange(T, dtype=np.float32))   # (valid ranks, which must not outlive the volume)
    assert _diff(_film(it)[0], ref.film) is None

    def swap(x, dens, temp):
        g = C.c_void_p()
        capi.check(L.vpt_grids_flatten(C.byref(dens.desc), C.byref(temp.desc) if temp is not None else None, C.byref(g)),
                   "flatten")
        try:
            return L.vpt_gpu_set_grids(x.h, g), L.vpt_last_error()
        finally:
            L.vpt_grids_free(g)

    capi.check(L.vpt_gpu_debug_fail_upload(it.h, nth), "debug_fail_upload")
    rc, msg = swap(it, other.dens, other.temp)
    assert rc == VPT_E_NOMEM and b"(the context has no volume now)" in msg and b"vpt_gpu_set_grids" in msg
    film = torch.zeros_like(it.film)
    plane = torch.full((16, 24), float("nan"), dtype=torch.float32, device=it.dev)
    rec = torch.full((ref.jobs * 64, 3), float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    s = C.c_void_p(it.stream_handle())
    fp, up = C.POINTER(C.c_float), C.POINTER(C.c_uint32)
    cost, rank = np.zeros(T, np.float32), np.zeros(T, np.uint32)
    o, d = np.zeros(3, np.float32), np.array([0, 0, 1], np.float32)
    rows, n = np.zeros((8, 9), np.float32), C.c_int()
    c = other.cfg.copy()
    calls = {
        "render_jobs": lambda: L.vpt_gpu_render_jobs(it.h, 0, ref.jobs, C.c_void_p(film.data_ptr()), s),
        "render_jobs_records": lambda: L.vpt_gpu_render_jobs_records(it.h, 0, ref.jobs, C.c_void_p(film.data_ptr()),
                                                                     C.c_void_p(rec.data_ptr()), s),
        "render_tiles": lambda: L.vpt_gpu_render_tiles(it.h, 0, T, 0, 2, C.c_void_p(film.data_ptr()), s),
        "render_alpha": lambda: L.vpt_gpu_render_alpha(it.h, 1, C.c_void_p(plane.data_ptr()), None, s),
        "tile_costs": lambda: L.vpt_gpu_tile_costs(it.h, cost.ctypes.data_as(fp), rank.ctypes.data_as(up)),
        "set_tile_costs": lambda: L.vpt_gpu_set_tile_costs(it.h, cost.ctypes.data_as(fp)),
        "majorant_trace": lambda: L.vpt_gpu_majorant_trace(it.h, o.ctypes.data_as(fp), d.ctypes.data_as(fp),
                                                           rows.ctypes.data_as(fp), 8, C.byref(n)),
        "set_scene": lambda: L.vpt_gpu_set_scene(it.h, C.byref(c)),
    }
    for rounds in range(2):   # (the second round: after set_tile_costs was refused, nothing made the ranks valid)
        for name, call in calls.items():
            assert call() == VPT_E_STATE, name
            assert b"no volume" in L.vpt_last_error(), name
    with pytest.raises(RuntimeError, match="no volume"):
        _fused_uniform(it, 4)
    torch.cuda.synchronize()
    assert not film.any() and torch.isnan(plane).all() and torch.isnan(rec).all()   # nothing was written
    assert bytes(it.cfg) == bytes(ref.cfg)
    # settings and queries still work
    pool = it.pool_info()
    assert pool["sparse_bytes"] == (0, 0) and pool["dense_bytes"] == (0, 0) and pool["layout"] == capi.VPT_POOL_SPARSE
    assert it.kernel_variant()["has_temperature"] == (ref.temp is not None)
    it.set_tuning(gate_walk=2)
    it.set_tuning(gate_walk=1 if ref.temp is not None else 4)
    it.counters(reset=True)
    assert it.job_permutation_size() == 0 and it.launch_info()[1] == 256
    # a swap that still fails (the presence rule is checked first and leaves the state as it is)
    capi.check(L.vpt_gpu_debug_fail_upload(it.h, 1), "debug_fail_upload")
    rc, msg = swap(it, other.dens, other.temp)
    assert rc == VPT_E_NOMEM and calls["render_jobs"]() == VPT_E_STATE
    # the recovery: a good swap, then the scene
    it.set_volume(other.dens, other.temp)
    it.set_scene(other.cfg)
    fails = []
    _check_stop(fails, "after the recovery", it, other)
    fresh = _integrator(other.cfg, other.dens, other.temp)
    assert _volume_state(it) == _volume_state(fresh)
    assert it.tile_costs()[0].tobytes() == fresh.tile_costs()[0].tobytes()
    assert not fails, "\n  ".join(fails)
    # a context without a volume is destroyed like any other
    capi.check(L.vpt_gpu_debug_fail_upload(fresh.h, 1), "debug_fail_upload")
    assert swap(fresh, ref.dens, ref.temp)[0] == VPT_E_NOMEM
    h, fresh.h = fresh.h, None
    assert L.vpt_gpu_destroy(h) == capi.VPT_OK
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 8. render_sequence

def test_render_sequence_with_a_png_sink(tmp_path):
    from volume_path_tracer_amd.render import render_sequence, render_uniform

    base = _c3_cfg()
    cfgs = orbit(base, 4)
    dens = P.reference("g=0").dens
    it = _integrator(cfgs[0], dens)
    seen, films = [], {}

    def sink(k, film):
        assert isinstance(film, np.ndarray)   # a host copy
        seen.append(k)
        films[k] = film
        image.save_png(tmp_path / f"o_{k}.png", image.film_to_image(film))

    stats = render_sequence(it, [(None, None)] + [(c, None) for c in cfgs[1:]],
                            lambda i: render_uniform(i, moments=False), sink)
    assert seen == [0, 1, 2, 3] and stats["frames"] == 4 and len(stats["update_ms"]) == 4
    for k, c in enumerate(cfgs):
        want = _film(_integrator(c, dens))[0]
        d = _diff(films[k], want)
        assert d is None, f"frame {k}: {d}"
        png = image.decode_png((tmp_path / f"o_{k}.png").read_bytes())
        assert (png == image.film_to_image(want)).all()
    assert len({f.tobytes() for f in films.values()}) == 4
    # a sink that fails ends the sequence with its exception
    def bad(k, film):
        raise OSError("disk full")

    with pytest.raises(OSError, match="disk full"):
        render_sequence(it, [(c, None) for c in cfgs], lambda i: render_uniform(i, moments=False), bad)


# ------------------------------------------------------------------------------------------------ 9. command line

def _cli_cfg():
    cfg = read_configuration(SCENE_DIR / "wdas_cloud.json")
    cfg.num_waves = 2
    cfg.output_size[0], cfg.output_size[1] = 24, 16
    return cfg


def test_cli_orbit_sequence(tmp_path, capsys):
    from volume_path_tracer_amd.__main__ import main

    scene = str(SCENE_DIR / "wdas_cloud.json")
    base = ["--synthetic", "cloud:64", "--size", "24x16", "--spp", "2"]
    seq = ["--frames", "3", "--orbit", "90"]
    assert main([scene, str(tmp_path / "out_%02d.png")] + base + seq + ["--film-out", str(tmp_path / "f_%02d.npy")]) == 0
    err = capsys.readouterr().err
    assert all(f"frame {k}: Rendering complete" in err for k in range(3)) and "Sequence complete: 3 frames" in err
    dens = SynthGrid(1, 64).grid()
    films = []
    for k, c in enumerate(orbit(_cli_cfg(), 3, 90.0)):
        film = np.load(tmp_path / f"f_{k:02d}.npy")
        d = _diff(film, _film(_integrator(c, dens))[0])
        assert d is None, f"frame {k}: {d}"
        png = image.decode_png((tmp_path / f"out_{k:02d}.png").read_bytes())
        assert (png == image.film_to_image(film)).all()
        films.append(film.tobytes())
    assert len(set(films)) == 3
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([f"out_{k:02d}.png" for k in range(3)] +
                                                                [f"f_{k:02d}.npy" for k in range(3)])
    # --denoise --alpha: RGBA files; frame 0's RGB is the single-frame program's with the same flags
    assert main([scene, str(tmp_path / "dn_%d.png")] + base + seq + ["--denoise", "--alpha"]) == 0
    assert main([scene, str(tmp_path / "single.png")] + base + ["--denoise", "--alpha"]) == 0
    single = image.decode_png((tmp_path / "single.png").read_bytes())
    for k in range(3):
        rgba = image.decode_png((tmp_path / f"dn_{k}.png").read_bytes())
        assert rgba.shape == (16, 24, 4)
    rgba0 = image.decode_png((tmp_path / "dn_0.png").read_bytes())
    assert (rgba0 == single).all()


def test_cli_camera_path_and_volume_sequence(tmp_path, capsys):
    import json

    from volume_path_tracer_amd import volumes
    from volume_path_tracer_amd.__main__ import main

    scene = str(SCENE_DIR / "wdas_cloud.json")
    base = ["--size", "24x16", "--spp", "2"]
    vols = [SynthGrid(1, 64).grid(), G.signed_grid()]
    for k, g in enumerate(vols):
        volumes.save_npz(tmp_path / f"v_{k}.npz", g)
    # two single-frame runs: the scene file's volume_path is relative to it, so each gets its own scene file
    doc = json.loads((SCENE_DIR / "wdas_cloud.json").read_text())
    singles = []
    for k in range(2):
        doc["volume_path"] = f"v_{k}.npz"
        (tmp_path / f"scene_{k}.json").write_text(json.dumps(doc))
        assert main([str(tmp_path / f"scene_{k}.json"), str(tmp_path / f"s_{k}.png")] + base +
                    ["--film-out", str(tmp_path / f"s_{k}.npy")]) == 0
        singles.append(np.load(tmp_path / f"s_{k}.npy"))
    assert main([scene, str(tmp_path / "q_%d.png")] + base + ["--frames", "2", "--volume-sequence",
                                                              str(tmp_path / "v_%d.npz"), "--film-out",
                                                              str(tmp_path / "q_%d.npy")]) == 0
    for k in range(2):
        d = _diff(np.load(tmp_path / f"q_{k}.npy"), singles[k])
        assert d is None, f"frame {k}: {d}"
        assert (tmp_path / f"q_{k}.png").read_bytes() == (tmp_path / f"s_{k}.png").read_bytes()
    assert singles[0].tobytes() != singles[1].tobytes()
    # a camera path
    cfg = _cli_cfg()
    cams = [{"position": list(cfg.camera_parameters.position), "look": list(cfg.camera_parameters.look)},
            {"position": [0.0, 20.0, -120.0], "look": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov_deg": 40.0}]
    (tmp_path / "cams.json").write_text(json.dumps(cams))
    assert main([scene, str(tmp_path / "c_%d.png")] + base + ["--synthetic", "cloud:64", "--camera-path",
                                                              str(tmp_path / "cams.json"), "--film-out",
                                                              str(tmp_path / "c_%d.npy")]) == 0
    from volume_path_tracer_amd.scenes import with_camera

    for k, cam in enumerate(cams):
        want = _film(_integrator(with_camera(cfg, **cam), vols[0]))[0]
        d = _diff(np.load(tmp_path / f"c_{k}.npy"), want)
        assert d is None, f"camera {k}: {d}"
