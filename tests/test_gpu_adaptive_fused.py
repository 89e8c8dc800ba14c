"""The adaptive driver in one launch (include/vpt_gpu.h, vpt_gpu_render_adaptive_fused): a wavefront owns a tile,
renders its waves in groups of up to 64, adds them into the film and the plane itself and evaluates the tile's error
at the round boundaries.

Every output must equal, BIT FOR BIT, both the driver's rule emulated on the oracle's per-wave states
(tests/adaptive_ref.py emulate_adaptive) and the rounds driver (vpt_gpu_render_adaptive) on the same integrator.
The frames, helpers and the cached oracle references are those of tests/test_gpu_adaptive.py.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as A
from test_gpu_adaptive import (ADAPTIVE, MAX_W, MIN_W, SENTINEL, STEP_W, VPT_E_INVALID, VPT_E_STATE, _assert_bitwise,
                               _integrator, _new_plane, _reference, _wl)
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SCENE_DIR

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

FLOOR = 1e-3
GRID_N = 64


def _hist(waves):
    v, c = np.unique(waves, return_counts=True)
    return {int(a): int(b) for a, b in zip(v, c)}


def _emulated(name, w, h, tile, sp, target, mn, step, mx):
    wl = _wl(name, w, h, GRID_N, mx, tile, sp)
    _, films, m2s = _reference(name, w, h, GRID_N, 0, mx, tile, sp, 0.0)
    return wl, A.emulate_adaptive(wl.cfg, films, m2s, target, FLOOR, mn, step, mx)


def _run(it, target, mn, step, mx, fused):
    """render_adaptive with the plane returned too -> (film, plane, waves, err, info)."""
    T = it.cfg.jobs_per_wave()
    film, m2 = torch.zeros_like(it.film), _new_plane(it, 0.0)
    torch.cuda.synchronize()
    p = capi.AdaptiveParams(float(target), FLOOR, mn, step, mx)
    res = capi.AdaptiveResult()
    waves, err = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    L = capi.lib()
    fn = L.vpt_gpu_render_adaptive_fused if fused else L.vpt_gpu_render_adaptive
    capi.check(fn(it.h, C.byref(p), C.c_void_p(film.data_ptr()), C.c_void_p(m2.data_ptr()),
                  waves.ctypes.data_as(C.POINTER(C.c_uint32)), err.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res),
                  C.c_void_p(it.stream_handle())), "fused" if fused else "rounds")
    return film.cpu().numpy(), m2.cpu().numpy(), waves, err, res.as_dict()


def _assert_same(got, want, what):
    (f, m, w, e, i), (wf, wm, ww, we, wi) = got, want
    np.testing.assert_array_equal(w, ww, err_msg=f"{what}: waves")
    _assert_bitwise(f, wf, f"{what}: film")
    _assert_bitwise(m, wm, f"{what}: plane")
    _assert_bitwise(e, we, f"{what}: err")
    if wi is not None:
        assert i == wi, f"{what}: info"


# ------------------------------------------------------------------- 1. the emulated rule and the rounds driver

CASES = {
    # id: (workload, width, height, tile, target, min / step / max, the oracle's waves: tiles)
    "A-c3": ("c3", 48, 40, None, 0.1, (70, 70, 200), {70: 16, 140: 11, 200: 3}),
    "A-c4-temperature": ("c4", 40, 32, None, 0.02, (70, 70, 200), {70: 9, 140: 3, 200: 8}),
    "A-c3-ragged-12x8": ("c3", 37, 29, (12, 8), 0.08, (70, 70, 200), {70: 10, 140: 2, 200: 4}),
    "A-c3-ragged-4x4": ("c3", 37, 29, (4, 4), 0.1, (70, 70, 200), {70: 50, 140: 24, 200: 6}),
    "A-c3-16x16": ("c3", 48, 40, (16, 16), 0.08, (70, 70, 200), {70: 3, 140: 4, 200: 2}),
    "A-c2-runs": ("c2", 48, 40, None, 0.1, (70, 70, 200), {70: 11, 140: 4, 200: 15}),
    "B-c3": ("c3",) + ADAPTIVE["c3"][:2] + (None, ADAPTIVE["c3"][2], (MIN_W, STEP_W, MAX_W), {8: 16, 16: 1, 24: 6, 32: 7}),
    "B-c4-temperature": ("c4",) + ADAPTIVE["c4"][:2] + (None, ADAPTIVE["c4"][2], (MIN_W, STEP_W, MAX_W),
                                                         {8: 12, 16: 2, 32: 6}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_fused_equals_the_emulated_rule_and_the_rounds_driver(case):
    name, w, h, tile, target, (mn, step, mx), hist = CASES[case]
    wl, (e_film, e_m2, e_waves, e_err) = _emulated(name, w, h, tile, None, target, mn, step, mx)
    T = wl.cfg.jobs_per_wave()
    # the spread that makes the case meaningful, on the reference alone: tiles at the minimum, in between, at the cap
    assert _hist(e_waves) == hist
    assert (e_waves == mn).any() and ((e_waves > mn) & (e_waves < mx)).any() and (e_waves == mx).any()
    it = _integrator(wl)
    if name == "c2":
        it.set_run_skipping(1)
        assert it.kernel_variant() == {"has_temperature": False, "run_skipping": True}
    if name == "c4":
        assert it.kernel_variant()["has_temperature"]
    fused = _run(it, target, mn, step, mx, fused=True)
    _assert_same(fused, (e_film, e_m2, e_waves, e_err, None), f"{case}: fused vs the emulated rule")
    info = fused[4]
    assert info["jobs_rendered"] == int(e_waves.sum()) and info["jobs_uniform"] == mx * T
    assert info["tiles_at_max"] == int((e_waves == mx).sum())
    assert info["rounds"] == 1 + -(-(int(e_waves.max()) - mn) // step)
    assert np.float32(info["max_error"]) == e_err.max()
    rounds = _run(it, target, mn, step, mx, fused=False)
    _assert_same(fused, rounds, f"{case}: fused vs the rounds driver")


# ------------------------------------------------------------------------------------------------ 2. grid sizes

def test_one_block_and_the_default_grid_give_the_same_bytes():
    """grid_blocks = 1: four wavefronts claim all 30 tiles in turn; the default grid: most wavefronts claim nothing."""
    name, w, h, tile, target, (mn, step, mx), _ = CASES["A-c3"]
    wl, (e_film, e_m2, e_waves, e_err) = _emulated(name, w, h, tile, None, target, mn, step, mx)
    assert wl.cfg.jobs_per_wave() == 30
    it = _integrator(wl)
    assert it.launch_info()[0] * (it.launch_info()[1] // 64) > 30
    full = _run(it, target, mn, step, mx, fused=True)
    it.set_tuning(grid_blocks=1)
    assert it.launch_info() == (1, 256)
    one = _run(it, target, mn, step, mx, fused=True)
    _assert_same(one, full, "one block vs the default grid")
    _assert_same(one, (e_film, e_m2, e_waves, e_err, None), "one block vs the emulated rule")


# -------------------------------------------------------------------------------------------------- 3. counters

PRODUCTION_COUNTERS = ("samples", "dda_steps", "stencils", "temp_stencils")  # (what the production kernels keep)


@pytest.mark.parametrize("case", ["B-c3", "B-c4-temperature"])
def test_counters_equal_the_rounds_driver(case):
    name, w, h, tile, target, (mn, step, mx), _ = CASES[case]
    wl = _wl(name, w, h, GRID_N, mx, tile)
    it = _integrator(wl)
    it.counters(reset=True)
    fused = _run(it, target, mn, step, mx, fused=True)
    c_f = it.counters(reset=True)
    _run(it, target, mn, step, mx, fused=False)
    c_r = it.counters(reset=True)
    for k in PRODUCTION_COUNTERS:
        assert c_f[k] == c_r[k] and (c_f[k] > 0 or k == "temp_stencils"), k
    assert (c_f["temp_stencils"] > 0) == (name == "c4")
    pixels = np.array([A.tile_rect(wl.cfg, t)[2] * A.tile_rect(wl.cfg, t)[3] for t in range(wl.cfg.jobs_per_wave())])
    assert c_f["samples"] == int((pixels * fused[2].astype(np.int64)).sum())


# -------------------------------------------------------------------------------------------------- 4. extremes

def test_extremes():
    name, (w, h, _) = "c3", ADAPTIVE["c3"]
    wl = _wl(name, w, h, GRID_N, MAX_W)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    # target 0: no tile ever stops (black tiles, whose estimate is 0, included): the uniform frame, byte for byte
    film, m2, waves, err, info = _run(it, 0.0, MIN_W, STEP_W, MAX_W, fused=True)
    uniform = torch.zeros_like(it.film)
    it.render_jobs(0, MAX_W * T, film=uniform)
    torch.cuda.synchronize()
    assert film.tobytes() == uniform.cpu().numpy().tobytes()
    assert (waves == MAX_W).all() and info["jobs_rendered"] == MAX_W * T and info["tiles_at_max"] == T
    assert info["rounds"] == 4 and (err == 0).any()  # (this frame has black tiles)
    _assert_same((film, m2, waves, err, info), _run(it, 0.0, MIN_W, STEP_W, MAX_W, fused=False), "target 0")
    # target inf: every tile stops at the first boundary
    film, m2, waves, err, info = _run(it, float("inf"), MIN_W, STEP_W, MAX_W, fused=True)
    assert (waves == MIN_W).all() and info["rounds"] == 1 and info["jobs_rendered"] == MIN_W * T
    first = torch.zeros_like(it.film)
    it.render_jobs(0, MIN_W * T, film=first)
    torch.cuda.synchronize()
    assert film.tobytes() == first.cpu().numpy().tobytes()
    _assert_same((film, m2, waves, err, info), _run(it, float("inf"), MIN_W, STEP_W, MAX_W, fused=False), "target inf")
    # a step that overshoots the cap is cut to it: 8, 28, 32
    _, (e_film, e_m2, e_waves, e_err) = _emulated(name, w, h, None, None, 0.2, 8, 20, 32)
    assert set(np.unique(e_waves)) <= {8, 28, 32} and (e_waves == 32).any() and (e_waves == 28).any()
    got = _run(it, 0.2, 8, 20, 32, fused=True)
    _assert_same(got, (e_film, e_m2, e_waves, e_err, None), "8 / 20 / 32 vs the emulated rule")
    _assert_same(got, _run(it, 0.2, 8, 20, 32, fused=False), "8 / 20 / 32 vs the rounds driver")


def test_single_pixel_mode():
    """c4 40 x 32 at pixel (20, 16): only that pixel's film and plane change."""
    name, w, h, sp, target = "c4", 40, 32, (20, 16), ADAPTIVE["c4"][2]
    wl, (e_film, e_m2, e_waves, e_err) = _emulated(name, w, h, None, sp, target, MIN_W, STEP_W, MAX_W)
    it = _integrator(wl)
    got = _run(it, target, MIN_W, STEP_W, MAX_W, fused=True)
    film, m2 = got[0], got[1]
    touched = (film != 0).any(-1)
    assert touched.sum() == 1 and touched[sp[1], sp[0]] and film[sp[1], sp[0], 3] >= MIN_W
    assert (m2 != 0).sum() <= 1 and (np.delete(m2.ravel(), sp[1] * w + sp[0]) == 0).all()
    _assert_same(got, (e_film, e_m2, e_waves, e_err, None), "single pixel vs the emulated rule")
    _assert_same(got, _run(it, target, MIN_W, STEP_W, MAX_W, fused=False), "single pixel vs the rounds driver")


# ---------------------------------------------------------------------------------------------- 5. housekeeping

def test_housekeeping():
    name, w, h, tile, target, (mn, step, mx), _ = CASES["B-c3"]
    wl, (e_film, e_m2, e_waves, e_err) = _emulated(name, w, h, tile, None, target, mn, step, mx)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    prev = _new_plane(it)
    it.set_film_moments(prev)  # an attachment of the caller's: back afterwards, never written by the call
    it.render_jobs(0, T)  # (the sample buffer exists: its size must not change)
    torch.cuda.synchronize()
    _, _, one = _reference(name, w, h, GRID_N, 0, 1, None, None, float(SENTINEL))
    _assert_bitwise(prev.cpu().numpy(), one[1], "the caller's plane before the call")
    before = it.film_order_info()
    a = _run(it, target, mn, step, mx, fused=True)
    after = it.film_order_info()
    assert after["ordered_launches"] == before["ordered_launches"] + 1
    assert after["atomic_launches"] == before["atomic_launches"] == 0
    assert after["buffer_bytes"] == before["buffer_bytes"] > 0
    b = _run(it, target, mn, step, mx, fused=True)
    assert it.film_order_info()["ordered_launches"] == before["ordered_launches"] + 2
    for x, y in zip(a[:4], b[:4]):  # two runs give identical bytes
        assert x.tobytes() == y.tobytes()
    assert a[4] == b[4]
    _assert_same(a, (e_film, e_m2, e_waves, e_err, None), "vs the emulated rule")
    # the previous attachment is back and unwritten: the next launch adds its wave to the caller's plane
    _assert_bitwise(prev.cpu().numpy(), one[1], "the caller's plane after the call")
    it.render_jobs(T, T)
    torch.cuda.synchronize()
    _, _, two = _reference(name, w, h, GRID_N, 0, 2, None, None, float(SENTINEL))
    _assert_bitwise(prev.cpu().numpy(), two[2], "the caller's plane after a further launch")


# ------------------------------------------------------------------------------------------------- 6. refusals

def _raw_call(it, film, m2, wv, er, res, params, fn=None, ctx=True):
    L = capi.lib()
    p = capi.AdaptiveParams(*params) if params is not None else None
    return L.vpt_gpu_render_adaptive_fused(
        it.h if ctx else None, C.byref(p) if p is not None else None,
        C.c_void_p(film.data_ptr()) if film is not None else None, C.c_void_p(m2.data_ptr()) if m2 is not None else None,
        wv.ctypes.data_as(C.POINTER(C.c_uint32)) if wv is not None else None,
        er.ctypes.data_as(C.POINTER(C.c_float)) if er is not None else None, C.byref(res) if res is not None else None,
        C.c_void_p(it.stream_handle()))


def test_refusals_leave_the_context_usable():
    name, w, h, tile, target, (mn, step, mx), _ = CASES["B-c3"]
    wl, want = _emulated(name, w, h, tile, None, target, mn, step, mx)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    L = capi.lib()
    film, m2 = torch.zeros_like(it.film), _new_plane(it, 0.0)
    wv, er, res = np.zeros(T, np.uint32), np.zeros(T, np.float32), capi.AdaptiveResult()
    good = (target, FLOOR, mn, step, mx)

    def call(params=good, **kw):
        a = dict(film=film, m2=m2, wv=wv, er=er, res=res)
        a.update(kw)
        return _raw_call(it, a["film"], a["m2"], a["wv"], a["er"], a["res"], params, ctx=a.get("ctx", True))

    def still_renders(what):
        torch.cuda.synchronize()
        assert film.cpu().numpy().tobytes() == np.zeros((h, w, 4), np.float32).tobytes(), f"{what}: something was rendered"
        assert (m2.cpu().numpy() == 0).all() and (wv == 0).all()
        _assert_same(_run(it, target, mn, step, mx, fused=True), want + (None,), what)

    for bad in ((0.1, FLOOR, 1, 8, 32), (0.1, FLOOR, 8, 0, 32), (0.1, FLOOR, 8, 8, 7), (-0.1, FLOOR, 8, 8, 32),
                (float("nan"), FLOOR, 8, 8, 32), (0.1, 0.0, 8, 8, 32), (0.1, -1.0, 8, 8, 32)):
        assert call(bad) == VPT_E_INVALID, bad
    assert call(ctx=False) == VPT_E_INVALID and call(None) == VPT_E_INVALID
    assert call(m2=None) == VPT_E_INVALID and call(wv=None) == VPT_E_INVALID and call(er=None) == VPT_E_INVALID
    still_renders("after bad parameters and null arguments")
    it.set_rng_mode(capi.VPT_RNG_PIXEL)
    assert call() == VPT_E_INVALID
    it.set_rng_mode(capi.VPT_RNG_REFERENCE)
    still_renders("after the pixel RNG mode")
    it.set_film_order(capi.VPT_FILM_ATOMIC)
    assert call() == VPT_E_STATE and b"ordered film" in L.vpt_last_error()
    it.set_film_order(capi.VPT_FILM_ORDERED)
    still_renders("after the atomic film mode")
    granted = C.c_uint64(2)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open")
    assert call() == VPT_E_STATE and b"frame" in L.vpt_last_error()
    granted = C.c_uint64(0)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open (close)")
    still_renders("after an open frame")
    assert call(res=None) == capi.VPT_OK  # (the result struct is optional)
    np.testing.assert_array_equal(wv, want[2])


def test_tiles_of_more_than_256_pixels_are_refused():
    wl = _wl("c3", 48, 40, GRID_N, MAX_W, (24, 16))
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    film, m2 = torch.zeros_like(it.film), _new_plane(it, 0.0)
    wv, er = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    assert _raw_call(it, film, m2, wv, er, None, (0.2, FLOOR, MIN_W, STEP_W, MAX_W)) == VPT_E_INVALID
    assert b"256" in capi.lib().vpt_last_error()
    torch.cuda.synchronize()
    assert not film.cpu().numpy().any() and not wv.any()
    _, _, waves, _, info = _run(it, 0.2, MIN_W, STEP_W, MAX_W, fused=False)
    assert info["jobs_rendered"] == int(waves.sum()) > 0  # the rounds driver renders such tiles


def test_open_feed_refusal():
    """While a feed of the context is launched and not closed the call is refused (it allocates, and an allocation must
    not wait for a launch that holds the device); after the close it renders."""
    name, w, h, waves = "c3", 64, 48, 16
    mn, step, mx, target = 8, 8, 16, 0.2
    wl, want = _emulated(name, w, h, None, None, target, mn, step, mx)
    it = _integrator(wl)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()  # (the cost pass refuses while a feed is open: done before)
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film, film, m2 = torch.zeros_like(it.film), torch.zeros_like(it.film), _new_plane(it, 0.0)
    wv, er = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    assert _raw_call(it, film, m2, wv, er, None, (target, FLOOR, mn, step, mx)) == VPT_E_STATE
    assert b"feed" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    np.testing.assert_array_equal(feed_film.cpu().numpy()[..., 3], float(waves))
    assert not film.cpu().numpy().any() and not m2.cpu().numpy().any() and not wv.any()  # the refused call rendered nothing
    _assert_same(_run(it, target, mn, step, mx, fused=True), want + (None,), "after the feed")


# ------------------------------------------------------------------------------------------------------- 7. CLI

def test_cli_adaptive_fused(tmp_path, capfd):
    from volume_path_tracer_amd.__main__ import main
    from volume_path_tracer_amd.scenes import read_configuration

    cfg = read_configuration(SCENE_DIR / "fire.json")
    cfg.output_size[0], cfg.output_size[1] = 40, 32
    T = cfg.jobs_per_wave()
    common = [str(SCENE_DIR / "fire.json"), str(tmp_path / "o.png"), "--synthetic", "fire", "--size", "40x32",
              "--spp", "16", "--adaptive", "0.05", "--min-spp", "8", "--spp-step", "8"]
    # in-process: the test runner's own GPU context (one process on the card)
    rc = main(common + ["--adaptive-fused", "--waves-out", str(tmp_path / "w.npy"), "--film-out", str(tmp_path / "film.npy")])
    assert rc == 0
    assert (tmp_path / "o.png").read_bytes()[:8] == b"\x89PNG\r\n\x1a\n"
    waves = np.load(tmp_path / "w.npy")
    assert waves.dtype == np.uint32 and waves.shape == (T,) and set(np.unique(waves)) <= {8, 16}
    film = np.load(tmp_path / "film.npy")
    for t in range(T):  # the film's sample counts are the wave map
        assert (film[..., 3][A.tile_mask(cfg, [t])] == waves[t]).all()
    err = capfd.readouterr().err
    assert f"{int(waves.sum())} of {16 * T} jobs" in err and "fused" in err  # the summary line names the driver
