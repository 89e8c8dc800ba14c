"""Light groups on the device (vpt_gpu_set_light_groups, vpt_gpu_relight): the emission, sun and sky planes of one render
against the oracle's isolated films (tests/light_groups_lib.py isolated_oracle: the oracle run with the other two
sources switched off), byte for byte up to the sign of a zero -- on the plain and the band kernels, tile lists, split
launches, run skipping on and off, with a moment plane beside them -- and the relight kernel against image.relight.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import adaptive_ref as A
import light_groups_lib as LG
from volume_path_tracer_amd import capi, image
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6
N = 64  # grid_n
_cache = {}


def _grids(wl):
    key = ("grids", wl.density_kind, wl.temperature)
    if key not in _cache:
        _cache[key] = (SynthGrid(wl.density_kind, N).grid(), SynthGrid(2, N).grid() if wl.temperature else None)
    return _cache[key]


def _integrator(wl):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(wl.cfg, *_grids(wl), device=0)


def _iso(name, w, h, waves, tweak=None):
    """The oracle's plain and isolated films of `waves` whole waves, computed once per case."""
    key = ("iso", name, w, h, waves, tweak)
    if key not in _cache:
        wl = _wl(name, w, h, waves, tweak)
        _cache[key] = LG.isolated_oracle(wl.cfg, *_grids(wl), 0, waves * wl.cfg.jobs_per_wave())
    return _cache[key]


def _wl(name, w, h, waves, tweak=None):
    wl = workload(name, width=w, height=h, spp=waves, grid_n=N)
    if tweak == "sun_off":
        wl.cfg.worker_parameters.distant_light_multiplier = 0.0
    elif tweak == "no_emission":
        wl.cfg.volume_parameters.le_scale = 0.0
    return wl


def _planes(it, fill=0.0):
    return torch.full((3, it.cfg.height, it.cfg.width, 4), fill, dtype=torch.float32, device=it.dev)


def _render(it, how, waves, groups=None, m2=None, tiles=None, fill=0.0):
    """One call with the attachments given -> the film (numpy).  how: jobs | tiles | list."""
    film = torch.full_like(it.film, fill)
    T = it.cfg.jobs_per_wave()
    it.set_light_groups(groups)
    it.set_film_moments(m2)
    try:
        if how == "jobs":
            it.render_jobs(0, waves * T, film=film)
        elif how == "tiles":
            it.render_tiles(0, T, 1, waves, film=film)
        else:
            it.render_tile_list(tiles, 1, waves, film=film)
        torch.cuda.synchronize()
    finally:
        it.set_light_groups(None)
        it.set_film_moments(None)
    return film.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_groups(got, iso, what, mask=None):
    for g, name in enumerate(LG.GROUPS):
        a, b = got[g], iso["group_films"][g]
        if mask is not None:
            assert np.isnan(a[~mask]).all(), f"{what}: {name}: a pixel outside the list was touched"
            a, b = a[mask], b[mask]
        bad = _bits(a + np.float32(0)) != _bits(b + np.float32(0))
        assert not bad.any(), f"{what}: {name}: {int(bad.sum())} of {bad.size} values differ from the isolated oracle film"


# ------------------------------------------------------------------------------------------ 1. ragged tiles, 3 waves

@pytest.mark.parametrize("name", ["c3", "c4"])
def test_planes_are_the_isolated_oracle_films(name):
    """20 x 12 pixels (ragged 8 x 8 tiles), 3 waves (a partly filled band group): render_jobs, render_tiles over the
    whole band and render_tile_list over tiles {0, 2, 5}."""
    w, h, waves = 20, 12, 3
    wl = _wl(name, w, h, waves)
    iso = _iso(name, w, h, waves)
    it = _integrator(wl)
    for how in ("jobs", "tiles"):
        gp = _planes(it)
        film = _render(it, how, waves, groups=gp)
        assert np.array_equal(_bits(film), _bits(iso["film"])), f"{how}: the beauty film differs from the oracle's"
        assert np.array_equal(_bits(film), _bits(_render(it, how, waves))), f"{how}: the film changes with groups attached"
        _assert_groups(gp.cpu().numpy(), iso, f"{name} {how}")
    tiles = [0, 2, 5]
    mask = A.tile_mask(wl.cfg, tiles)
    gp = _planes(it, float("nan"))
    gp[:, torch.from_numpy(mask).to(gp.device)] = 0.0
    start = torch.full_like(it.film, float("nan"))
    start[torch.from_numpy(mask).to(gp.device)] = 0.0

    def list_film(groups):
        film = start.clone()
        it.set_light_groups(groups)
        try:
            it.render_tile_list(tiles, 1, waves, film=film)
            torch.cuda.synchronize()
        finally:
            it.set_light_groups(None)
        return film.cpu().numpy()

    film = list_film(gp)
    assert np.isnan(film[~mask]).all() and np.array_equal(_bits(film[mask]), _bits(iso["film"][mask]))
    assert np.array_equal(_bits(film), _bits(list_film(None)))
    _assert_groups(gp.cpu().numpy(), iso, f"{name} list", mask)


# ------------------------------------------------------------------------------- 2. 70 waves: past the 64-wave group

@pytest.mark.parametrize("name", ["c3", "c4"])
def test_seventy_waves_both_kernels_runs_and_split_launches(name):
    w, h, waves = 16, 8, 70
    wl = _wl(name, w, h, waves)
    iso = _iso(name, w, h, waves)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    results = {}
    for runs in ((0, 1) if name == "c3" else (-1,)):
        it.set_run_skipping(runs)
        for how in ("jobs", "tiles"):
            for split in (False, True):
                # 48 bytes per sample with groups: half the launch's buffer -> at least two launches
                it.set_film_order(capi.VPT_FILM_ORDERED, waves * T * 64 * 48 // 2 if split else 0)
                before = it.film_order_info()["ordered_launches"]
                gp = _planes(it)
                film = _render(it, how, waves, groups=gp)
                launches = it.film_order_info()["ordered_launches"] - before
                assert (launches >= 2) if split else (launches == 1), (runs, how, split, launches)
                if not split:
                    assert it.film_order_info()["buffer_bytes"] >= waves * T * 64 * 48
                assert np.array_equal(_bits(film), _bits(iso["film"])), (runs, how, split)
                results[(runs, how, split)] = gp.cpu().numpy()
    it.set_film_order(capi.VPT_FILM_ORDERED, 0)
    first = next(iter(results.values()))
    _assert_groups(first, iso, name)
    for key, planes in results.items():
        assert np.array_equal(_bits(planes), _bits(first)), f"{key}: the planes' bytes differ between launches"


# ----------------------------------------------------------------------------------------------- 3. a source off

@pytest.mark.parametrize("name,tweak,group", [("c3", "sun_off", 1), ("c4", "no_emission", 0)])
def test_a_switched_off_source_leaves_counts_and_plus_zero(name, tweak, group):
    w, h, waves = 20, 12, 3
    wl = _wl(name, w, h, waves, tweak)
    iso = _iso(name, w, h, waves, tweak)
    it = _integrator(wl)
    for how in ("jobs", "tiles"):
        gp = _planes(it)
        film = _render(it, how, waves, groups=gp)
        planes = gp.cpu().numpy()
        assert np.array_equal(_bits(film), _bits(iso["film"]))
        assert (planes[group][..., 3] == waves).all()
        assert (_bits(planes[group][..., :3]) == 0).all(), "the switched-off source's plane is not +0.0"
        _assert_groups(planes, iso, f"{name} {tweak} {how}")
    if name == "c3":  # no temperature grid: the emission plane holds the counts and +0.0 as well
        assert (planes[0][..., 3] == waves).all() and (_bits(planes[0][..., :3]) == 0).all()


# --------------------------------------------------------------------------------------------- 4. both attachments

@pytest.mark.parametrize("how", ["jobs", "tiles", "list"])
def test_moment_plane_and_groups_combine(how):
    w, h, waves = 20, 12, 3
    wl = _wl("c4", w, h, waves)
    it = _integrator(wl)
    tiles = [0, 2, 5]

    def run(with_m2, with_groups):
        m2 = torch.zeros((h, w), dtype=torch.float32, device=it.dev) if with_m2 else None
        gp = _planes(it) if with_groups else None
        film = _render(it, how, waves, groups=gp, m2=m2, tiles=tiles)
        return film, (m2.cpu().numpy() if with_m2 else None), (gp.cpu().numpy() if with_groups else None)

    f_b, m_b, g_b = run(True, True)
    f_m, m_m, _ = run(True, False)
    f_g, _, g_g = run(False, True)
    assert np.array_equal(_bits(f_b), _bits(f_m)) and np.array_equal(_bits(f_b), _bits(f_g))
    assert np.array_equal(_bits(m_b), _bits(m_m)) and (m_b != 0).any()
    assert np.array_equal(_bits(g_b), _bits(g_g)) and (g_b[..., :3] != 0).any()


# ------------------------------------------------------------------------------------------- 5. the scaling identity

def test_power_of_two_gains_scale_the_planes_exactly():
    """set_scene with the sun x 2, the sky x 0.5 and le_scale x 4 on the same context: each plane is the old one times
    its gain byte for byte (a power of two commutes with every rounding while nothing under- or overflows)."""
    from volume_path_tracer_amd.render import render_uniform
    from volume_path_tracer_amd.scenes import light_gains

    w, h, waves = 20, 12, 3
    wl = _wl("c4", w, h, waves)
    it = _integrator(wl)
    _, _, g0 = render_uniform(it, groups=True)
    g0 = g0.cpu().numpy()
    mag = np.abs(g0[..., :3][g0[..., :3] != 0])
    assert mag.size and mag.min() >= 2.0 ** -100 and mag.max() <= 2.0 ** 100
    cfg2 = wl.cfg.copy()
    cfg2.worker_parameters.distant_light_multiplier = wl.cfg.worker_parameters.distant_light_multiplier * 2
    cfg2.worker_parameters.infinite_light_multiplier = wl.cfg.worker_parameters.infinite_light_multiplier * 0.5
    cfg2.volume_parameters.le_scale = wl.cfg.volume_parameters.le_scale * 4
    it.set_scene(cfg2)
    film2, _, g1 = render_uniform(it, groups=True)
    g1 = g1.cpu().numpy()
    k = light_gains(wl.cfg, cfg2)
    assert np.array_equal(k, np.array([[4] * 3, [2] * 3, [0.5] * 3], np.float32))
    for g, name in enumerate(LG.GROUPS):
        want = g0[g].copy()
        want[..., :3] = want[..., :3] * k[g]
        assert np.array_equal(_bits(g1[g]), _bits(want)), name
        assert (g0[g][..., :3] != 0).any(), name
    # and the attachment's restore: the context has none now
    assert getattr(it, "_groups", None) is None


# ----------------------------------------------------------------------------------------------------- 6. relight

def test_relight_kernel_equals_the_numpy_restatement():
    from volume_path_tracer_amd.render import render_uniform

    w, h, waves = 20, 12, 3
    wl = _wl("c4", w, h, waves)
    it = _integrator(wl)
    _, _, gp = render_uniform(it, groups=True)
    k = np.array([[0.3, 1.7, 2.9], [1.1, 0.7, 0.2], [5.3, 0.9, 1.3]], np.float32)
    out = it.relight(gp, k)
    assert torch.is_tensor(out)
    torch.cuda.synchronize()
    g_host = gp.cpu().numpy()
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(image.relight(g_host, k)))
    assert np.array_equal(_bits(it.relight(g_host, k)), _bits(image.relight(g_host, k)))  # numpy in, numpy out
    # a hand-made frame: zeros, negative values, a pixel with w = 0
    rng = np.random.default_rng(11)
    hand = (rng.standard_normal((3, h, w, 4)) * 10.0 ** rng.integers(-6, 6, (3, h, w, 4))).astype(np.float32)
    hand[:, 0, 0] = 0.0
    hand[1, 0, 1] = -0.0
    hand[0, 1, 1, 3] = 0.0
    hand[..., 3] = np.abs(hand[..., 3])
    hand[0, 1, 1, 3] = 0.0
    got = it.relight(hand, k)
    assert np.array_equal(_bits(got), _bits(image.relight(hand, k))) and got[1, 1, 3] == 0.0
    L = capi.lib()
    kp = k.ctypes.data_as(C.POINTER(C.c_float))
    base = gp.data_ptr()
    for alias in (base, base + h * w * 16, base + 2 * h * w * 16 + 16):
        assert L.vpt_gpu_relight(it.h, C.c_void_p(base), kp, C.c_void_p(alias), None) == VPT_E_INVALID
        assert b"alias" in L.vpt_last_error()
    assert L.vpt_gpu_relight(it.h, None, kp, C.c_void_p(base), None) == VPT_E_INVALID
    with pytest.raises(ValueError):
        it.relight(g_host[:2], k)


# ------------------------------------------------------------------------------------------ 7. sanity on the sum

@pytest.mark.parametrize("name", ["c3", "c4"])
def test_groups_sum_to_the_beauty_within_reassociation(name):
    """Not the parity check: it catches a group dropped or added twice (an error of order 1).  Re-associating n
    non-negative terms moves a sum by at most (n - 1) 2^-24 relative: < 1e-3 for n <= 16384, and the frame's terms --
    samples + shadow rays + density evaluations, from a records launch's counters -- stay under that."""
    from volume_path_tracer_amd.render import render_uniform

    w, h, waves = 20, 12, 3
    wl = _wl(name, w, h, waves)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    it.counters(reset=True)
    rec = torch.zeros((waves * T * 64, 3), dtype=torch.float32, device=it.dev)
    it.render_jobs(0, waves * T, film=torch.zeros_like(it.film), records=rec)
    torch.cuda.synchronize()
    cnt = it.counters(reset=True)
    n = cnt["samples"] + cnt["shadow_rays"] + cnt["density_evals"]
    assert cnt["samples"] == w * h * waves and 0 < n <= 16384, cnt
    film, _, gp = render_uniform(it, groups=True)
    film, gp = film.cpu().numpy().astype(np.float64), gp.cpu().numpy()
    relit = it.relight(gp, np.ones((3, 3), np.float32)).astype(np.float64)
    total = gp.astype(np.float64).sum(axis=0)
    nz = film[..., :3] != 0
    assert nz.any()
    for what, s in (("sum", total), ("relit", relit)):
        err = np.abs(s[..., :3] - film[..., :3])[nz] / np.abs(film[..., :3])[nz]
        assert err.max() <= 1e-3, (what, err.max())
        assert np.array_equal(s[..., :3][~nz], film[..., :3][~nz])
    assert np.array_equal(relit[..., 3], film[..., 3])


# ------------------------------------------------------------------------------------------------ 8. state rules

def test_groups_refuse_launches_that_add_with_atomics():
    w, h, waves = 20, 12, 3
    wl = _wl("c3", w, h, waves)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    L = capi.lib()
    film, gp = torch.zeros_like(it.film), _planes(it, 0.25)
    fptr, gptr, s = C.c_void_p(film.data_ptr()), C.c_void_p(gp.data_ptr()), C.c_void_p(it.stream_handle())
    assert L.vpt_gpu_set_light_groups(None, gptr) == VPT_E_INVALID
    assert L.vpt_gpu_set_light_groups(it.h, C.c_void_p(gp.data_ptr() + 4)) == VPT_E_INVALID  # not 16-byte aligned
    it.set_film_order(capi.VPT_FILM_ATOMIC)
    assert L.vpt_gpu_set_light_groups(it.h, gptr) == VPT_E_STATE
    it.set_film_order(capi.VPT_FILM_ORDERED)
    granted = C.c_uint64(2)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open")
    assert L.vpt_gpu_set_light_groups(it.h, gptr) == VPT_E_STATE and b"frame" in L.vpt_last_error()
    granted = C.c_uint64(0)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open (close)")
    it.set_light_groups(gp)
    rec = torch.zeros((T * 64, 3), dtype=torch.float32, device=it.dev)
    assert L.vpt_gpu_render_jobs_records(it.h, 0, T, fptr, C.c_void_p(rec.data_ptr()), s) == VPT_E_STATE
    assert b"light groups" in L.vpt_last_error()
    it.set_rng_mode(capi.VPT_RNG_PIXEL)
    assert L.vpt_gpu_render_jobs(it.h, 0, T, fptr, s) == VPT_E_STATE
    it.set_rng_mode(capi.VPT_RNG_REFERENCE)
    it.set_film_order(capi.VPT_FILM_ATOMIC)
    assert L.vpt_gpu_render_jobs(it.h, 0, T, fptr, s) == VPT_E_STATE
    it.set_film_order(capi.VPT_FILM_ORDERED)
    granted = C.c_uint64(2)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open")
    assert L.vpt_gpu_render_jobs(it.h, 0, T, fptr, s) == VPT_E_STATE and b"frame" in L.vpt_last_error()
    granted = C.c_uint64(0)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open (close)")
    # the fused adaptive driver does not write the planes
    m2 = torch.zeros((h, w), dtype=torch.float32, device=it.dev)
    p, res = capi.AdaptiveParams(0.1, 1e-3, 2, 1, 3), capi.AdaptiveResult()
    wv, er = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    assert L.vpt_gpu_render_adaptive_fused(it.h, C.byref(p), fptr, C.c_void_p(m2.data_ptr()),
                                           wv.ctypes.data_as(C.POINTER(C.c_uint32)), er.ctypes.data_as(C.POINTER(C.c_float)),
                                           C.byref(res), s) == VPT_E_STATE
    assert b"light groups" in L.vpt_last_error()
    torch.cuda.synchronize()
    assert film.cpu().numpy().tobytes() == np.zeros((h, w, 4), np.float32).tobytes()  # nothing was rendered
    assert (gp.cpu().numpy() == np.float32(0.25)).all()
    # the attachment survives set_scene and set_volume, and the context still renders film and planes
    it.set_scene(wl.cfg)
    it.set_volume(*_grids(wl))
    gp.zero_()
    it.render_jobs(0, waves * T, film=film)
    torch.cuda.synchronize()
    it.set_light_groups(None)
    iso = _iso("c3", w, h, waves)
    assert np.array_equal(_bits(film.cpu().numpy()), _bits(iso["film"]))
    _assert_groups(gp.cpu().numpy(), iso, "after the refusals")


def test_feeds_never_write_the_planes_and_a_growing_buffer_is_refused():
    w, h, waves = 64, 48, 16
    wl = _wl("c3", w, h, waves)
    it = _integrator(wl)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()  # (the cost pass refuses while a feed is open: done before)
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film, film, gp = torch.zeros_like(it.film), torch.zeros_like(it.film), _planes(it, 0.25)
    torch.cuda.synchronize()
    it.set_light_groups(gp)  # attached before the feed opens
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    fptr, own = C.c_void_p(film.data_ptr()), C.c_void_p(it.stream_handle())
    assert L.vpt_gpu_render_jobs(it.h, 0, waves * T, fptr, own) == VPT_E_STATE and b"grow" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    it.set_light_groups(None)
    np.testing.assert_array_equal(feed_film.cpu().numpy()[..., 3], float(waves))
    assert film.cpu().numpy().tobytes() == np.zeros((h, w, 4), np.float32).tobytes()  # the refused call rendered nothing
    assert (gp.cpu().numpy() == np.float32(0.25)).all()  # and the feed never wrote the planes


def test_rounds_driver_renders_the_groups_and_the_fused_one_refuses():
    from volume_path_tracer_amd.render import render_adaptive, render_uniform

    w, h, waves = 20, 12, 6
    wl = _wl("c4", w, h, waves)
    it = _integrator(wl)
    film_u, _, g_u = render_uniform(it, groups=True)
    film, wv, err, info, g_a = render_adaptive(it, 0.0, min_waves=2, step_waves=2, max_waves=waves, groups=True)
    assert (wv == waves).all()  # (target 0: no tile ever stops)
    assert np.array_equal(_bits(film), _bits(film_u.cpu().numpy()))
    assert np.array_equal(_bits(g_a), _bits(g_u.cpu().numpy())) and (g_a[..., :3] != 0).any()
    with pytest.raises(ValueError):
        render_adaptive(it, 0.1, min_waves=2, step_waves=2, max_waves=waves, fused=True, groups=True)
    assert len(render_adaptive(it, 0.0, min_waves=2, step_waves=2, max_waves=2)) == 4  # without the keyword: as before
    assert torch.is_tensor(render_uniform(it, moments=False)) and len(render_uniform(it)) == 2


# -------------------------------------------------------------------------------------------------------- 9. CLI

def test_cli_light_groups_and_relight(tmp_path):
    from volume_path_tracer_amd.__main__ import main

    scene = str(SCENE_DIR / "fire.json")
    common = ["--synthetic", f"fire:{N}", "--size", "16x16", "--spp", "2"]  # (two samples: any order adds the same)
    assert main([scene, str(tmp_path / "plain.png"), *common]) == 0
    assert main([scene, str(tmp_path / "o.png"), *common, "--light-groups", "--groups-out", str(tmp_path / "g.npy"),
                 "--film-out", str(tmp_path / "film.npy")]) == 0
    assert (tmp_path / "o.png").read_bytes() == (tmp_path / "plain.png").read_bytes()
    g = np.load(tmp_path / "g.npy")
    assert g.dtype == np.float32 and g.shape == (3, 16, 16, 4) and (g[..., 3] == 2).all() and (g[..., :3] != 0).any()
    for k, name in enumerate(LG.GROUPS):
        png = image.decode_png((tmp_path / f"o.{name}.png").read_bytes())
        assert np.array_equal(png, image.film_to_image(g[k])), name
    spec, gains = "emission=2.5,sun=0.3:1.1:0.7,sky=0", [[2.5] * 3, [0.3, 1.1, 0.7], [0.0] * 3]
    assert main([scene, str(tmp_path / "r.png"), *common, "--relight", spec, "--alpha"]) == 0
    rgba = image.decode_png((tmp_path / "r.png").read_bytes())
    assert rgba.shape == (16, 16, 4) and np.array_equal(rgba[..., :3], image.film_to_image(image.relight(g, gains)))
    assert (tmp_path / "r.sun.png").exists()  # --relight implies --light-groups
    # --relight-from: a child process that sees no device reproduces --relight's PNG
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    r = subprocess.run([sys.executable, "-m", "volume_path_tracer_amd", "unused.json", str(tmp_path / "host.png"),
                        "--relight-from", str(tmp_path / "g.npy"), "--relight", spec], env=env, cwd=str(LG.ROOT),
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert np.array_equal(image.decode_png((tmp_path / "host.png").read_bytes()), rgba[..., :3])
    # out of scope with groups: refused before a device is touched (the scene file is never read)
    for flag in ("--denoise", "--alpha-foreground", "--adaptive-fused"):
        assert main(["missing.json", str(tmp_path / "x.png"), "--light-groups", flag]) == 1
        assert not (tmp_path / "x.png").exists()
    assert main(["missing.json", str(tmp_path / "x.png"), "--relight", "moon=2"]) == 1
    # the rounds driver with groups
    assert main([scene, str(tmp_path / "a.png"), *common, "--spp", "4", "--adaptive", "0.05", "--min-spp", "2", "--spp-step",
                 "2", "--groups-out", str(tmp_path / "ga.npy"), "--film-out", str(tmp_path / "fa.npy")]) == 0
    ga, fa = np.load(tmp_path / "ga.npy"), np.load(tmp_path / "fa.npy")
    assert np.array_equal(ga[0][..., 3], fa[..., 3]) and np.array_equal(ga[2][..., 3], fa[..., 3])
