"""Camera motion blur on the device (vpt_gpu_set_shutter): wave k renders through entry k % n of the shutter table and
nothing else changes, so the film is, bit for bit, the ordered fp32 sum of the films the unchanged oracle renders wave
by wave, each with that wave's camera (tests/shutter_lib.py Reference) -- on the plain and the band kernels, tile
lists, split launches, run skipping on and off, with a moment plane and light-group planes attached, through the rounds
driver of adaptive sampling, across set_scene / set_volume -- and the state and validation rules of the call.
"""
import ctypes as C

import numpy as np
import pytest

import adaptive_ref as A
import light_groups_lib as LG
import shutter_lib as SH
from volume_path_tracer_amd import capi, scenes
from volume_path_tracer_amd.scenes import SynthGrid, workload

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6
N = 64  # grid_n
_cache = {}


def _wl(name, w, h, waves):
    return workload(name, width=w, height=h, spp=waves, grid_n=N)


def _grids(wl):
    key = ("grids", wl.density_kind, wl.temperature)
    if key not in _cache:
        _cache[key] = (SynthGrid(wl.density_kind, N).grid(), SynthGrid(2, N).grid() if wl.temperature else None)
    return _cache[key]


def _integrator(wl):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(wl.cfg, *_grids(wl), device=0)


def _cameras(cfg, cams):
    return SH.three_cameras(cfg) if cams == "three" else SH.moving_cameras(cfg, cams)


def _ref(name, w, h, waves, cams, groups=False):
    """The oracle's per-wave runs of a case, computed once."""
    key = ("ref", name, w, h, waves, cams, groups)
    if key not in _cache:
        wl = _wl(name, w, h, waves)
        _cache[key] = SH.Reference(wl.cfg, *_grids(wl), _cameras(wl.cfg, cams), waves, groups=groups)
    return _cache[key]


def _render(it, how, waves, tiles=None, fill=0.0, first_wave=1):
    """One call -> the film (numpy).  how: jobs | tiles | list."""
    film = torch.full_like(it.film, fill)
    T = it.cfg.jobs_per_wave()
    if how == "jobs":
        it.render_jobs((first_wave - 1) * T, waves * T, film=film)
    elif how == "tiles":
        it.render_tiles(0, T, first_wave, waves, film=film)
    else:
        it.render_tile_list(tiles, first_wave, waves, film=film)
    torch.cuda.synchronize()
    return film.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------- 1. three unlike cameras, every launch kind

@pytest.mark.parametrize("name", ["c3", "c4"])
def test_film_is_the_ordered_sum_of_the_oracle_wave_films(name):
    """20 x 12 pixels (ragged 8 x 8 tiles), 3 waves, 3 cameras (position, look, vfov): render_jobs, render_tiles and
    render_tile_list over tiles {0, 2, 5}, run skipping on and off."""
    w, h, waves = 20, 12, 3
    wl = _wl(name, w, h, waves)
    ref = _ref(name, w, h, waves, "three")
    want = ref.film()
    it = _integrator(wl)
    still = _render(it, "jobs", waves)
    it.set_shutter(_cameras(wl.cfg, "three"))
    assert it.shutter_info() == 3
    tiles = [0, 2, 5]
    mask = A.tile_mask(wl.cfg, tiles)
    for runs in ((0, 1) if name == "c3" else (-1,)):
        it.set_run_skipping(runs)
        for how in ("jobs", "tiles"):
            film = _render(it, how, waves)
            assert np.array_equal(_bits(film), _bits(want)), f"{name} runs={runs} {how}: differs from the reference"
        # (NaN outside the list: a touched pixel would show; the listed tiles start at zero)
        start = torch.full_like(it.film, float("nan"))
        start[torch.from_numpy(mask).to(start.device)] = 0.0
        lf = start.clone()
        it.render_tile_list(tiles, 1, waves, film=lf)
        torch.cuda.synchronize()
        lf = lf.cpu().numpy()
        assert np.isnan(lf[~mask]).all(), "a pixel outside the list was touched"
        assert np.array_equal(_bits(lf[mask]), _bits(want[mask])), f"{name} runs={runs} list"
    assert not np.array_equal(_bits(still), _bits(want)), "the cameras do not matter: a wrong choice of case"
    # waves 2 .. 3 alone: the entry follows the job id's wave, not the launch's first job
    later = _render(it, "jobs", 2, first_wave=2)
    two = np.zeros_like(want)
    for k in (1, 2):
        two = two + ref.wave_films[k]
    assert np.array_equal(_bits(later), _bits(two))
    assert np.array_equal(_bits(_render(it, "tiles", 2, first_wave=2)), _bits(two))


# ---------------------------------------------- 2. a full wavefront of one tile's waves, 64 cameras, two that wrap

@pytest.mark.parametrize("cams", [64, 5])
def test_sixty_six_waves_a_camera_per_lane(cams):
    """16 x 8 pixels (two tiles), 66 waves: under the same-tile order a wavefront's 64 lanes are 64 waves of one tile,
    each with a camera of its own; waves 64 and 65 wrap.  n = 5: a modulus that is no power of two."""
    w, h, waves = 16, 8, 66
    wl = _wl("c3", w, h, waves)
    want = _ref("c3", w, h, waves, cams).film()
    it = _integrator(wl)
    it.set_shutter(_cameras(wl.cfg, cams))
    T = wl.cfg.jobs_per_wave()
    for how in ("jobs", "tiles"):
        assert np.array_equal(_bits(_render(it, how, waves)), _bits(want)), how
    # one block: the launch is no longer spread one job per wavefront -- each of its four wavefronts' 64 lanes holds
    # a job of its own, consecutive waves of one tile, so one load instruction reads up to 64 different entries
    it.set_tuning(grid_blocks=1)
    for how in ("jobs", "tiles"):
        assert np.array_equal(_bits(_render(it, how, waves)), _bits(want)), f"{how}, one block"
    # 3. a launch split by max_bytes (12 bytes per sample: half the launch's buffer) is the same bytes
    for how in ("jobs", "tiles"):
        it.set_film_order(capi.VPT_FILM_ORDERED, waves * T * 64 * 12 // 2)
        before = it.film_order_info()["ordered_launches"]
        film = _render(it, how, waves)
        assert it.film_order_info()["ordered_launches"] - before >= 2, how
        assert film.tobytes() == want.tobytes(), f"{how}: the split launch differs"
    it.set_film_order(capi.VPT_FILM_ORDERED, 0)


# --------------------------------------------------------------- 4. identical entries, one entry, and detaching

def test_identical_entries_one_entry_and_detach():
    w, h, waves = 20, 12, 3
    wl = _wl("c4", w, h, waves)
    it = _integrator(wl)
    still = {how: _render(it, how, waves) for how in ("jobs", "tiles")}
    it.set_shutter([{}] * 7)  # seven times the scene's own camera
    assert it.shutter_info() == 7
    for how in ("jobs", "tiles"):
        assert _render(it, how, waves).tobytes() == still[how].tobytes(), how
    other = SH.three_cameras(wl.cfg)[0]
    it.set_shutter([other])
    one = _render(it, "jobs", waves)
    it.set_shutter(None)
    assert it.shutter_info() == 0
    for how in ("jobs", "tiles"):
        assert _render(it, how, waves).tobytes() == still[how].tobytes(), f"{how}: detached"
    it.set_camera(**other)
    assert _render(it, "jobs", waves).tobytes() == one.tobytes() and one.tobytes() != still["jobs"].tobytes()


# ----------------------------------------------------------------------------- 5. moment plane and group planes

@pytest.mark.parametrize("how", ["jobs", "tiles"])
def test_moment_plane_and_group_planes_keep_their_contracts(how):
    w, h, waves = 20, 12, 3
    wl = _wl("c4", w, h, waves)
    ref = _ref("c4", w, h, waves, "three", groups=True)
    films, m2s = ref.states()
    it = _integrator(wl)
    it.set_shutter(_cameras(wl.cfg, "three"))
    m2 = torch.zeros((h, w), dtype=torch.float32, device=it.dev)
    gp = torch.zeros((3, h, w, 4), dtype=torch.float32, device=it.dev)
    it.set_film_moments(m2)
    it.set_light_groups(gp)
    try:
        film = _render(it, how, waves)
    finally:
        it.set_film_moments(None)
        it.set_light_groups(None)
    assert np.array_equal(_bits(film), _bits(ref.film())) and np.array_equal(_bits(film), _bits(films[waves]))
    assert np.array_equal(_bits(m2.cpu().numpy()), _bits(m2s[waves])) and (m2s[waves] != 0).any()
    got, want = gp.cpu().numpy(), ref.group_films()
    for g, what in enumerate(LG.GROUPS):
        assert LG.same_but_zero_sign(got[g], want[g]), f"{how}: {what}: differs from the wave-by-wave isolated reference"
        assert (want[g][..., :3] != 0).any(), what
    assert np.array_equal(_bits(film), _bits(_render(it, how, waves))), "the film changes with the planes attached"


# --------------------------------------------------------------------------------------------- 6. the rounds driver

def test_rounds_driver_renders_each_tile_through_its_waves_cameras():
    from volume_path_tracer_amd.render import render_adaptive, render_uniform

    w, h, waves = 20, 12, 6
    wl = _wl("c4", w, h, waves)
    ref = _ref("c4", w, h, waves, "three")
    films, m2s = ref.states()
    it = _integrator(wl)
    it.set_shutter(_cameras(wl.cfg, "three"))
    uniform, m2_u = (t.cpu().numpy() for t in render_uniform(it))
    assert np.array_equal(_bits(uniform), _bits(ref.film())) and np.array_equal(_bits(m2_u), _bits(m2s[waves]))
    assert it.shutter_info() == 3
    film, wv, err, info = render_adaptive(it, 0.0, min_waves=2, step_waves=2, max_waves=waves)
    assert (wv == waves).all() and film.tobytes() == uniform.tobytes()
    # a target between the tiles' errors after the first round: some stop there, some go on
    e2 = A.tile_errors(wl.cfg, films[2], m2s[2], 1e-3)
    target = float(np.sort(e2)[len(e2) // 2 - 1])
    want_film, want_m2, want_wv, want_err = A.emulate_adaptive(wl.cfg, films, m2s, target, 1e-3, 2, 2, waves)
    assert want_wv.min() < want_wv.max(), "a wrong choice of target"
    film, wv, err, info, m2 = render_adaptive(it, target, min_waves=2, step_waves=2, max_waves=waves, return_moments=True)
    assert np.array_equal(wv, want_wv) and np.array_equal(_bits(err), _bits(want_err))
    for t in range(wl.cfg.jobs_per_wave()):
        m = A.tile_mask(wl.cfg, [t])
        assert np.array_equal(_bits(film[m]), _bits(ref.film(waves=int(wv[t]))[m])), f"tile {t} after {wv[t]} waves"
    assert np.array_equal(_bits(film), _bits(want_film)) and np.array_equal(_bits(m2), _bits(want_m2))
    with pytest.raises(ValueError):
        render_adaptive(it, 0.1, min_waves=2, step_waves=2, max_waves=waves, fused=True)


# ------------------------------------------------------------------------------ 7. across set_scene and set_volume

def test_shutter_survives_scene_and_volume_updates():
    w, h, waves = 20, 12, 3
    wl = _wl("c3", w, h, waves)
    cams = _cameras(wl.cfg, "three")
    it = _integrator(wl)
    it.set_shutter(cams)
    cfg2 = wl.cfg.copy()
    cfg2.volume_parameters.sigma_s = wl.cfg.volume_parameters.sigma_s * 0.5
    cfg2.volume_parameters.henyey_greenstein_g = 0.3
    it.set_scene(cfg2)
    it.set_volume(*_grids(wl))
    assert it.shutter_info() == 3
    got = {how: _render(it, how, waves) for how in ("jobs", "tiles")}
    wl2 = _wl("c3", w, h, waves)
    wl2.cfg = cfg2
    fresh = _integrator(wl2)
    fresh.set_shutter(cams)
    for how in ("jobs", "tiles"):
        assert got[how].tobytes() == _render(fresh, how, waves).tobytes(), how
    assert got["jobs"].tobytes() != _ref("c3", w, h, waves, "three").film().tobytes()  # (the medium did change)


# -------------------------------------------------------------------------------------- 8. state and validation

def _arr(cfg, cams):
    return scenes.shutter_entries(cfg, cams)


def test_validation_leaves_the_previous_shutter_in_force():
    w, h, waves = 20, 12, 3
    wl = _wl("c3", w, h, waves)
    it = _integrator(wl)
    L = capi.lib()
    cams = _cameras(wl.cfg, "three")
    it.set_shutter(cams)
    want = _render(it, "jobs", waves)
    good = _arr(wl.cfg, cams)
    assert L.vpt_gpu_set_shutter(None, good, 3) == VPT_E_INVALID
    assert L.vpt_gpu_set_shutter(it.h, None, 3) == VPT_E_INVALID
    assert L.vpt_gpu_set_shutter(it.h, good, 0) == VPT_E_INVALID
    big = (capi.ShutterCamera * 65537)()
    for e in big:
        C.memmove(C.byref(e), C.byref(good[0]), C.sizeof(capi.ShutterCamera))
    assert L.vpt_gpu_set_shutter(it.h, big, 65537) == VPT_E_INVALID
    p = [float(v) for v in wl.cfg.camera_parameters.position]
    bad = _arr(wl.cfg, [cams[0], {"look": p}, cams[2]])  # entry 1: look == position
    assert L.vpt_gpu_set_shutter(it.h, bad, 3) == VPT_E_INVALID and b"entry 1" in L.vpt_last_error()
    for field, value in (("vfov_deg", 0.0), ("vfov_deg", 180.0), ("up", [0.0, 0.0, 0.0]), ("position", [float("nan"), 0.0, 0.0])):
        assert L.vpt_gpu_set_shutter(it.h, _arr(wl.cfg, [{field: value}]), 1) == VPT_E_INVALID, field
        assert b"entry 0" in L.vpt_last_error()
    n = C.c_uint32(99)
    assert L.vpt_gpu_shutter_info(it.h, C.byref(n)) == 0 and n.value == 3
    assert _render(it, "jobs", waves).tobytes() == want.tobytes(), "a refused call changed the shutter"
    # the largest table: 65536 entries, all of them the first camera
    it.set_shutter([cams[0]])
    one = _render(it, "jobs", waves)
    assert L.vpt_gpu_set_shutter(it.h, big, 65536) == 0 and it.shutter_info() == 65536
    assert _render(it, "jobs", waves).tobytes() == one.tobytes() and one.tobytes() != want.tobytes()


def test_launches_that_cannot_honour_the_shutter_are_refused():
    w, h, waves = 20, 12, 3
    wl = _wl("c3", w, h, waves)
    it = _integrator(wl)
    T = wl.cfg.jobs_per_wave()
    L = capi.lib()
    film = torch.zeros_like(it.film)
    fptr, s = C.c_void_p(film.data_ptr()), C.c_void_p(it.stream_handle())
    # a drop-in frame is open: attaching is refused
    granted = C.c_uint64(2)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open")
    good = _arr(wl.cfg, _cameras(wl.cfg, "three"))
    assert L.vpt_gpu_set_shutter(it.h, good, 3) == VPT_E_STATE and b"frame" in L.vpt_last_error()
    granted = C.c_uint64(0)
    capi.check(L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T), "vpt_gpu_frame_open (close)")
    it.set_shutter(_cameras(wl.cfg, "three"))
    rec = torch.zeros((T * 64, 3), dtype=torch.float32, device=it.dev)
    assert L.vpt_gpu_render_jobs_records(it.h, 0, T, fptr, C.c_void_p(rec.data_ptr()), s) == VPT_E_STATE
    assert b"shutter" in L.vpt_last_error() and b"debug" in L.vpt_last_error()
    with pytest.raises(RuntimeError, match="shutter"):
        it.trace_jobs(0, 1, film=film)
    it.set_rng_mode(capi.VPT_RNG_PIXEL)
    assert L.vpt_gpu_render_jobs(it.h, 0, T, fptr, s) == VPT_E_STATE and b"pixel" in L.vpt_last_error()
    it.set_rng_mode(capi.VPT_RNG_REFERENCE)
    it.set_film_order(capi.VPT_FILM_ATOMIC)
    assert L.vpt_gpu_render_jobs(it.h, 0, T, fptr, s) == VPT_E_STATE and b"VPT_FILM_ATOMIC" in L.vpt_last_error()
    it.set_film_order(capi.VPT_FILM_ORDERED)
    granted = C.c_uint64(2)
    assert L.vpt_gpu_frame_open(it.h, 0, C.byref(granted), 0, T) == VPT_E_STATE and b"shutter" in L.vpt_last_error()
    fs, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(fs)), "stream")
    assert L.vpt_gpu_feed_open(it.h, fptr, fs, 1024, C.byref(f)) == VPT_E_STATE and b"shutter" in L.vpt_last_error()
    capi.check(L.vpt_gpu_stream_destroy(it.h, fs), "stream destroy")
    m2 = torch.zeros((h, w), dtype=torch.float32, device=it.dev)
    p, res = capi.AdaptiveParams(0.1, 1e-3, 2, 1, 3), capi.AdaptiveResult()
    wv, er = np.zeros(T, np.uint32), np.zeros(T, np.float32)
    assert L.vpt_gpu_render_adaptive_fused(it.h, C.byref(p), fptr, C.c_void_p(m2.data_ptr()),
                                           wv.ctypes.data_as(C.POINTER(C.c_uint32)), er.ctypes.data_as(C.POINTER(C.c_float)),
                                           C.byref(res), s) == VPT_E_STATE
    assert b"shutter" in L.vpt_last_error()
    alpha = torch.zeros((h, w), dtype=torch.float32, device=it.dev)
    assert L.vpt_gpu_render_alpha(it.h, 1, C.c_void_p(alpha.data_ptr()), None, s) == VPT_E_STATE
    assert b"shutter" in L.vpt_last_error()
    torch.cuda.synchronize()
    assert film.cpu().numpy().tobytes() == np.zeros((h, w, 4), np.float32).tobytes()  # nothing was rendered
    # and the context still renders the shuttered frame
    assert np.array_equal(_bits(_render(it, "jobs", waves)), _bits(_ref("c3", w, h, waves, "three").film()))


def test_set_shutter_under_an_open_feed_is_refused():
    w, h, waves = 64, 48, 16
    wl = _wl("c3", w, h, waves)
    it = _integrator(wl)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()  # (the cost pass refuses while a feed is open: done before)
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film = torch.zeros_like(it.film)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    good = _arr(wl.cfg, _cameras(wl.cfg, "three"))
    assert L.vpt_gpu_set_shutter(it.h, good, 3) == VPT_E_STATE and b"feed" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    assert it.shutter_info() == 0
    np.testing.assert_array_equal(feed_film.cpu().numpy()[..., 3], float(waves))
    it.set_shutter(_cameras(wl.cfg, "three"))  # (and once the feed is closed the call succeeds)
    assert it.shutter_info() == 3


# -------------------------------------------------------------------------------------------------------- 9. CLI

def test_cli_shutter_camera_sequence_and_pixel_mode(tmp_path):
    import json

    from volume_path_tracer_amd.__main__ import main
    from volume_path_tracer_amd.render import Integrator, render_uniform

    scene = str(scenes.SCENE_DIR / "fire.json")
    spp = 4
    common = ["--synthetic", f"fire:{N}", "--size", "16x16", "--spp", str(spp)]
    close = {"position": [30.0, 10.0, -90.0], "look": [0.0, 0.0, 0.0]}
    (tmp_path / "close.json").write_text(json.dumps(close))
    cfg = scenes.read_configuration(scene)
    cfg.num_waves, cfg.output_size[0], cfg.output_size[1] = spp, 16, 16
    grids = (SynthGrid(1, N).grid(), SynthGrid(2, N).grid())

    def api_film(c, cams):
        it = Integrator(c, *grids, device=0)
        it.set_shutter(cams)
        return render_uniform(it, moments=False).cpu().numpy()

    # one frame: the scene's camera at shutter open, the file's at shutter close, num_waves cameras between
    assert main([scene, str(tmp_path / "b.png"), *common, "--shutter-camera", str(tmp_path / "close.json"), "--film-out",
                 str(tmp_path / "b.npy")]) == 0
    cams = scenes.shutter_cameras(scenes.camera_of(cfg), scenes.camera_of(scenes.with_camera(cfg, **close)), spp)
    assert np.load(tmp_path / "b.npy").tobytes() == api_film(cfg, cams).tobytes()
    assert main([scene, str(tmp_path / "s.png"), *common, "--film-out", str(tmp_path / "s.npy")]) == 0
    assert np.load(tmp_path / "b.npy").tobytes() != np.load(tmp_path / "s.npy").tobytes()
    assert (tmp_path / "b.png").read_bytes() != (tmp_path / "s.png").read_bytes()
    # a sequence: frame k from its own camera by F towards frame k + 1's; the orbit's last frame towards index `frames`
    assert main([scene, str(tmp_path / "f_%d.png"), *common, "--frames", "2", "--orbit", "90", "--shutter", "0.5",
                 "--shutter-samples", "3", "--film-out", str(tmp_path / "f_%d.npy")]) == 0
    cfgs = scenes.orbit(cfg, 2, 90.0, closing=True)
    assert [bytes(c) for c in cfgs[:2]] == [bytes(c) for c in scenes.orbit(cfg, 2, 90.0)]
    for k in range(2):
        a, b = scenes.camera_of(cfgs[k]), scenes.camera_of(cfgs[k + 1])
        cams = scenes.shutter_cameras(a, scenes.lerp_camera(a, b, 0.5), 3)
        assert np.load(tmp_path / f"f_{k}.npy").tobytes() == api_film(cfgs[k], cams).tobytes(), f"frame {k}"
    # the rounds driver and the light groups with a shutter; the pixel RNG mode without one
    assert main([scene, str(tmp_path / "a.png"), *common, "--shutter-camera", str(tmp_path / "close.json"), "--adaptive", "0.05",
                 "--min-spp", "2", "--spp-step", "2", "--light-groups"]) == 0
    assert (tmp_path / "a.sun.png").exists()
    assert main([scene, str(tmp_path / "d.png"), *common, "--shutter-camera", str(tmp_path / "close.json"), "--denoise",
                 "--denoise-no-guides", "--film-out", str(tmp_path / "d.npy")]) == 0
    assert np.load(tmp_path / "d.npy").tobytes() == np.load(tmp_path / "b.npy").tobytes()  # (the raw film: the same frame)
    assert main([scene, str(tmp_path / "p.png"), *common, "--rng-mode", "pixel", "--film-out", str(tmp_path / "p.npy")]) == 0
    assert (np.load(tmp_path / "p.npy")[..., 3] == spp).all()
