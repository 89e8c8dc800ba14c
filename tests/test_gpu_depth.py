"""The depth pass on the GPU: vpt_depth_kernel against the host build of the same march (tests/native/depth_host.cpp:
depth and reach byte for byte), over the scene-parameter and grid spaces, against vpt_gpu_render_alpha's tau plane,
against the first real collisions of the integrate kernel's own paths, its state rules and side effects, and the command
line's planes."""
import ctypes as C

import numpy as np
import pytest

import analytic_anchor as A
import depth_lib as DL
from test_depth_host import LEVELS, cube_config, sparse_cfg
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, workload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6
FOUR = (0.25, 0.5, float(np.float32(0.5) + np.float32(1e-6)), 0.9)  # two levels that land in one piece


def _integrator(cfg, dens, temp=None):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(cfg, dens, temp, device=0)


def _op(opacity):
    a = np.ascontiguousarray(opacity, np.float32)
    return a, a.ctypes.data_as(C.POINTER(C.c_float))


def device_planes(it, opacity, sub, with_reach=True):
    """(rc, depth, reach) through the C ABI on NaN-filled planes: a pixel the pass skipped stays NaN."""
    a, ap = _op(opacity)
    shape = (a.size, it.cfg.height, it.cfg.width)
    d = torch.full(shape, float("nan"), dtype=torch.float32, device=it.dev)
    r = torch.full(shape, float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    rc = capi.lib().vpt_gpu_render_depth(it.h, sub, a.size, ap, C.c_void_p(d.data_ptr()),
                                         C.c_void_p(r.data_ptr()) if with_reach else None, C.c_void_p(it.stream_handle()))
    torch.cuda.synchronize()
    return rc, d.cpu().numpy(), r.cpu().numpy()


def check_parity(cfg, dens, temp, opacity, sub):
    it = _integrator(cfg, dens, temp)
    rc, d, r = device_planes(it, opacity, sub)
    assert rc == capi.VPT_OK, capi.lib().vpt_last_error()
    hd, hr = DL.render(cfg, dens, opacity, sub, fill=np.nan)
    assert np.isfinite(d).all() and np.isfinite(r).all()  # every pixel of the frame was written
    assert d.tobytes() == hd.tobytes(), (np.abs(d - hd).max(), int((d != hd).sum()))
    assert r.tobytes() == hr.tobytes(), int((r != hr).sum())
    assert not np.signbit(d).any() and ((r > 0) == (d > 0)).all()
    return it, d, r


def cloud_config(tile=(8, 8), jitter=True):
    """The cloud at 37x21 (ragged tiles on both axes) with camera_config's skewed camera."""
    from test_analytic_sparse import camera_config

    cfg = camera_config(jitter).cfg
    cfg.output_size[0], cfg.output_size[1] = 37, 21
    cfg.tile_size[0], cfg.tile_size[1] = tile
    return cfg


# ------------------------------------------------------------------------------------------- 6. host / device parity

def test_parity_cube():
    _, d, _ = check_parity(cube_config(), SynthGrid(0, 128).grid(), None, LEVELS, 1)
    assert (d[2] > 0).sum() > 300 and (d[0] == 0).sum() > 50


def test_parity_anchor_grid():
    _, d, _ = check_parity(sparse_cfg(), A.anchor_grid(), None, LEVELS, 1)
    assert (d[1] > 0).mean() > 0.3 and (d[1] == 0).any()


def test_parity_cloud_ragged_jitter_sub2():
    cfg = cloud_config()
    it, d, r = check_parity(cfg, SynthGrid(1, 64).grid(), None, FOUR, 2)
    assert (d[0] > 0).any() and (d[0] == 0).any() and ((r > 0) & (r < 1)).any()
    # the Python call: the same planes; sub=None is 4 with jitter, as for render_alpha
    pd, pr = it.render_depth(FOUR, sub=2, reach=True)
    assert pd.tobytes() == d.tobytes() and pr.tobytes() == r.tobytes()
    d4 = it.render_depth()
    assert d4.dtype == np.float32 and d4.shape == (2, 21, 37)
    assert d4.tobytes() == it.render_depth((1.0 / 255.0, 0.5), sub=4).tobytes()
    with pytest.raises(ValueError):
        it.render_depth(sub=9)
    with pytest.raises(ValueError):
        it.render_depth((0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(RuntimeError):
        it.render_depth((0.5, 0.5))


def test_parity_fire_with_temperature():
    wl = workload("c4", width=24, height=24, spp=1, grid_n=64)
    check_parity(wl.cfg, SynthGrid(1, 64).grid(), SynthGrid(2, 64).grid(), LEVELS, 1)


@pytest.mark.parametrize("tile", [(8, 8), (16, 16), (5, 3), (32, 8)])
def test_parity_tile_sizes(tile):
    """Tiles of one chunk, of four, smaller than a wavefront and ragged: the same planes whatever the tiling."""
    _, d, _ = check_parity(cloud_config(tile), SynthGrid(1, 64).grid(), None, LEVELS[:2], 1)
    hd, _ = DL.render(cloud_config((8, 8)), SynthGrid(1, 64).grid(), LEVELS[:2], 1)
    assert d.tobytes() == hd.tobytes()


@pytest.mark.parametrize("levels", [FOUR[:1], FOUR[1:3], FOUR], ids=["1", "2 in one piece", "4"])
def test_parity_level_counts(levels):
    cfg = cloud_config(jitter=False)
    _, d, _ = check_parity(cfg, SynthGrid(1, 64).grid(), None, levels, 1)
    assert (d[0] > 0).any()
    if len(levels) == 2:  # a and a + 1e-6: the same piece for nearly every pixel, handled in turn
        both = (d[0] > 0) & (d[1] > 0)
        assert both.any() and (d[1][both] >= d[0][both]).all() and (d[1][both] - d[0][both]).max() < 1e-2


def _space_ids():
    import grid_cases as GC
    import param_cases as P

    return [f"param/{i}" for i in P.IDS] + [f"grid/{i}" for i in GC.IDS]


@pytest.mark.parametrize("case_id", _space_ids())
def test_parameter_and_grid_space(case_id):
    import grid_cases as GC
    import param_cases as P

    space, _, name = case_id.partition("/")
    wl, dens, temp = (P if space == "param" else GC).BY_ID[name].build()
    check_parity(wl.cfg, dens, temp, (1.0 / 255.0, 0.5), 2)


# ---------------------------------------------------------------------------- 7. the equivalence with the matte's tau

@pytest.mark.parametrize("name", ["cube", "anchor", "cloud", "fire"])
def test_reach_is_the_alpha_kernels_tau_plane(name):
    """depth[k] > 0 exactly where vpt_gpu_render_alpha's own tau plane at sub = 1 is >= tau_k; +0.0 elsewhere."""
    from test_depth_host import scenes_under_test

    cfg, g = next((c, g) for n, c, g, _ in scenes_under_test() if n == name)
    it = _integrator(cfg, g, SynthGrid(2, 64).grid() if name == "fire" else None)
    _, tau = it.render_alpha(sub=1, tau=True)
    rc, d, r = device_planes(it, LEVELS, 1)
    assert rc == capi.VPT_OK
    tk = DL.levels(LEVELS)
    for k in range(len(LEVELS)):
        want = tau >= tk[k]
        assert np.array_equal(d[k] > 0, want), (name, k)
        assert (d[k][~want].view(np.uint32) == 0).all() and np.array_equal(r[k], want.astype(np.float32))
        if k:
            assert (d[k][want] >= d[k - 1][want]).all()
    assert (d[1] > 0).any()


# ------------------------------------------------------------------------- 8. the integrate kernel's first collisions

def test_depth_agrees_with_the_kernels_first_collisions():
    """test_depth_host's statistical test on the device: the first real collisions come from Integrator.trace_jobs at
    16x16 and 128 waves, the depths from vpt_depth_kernel, the not-reached branch's tau from vpt_alpha_kernel."""
    spp, op, capacity = 128, (0.25, 0.5), 1 << 22
    cfg = sparse_cfg(16, 16, spp)
    it = _integrator(cfg, A.anchor_grid())
    ev = it.trace_jobs(0, spp * cfg.jobs_per_wave(), capacity=capacity, film=torch.zeros_like(it.film))
    assert 0 < len(ev) <= capacity
    pixel, dist = DL.first_real_collisions(ev, cfg)
    depth = it.render_depth(op, sub=1)
    _, tau = it.render_alpha(sub=1, tau=True)
    assert DL.check_first_collisions(cfg, op, depth, tau, pixel, dist, spp) == 2 * 256
    half = depth[1] > 0
    assert half.mean() >= 0.3 and not half.all()


# ------------------------------------------------------------------------------------------ 9. state and arguments

def test_argument_errors():
    wl = workload("c3", width=16, height=16, spp=1, grid_n=64)
    it = _integrator(wl.cfg, SynthGrid(1, 64).grid())
    L = capi.lib()
    p = torch.full((4, 16, 16), float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    ptr, s = C.c_void_p(p.data_ptr()), C.c_void_p(it.stream_handle())
    good, gp = _op([0.25, 0.5])
    assert L.vpt_gpu_render_depth(None, 1, 2, gp, ptr, None, s) == VPT_E_INVALID and b"context" in L.vpt_last_error()
    assert L.vpt_gpu_render_depth(it.h, 1, 2, None, ptr, None, s) == VPT_E_INVALID and b"opacity" in L.vpt_last_error()
    assert L.vpt_gpu_render_depth(it.h, 1, 2, gp, None, ptr, s) == VPT_E_INVALID and b"depth plane" in L.vpt_last_error()
    for sub in (0, 9, 0xFFFFFFFF):
        assert L.vpt_gpu_render_depth(it.h, sub, 2, gp, ptr, None, s) == VPT_E_INVALID and b"sub" in L.vpt_last_error()
    for n in (0, 5, 0xFFFFFFFF):
        assert L.vpt_gpu_render_depth(it.h, 1, n, gp, ptr, None, s) == VPT_E_INVALID and b"levels" in L.vpt_last_error()
    for bad in ([0.0, 0.5], [0.5, 1.0], [-0.25, 0.5], [1.5], [0.5, 0.5], [0.6, 0.5], [np.nan], [0.25, np.nan]):
        a, ap = _op(bad)
        assert L.vpt_gpu_render_depth(it.h, 1, a.size, ap, ptr, None, s) == VPT_E_INVALID, bad
    torch.cuda.synchronize()
    assert torch.isnan(p).all()  # no refused call wrote anything
    assert L.vpt_gpu_render_depth(it.h, 8, 2, gp, ptr, None, s) == capi.VPT_OK  # reach plane omitted
    capi.check(L.vpt_gpu_sync(it.h), "sync")  # (vpt_gpu_sync waits for the pass)
    assert not torch.isnan(p[:2]).any() and torch.isnan(p[2:]).all() and float(p[0].max()) > 0


def test_open_feed_refuses_the_pass():
    """While a feed of the context is launched and not closed the pass returns VPT_E_STATE and writes nothing; after
    the close it renders (test_gpu_alpha's scene and feed)."""
    waves = 16
    wl = workload("c3", width=64, height=48, spp=waves, grid_n=64)
    it = _integrator(wl.cfg, SynthGrid(1, 64).grid())
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film = torch.zeros_like(it.film)
    plane = torch.full((1, 48, 64), float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    own = C.c_void_p(it.stream_handle())
    a, ap = _op([0.5])
    assert L.vpt_gpu_render_depth(it.h, 1, 1, ap, C.c_void_p(plane.data_ptr()), None, own) == VPT_E_STATE
    assert b"feed" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    assert torch.isnan(plane).all()  # the refused call wrote nothing
    assert L.vpt_gpu_render_depth(it.h, 1, 1, ap, C.c_void_p(plane.data_ptr()), None, own) == capi.VPT_OK
    capi.check(L.vpt_gpu_sync(it.h), "sync")
    assert not torch.isnan(plane).any()


def test_shutter_refuses_the_pass():
    import shutter_lib as SH

    wl = workload("c3", width=16, height=16, spp=2, grid_n=64)
    it = _integrator(wl.cfg, SynthGrid(1, 64).grid())
    before = it.render_depth((0.25, 0.5), sub=1)
    it.set_shutter(SH.three_cameras(wl.cfg))
    L = capi.lib()
    plane = torch.full((2, 16, 16), float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    a, ap = _op([0.25, 0.5])
    assert L.vpt_gpu_render_depth(it.h, 1, 2, ap, C.c_void_p(plane.data_ptr()), None,
                                  C.c_void_p(it.stream_handle())) == VPT_E_STATE
    assert b"shutter" in L.vpt_last_error()
    torch.cuda.synchronize()
    assert torch.isnan(plane).all()
    with pytest.raises(RuntimeError):
        it.render_depth((0.25, 0.5), sub=1)
    it.set_shutter(None)
    assert it.render_depth((0.25, 0.5), sub=1).tobytes() == before.tobytes() and (before > 0).any()


def test_single_pixel_mode_writes_one_pixel():
    cfg = cloud_config()
    wp = cfg.worker_parameters
    wp.single_pixel_enabled = 1
    wp.single_pixel_coord[0], wp.single_pixel_coord[1] = 17, 9
    dens = SynthGrid(1, 64).grid()
    rc, d, r = device_planes(_integrator(cfg, dens), (0.05, 0.25), 2)
    assert rc == capi.VPT_OK
    only = np.zeros((2, 21, 37), bool)
    only[:, 9, 17] = True
    assert np.isnan(d[~only]).all() and np.isnan(r[~only]).all()
    hd, hr = DL.render(cfg, dens, (0.05, 0.25), 2, fill=np.nan)
    assert d[only].tobytes() == hd[only].tobytes() and r[only].tobytes() == hr[only].tobytes() and d[0, 9, 17] > 0
    assert np.isnan(hd[~only]).all()


def test_no_side_effects():
    """A film rendered before the pass and one rendered after it are the same bytes; render_alpha's planes before and
    after are the same bytes; the pass after set_scene equals a fresh context's."""
    from volume_path_tracer_amd.scenes import orbit

    wl = workload("c4", width=16, height=16, spp=2, grid_n=64)
    dens, temp = SynthGrid(1, 64).grid(), SynthGrid(2, 64).grid()
    plain = _integrator(wl.cfg, dens, temp)
    plain.render_waves(1, 2)
    want = plain.film_host()
    it = _integrator(wl.cfg, dens, temp)
    it.render_waves(1, 1)
    before = it.film_host()
    a0, t0 = it.render_alpha(sub=2, tau=True)
    d, r = it.render_depth(sub=3, reach=True)
    assert (d > 0).any() and r.max() == 1.0
    assert it.film_host().tobytes() == before.tobytes()  # the context's own film is not touched
    a1, t1 = it.render_alpha(sub=2, tau=True)
    assert a0.tobytes() == a1.tobytes() and t0.tobytes() == t1.tobytes()
    it.render_waves(2, 1)
    assert it.film_host().tobytes() == want.tobytes()  # and later launches render what they would have
    moved = orbit(wl.cfg, 2, 90.0)[1]
    it.set_scene(moved)
    after = it.render_depth(sub=3)
    assert after.tobytes() == _integrator(moved, dens, temp).render_depth(sub=3).tobytes()
    assert after.tobytes() != d.tobytes()


# ---------------------------------------------------------------------------------------------------------- 10. CLI

def test_cli_depth(tmp_path):
    from volume_path_tracer_amd.__main__ import main
    from volume_path_tracer_amd.scenes import read_configuration

    # in-process: the test runner's own GPU context (one process on the card)
    args = [str(SCENE_DIR / "fire.json"), str(tmp_path / "o.png"), "--synthetic", "fire:64", "--size", "16x16", "--spp", "2",
            "--depth-out", str(tmp_path / "z.npy"), "--depth-reach-out", str(tmp_path / "r.npy"), "--depth-sub", "2",
            "--depth-opacity", "0.1,0.5,0.9"]
    assert main(args) == 0
    z, r = np.load(tmp_path / "z.npy"), np.load(tmp_path / "r.npy")
    assert z.dtype == np.float32 and z.shape == (3, 16, 16) and r.dtype == np.float32 and r.shape == (3, 16, 16)
    cfg = read_configuration(SCENE_DIR / "fire.json")
    cfg.output_size[0], cfg.output_size[1] = 16, 16
    cfg.num_waves = 2
    it = _integrator(cfg, SynthGrid(1, 64).grid(), SynthGrid(2, 64).grid())
    d, rr = it.render_depth((0.1, 0.5, 0.9), sub=2, reach=True)
    assert z.tobytes() == d.tobytes() and r.tobytes() == rr.tobytes() and (z > 0).any() and (z == 0).any()
    # the defaults: 1/255 (as 0.00392157) and 0.5, one sub-ray
    assert main(args[:8] + ["--depth-out", str(tmp_path / "z2.npy")]) == 0
    z2 = np.load(tmp_path / "z2.npy")
    assert z2.shape == (2, 16, 16) and z2.tobytes() == it.render_depth((np.float32(0.00392157), 0.5), sub=1).tobytes()
