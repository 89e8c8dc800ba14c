"""The coverage (alpha) pass on the GPU: vpt_alpha_kernel against the host build of the same march
(tests/native/alpha_host.cpp: tau byte for byte, alpha within expf's error), over the scene-parameter space, against
the film the integrate kernel renders, its side effects and state rules, and the command line's RGBA output."""
import ctypes as C

import numpy as np
import pytest

import alpha_lib as AL
import analytic_anchor as A
from test_alpha_host import cube_config
from volume_path_tracer_amd import capi, image
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, workload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6
EXPF_TOL = 2.0 ** -22  # expf within 2 ulp of a value <= 1, plus the roundings of the mean and of 1 - T


def _integrator(cfg, dens, temp=None):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(cfg, dens, temp, device=0)


def device_planes(it, sub, with_tau=True):
    """(rc, alpha, tau) through the C ABI on NaN-filled planes: a pixel the pass skipped stays NaN."""
    shape = (it.cfg.height, it.cfg.width)
    a = torch.full(shape, float("nan"), dtype=torch.float32, device=it.dev)
    t = torch.full(shape, float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    rc = capi.lib().vpt_gpu_render_alpha(it.h, sub, C.c_void_p(a.data_ptr()), C.c_void_p(t.data_ptr()) if with_tau else None,
                                         C.c_void_p(it.stream_handle()))
    torch.cuda.synchronize()
    return rc, a.cpu().numpy(), t.cpu().numpy()


def check_parity(cfg, dens, temp, sub):
    it = _integrator(cfg, dens, temp)
    rc, a, t = device_planes(it, sub)
    assert rc == capi.VPT_OK, capi.lib().vpt_last_error()
    ha, ht = AL.render(cfg, dens, sub, fill=np.nan)
    assert np.isfinite(t).all() and np.isfinite(a).all()  # every pixel of the frame was written
    assert t.tobytes() == ht.tobytes(), (np.abs(t - ht).max(), int((t != ht).sum()))
    assert np.abs(a.astype(np.float64) - ha).max() <= EXPF_TOL
    if sub == 1 or not cfg.worker_parameters.use_jitter:
        assert np.abs(a + np.expm1(-t.astype(np.float64))).max() <= EXPF_TOL
    assert (a >= 0).all() and (a <= 1).all() and not np.signbit(a).any() and not np.signbit(t).any()
    return it, a, t


def cloud_config(tile=(8, 8), jitter=True):
    """The cloud at 37x21 (ragged tiles on both axes) with camera_config's skewed camera."""
    from test_analytic_sparse import camera_config

    cfg = camera_config(jitter).cfg
    cfg.output_size[0], cfg.output_size[1] = 37, 21
    cfg.tile_size[0], cfg.tile_size[1] = tile
    return cfg


# ------------------------------------------------------------------------------------------- 1. host / device parity

def test_parity_cube():
    _, a, t = check_parity(cube_config(), SynthGrid(0, 128).grid(), None, 1)
    assert t.max() > 10 and (t == 0).sum() > 50


def test_parity_anchor_grid():
    from test_analytic_sparse import sparse_config

    _, a, t = check_parity(sparse_config(24, 24, 1).cfg, A.anchor_grid(), None, 1)
    assert a.max() > 0.3


def test_parity_cloud_ragged_jitter_sub2():
    cfg = cloud_config()
    it, a, t = check_parity(cfg, SynthGrid(1, 64).grid(), None, 2)
    assert 0.05 < a.max() and (a == 0).any()
    # the Python call: the same planes; sub=None is 4 with jitter
    pa, pt = it.render_alpha(sub=2, tau=True)
    assert pa.tobytes() == a.tobytes() and pt.tobytes() == t.tobytes()
    a4 = it.render_alpha()
    assert a4.dtype == np.float32 and a4.shape == (21, 37) and a4.tobytes() == it.render_alpha(sub=4).tobytes()
    with pytest.raises(ValueError):
        it.render_alpha(sub=9)


def test_parity_fire_with_temperature():
    wl = workload("c4", width=24, height=24, spp=1, grid_n=64)
    check_parity(wl.cfg, SynthGrid(1, 64).grid(), SynthGrid(2, 64).grid(), 1)


@pytest.mark.parametrize("tile", [(8, 8), (16, 16), (5, 3), (32, 8)])
def test_parity_tile_sizes(tile):
    """Tiles of one chunk, of four, smaller than a wavefront and ragged: the same planes whatever the tiling."""
    _, a, t = check_parity(cloud_config(tile), SynthGrid(1, 64).grid(), None, 1)
    ha, ht = AL.render(cloud_config((8, 8)), SynthGrid(1, 64).grid(), 1)
    assert t.tobytes() == ht.tobytes()


def test_single_pixel_mode_writes_one_pixel():
    cfg = cloud_config()
    wp = cfg.worker_parameters
    wp.single_pixel_enabled = 1
    wp.single_pixel_coord[0], wp.single_pixel_coord[1] = 17, 9
    dens = SynthGrid(1, 64).grid()
    rc, a, t = device_planes(_integrator(cfg, dens), 2)
    assert rc == capi.VPT_OK
    only = np.zeros((21, 37), bool)
    only[9, 17] = True
    assert np.isnan(a[~only]).all() and np.isnan(t[~only]).all()
    ha, ht = AL.render(cfg, dens, 2, fill=np.nan)
    assert t[9, 17] == ht[9, 17] and t[9, 17] > 0 and abs(float(a[9, 17]) - float(ha[9, 17])) <= EXPF_TOL
    assert np.isnan(ht[~only]).all()


# ------------------------------------------------------------------------------------------------ 2. parameter space

def _param_ids():
    import param_cases as P

    return P.IDS


@pytest.mark.parametrize("case_id", _param_ids())
def test_parameter_space(case_id):
    import param_cases as P

    wl, dens, temp = P.BY_ID[case_id].build()
    check_parity(wl.cfg, dens, temp, 2)


# -------------------------------------------------------------------------------------- 3. the film agrees with the matte

def test_film_agrees_with_the_matte():
    """check_sparse_film's bars on the production kernel's film (48x48, 256 spp) with the survival probability
    taken as 1 - alpha from vpt_alpha_kernel instead of from the float64 integral; the same exclusion rule
    (pixels whose float64 expectation moves by > 1e-3 under +-1e-3-pixel offsets) and the same 70 % cap."""
    from scipy.stats import binom

    from test_analytic_sparse import expected_survival, sparse_config

    spp = 256
    cfg = sparse_config(48, 48, spp).cfg
    it = _integrator(cfg, A.anchor_grid())
    rc, a, _ = device_planes(it, 1)
    assert rc == capi.VPT_OK
    it.render_waves(1, spp)
    film = it.film_host()
    le = np.asarray(cfg.worker_parameters.infinite_light_xyz, np.float64) * cfg.worker_parameters.infinite_light_multiplier
    r = cfg.camera_parameters.imaging_ratio
    np.testing.assert_array_equal(film[..., 3], spp)
    est = film[..., 1].astype(np.float64) / film[..., 3] / (r * le[1])
    t = 1.0 - a.astype(np.float64)
    t64, spread = expected_survival(cfg)
    miss = t64 == 1.0
    assert (a[miss] == 0).all()
    np.testing.assert_allclose(est[miss], 1.0, rtol=2e-5)
    use = (spread < 1e-3) & ~miss
    assert use.sum() >= 0.7 * use.size, use.sum()
    assert t[use].min() < 0.5 and (t[use] < 0.8).mean() > 0.5, (t[use].min(), t[use].max())
    k = np.rint(est[use] * spp)
    assert np.abs(est[use] * spp - k).max() < 0.05
    ti = t[use]
    p_two = 2 * np.minimum(binom.cdf(k, spp, ti), binom.sf(k - 1, spp, ti))
    assert p_two.min() > 1e-3 / use.sum(), (p_two.min(), int(k[p_two.argmin()]), ti[p_two.argmin()])
    z = (est[use] - ti) / np.sqrt(ti * (1 - ti) / spp)
    assert abs(z.mean()) < 4.0 / np.sqrt(z.size), (z.mean(), z.size)


# ------------------------------------------------------------------------------------------ 4. side effects and state

def test_no_side_effects_and_argument_errors():
    wl = workload("c4", width=16, height=16, spp=2, grid_n=64)
    dens, temp = SynthGrid(1, 64).grid(), SynthGrid(2, 64).grid()
    plain = _integrator(wl.cfg, dens, temp)
    plain.render_waves(1, 2)
    want = plain.film_host()
    it = _integrator(wl.cfg, dens, temp)
    it.render_waves(1, 1)
    before = it.film_host()
    a = it.render_alpha(sub=3)
    assert a.max() > 0.05
    assert it.film_host().tobytes() == before.tobytes()  # the context's own film is not touched
    it.render_waves(2, 1)
    assert it.film_host().tobytes() == want.tobytes()  # and later launches render what they would have
    L = capi.lib()
    p = torch.zeros((16, 16), dtype=torch.float32, device=it.dev)
    ptr, s = C.c_void_p(p.data_ptr()), C.c_void_p(it.stream_handle())
    for sub in (0, 9, 0xFFFFFFFF):
        assert L.vpt_gpu_render_alpha(it.h, sub, ptr, None, s) == VPT_E_INVALID and b"sub" in L.vpt_last_error()
    assert L.vpt_gpu_render_alpha(it.h, 1, None, ptr, s) == VPT_E_INVALID and b"alpha plane" in L.vpt_last_error()
    assert L.vpt_gpu_render_alpha(it.h, 8, ptr, None, s) == capi.VPT_OK  # tau plane omitted
    torch.cuda.synchronize()
    assert float(p.max()) > 0.05


def test_open_feed_refuses_the_pass():
    """While a feed of the context is launched and not closed the pass returns VPT_E_STATE and writes nothing; after
    the close it renders."""
    waves = 16
    wl = workload("c3", width=64, height=48, spp=waves, grid_n=64)
    it = _integrator(wl.cfg, SynthGrid(1, 64).grid())
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    feed_film = torch.zeros_like(it.film)
    plane = torch.full((48, 64), float("nan"), dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    s, f = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(f)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(f, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    own = C.c_void_p(it.stream_handle())
    assert L.vpt_gpu_render_alpha(it.h, 1, C.c_void_p(plane.data_ptr()), None, own) == VPT_E_STATE
    assert b"feed" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(f), "close")
    capi.check(L.vpt_gpu_feed_destroy(f), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    assert torch.isnan(plane).all()  # the refused call wrote nothing
    assert L.vpt_gpu_render_alpha(it.h, 1, C.c_void_p(plane.data_ptr()), None, own) == capi.VPT_OK
    capi.check(L.vpt_gpu_sync(it.h), "sync")  # (vpt_gpu_sync waits for the pass)
    assert not torch.isnan(plane).any()


# ----------------------------------------------------------------------------------------------------------- 5. CLI

def test_cli_alpha(tmp_path):
    from volume_path_tracer_amd.__main__ import main

    # in-process: the test runner's own GPU context (one process on the card)
    base = [str(SCENE_DIR / "fire.json"), "--synthetic", "fire:64", "--size", "48x32", "--spp", "4"]
    assert main(base[:1] + [str(tmp_path / "rgb.png")] + base[1:]) == 0
    assert main(base[:1] + [str(tmp_path / "rgba.png")] + base[1:] + ["--alpha", "--alpha-out", str(tmp_path / "a.npy")]) == 0
    data = (tmp_path / "rgba.png").read_bytes()
    assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[25] == 6
    rgba, rgb = image.decode_png(data), image.decode_png((tmp_path / "rgb.png").read_bytes())
    assert rgba.shape == (32, 48, 4) and rgb.shape == (32, 48, 3)
    assert (rgba[..., :3] == rgb).all()
    a = np.load(tmp_path / "a.npy")
    assert a.dtype == np.float32 and a.shape == (32, 48) and a.max() > 0.3 and (a == 0).any()
    assert (rgba[..., 3] == np.rint(np.float32(255.0) * a).astype(np.uint8)).all()
    # --alpha-foreground implies --alpha: the same matte, the environment light gone from the uncovered pixels
    assert main(base[:1] + [str(tmp_path / "fg.png")] + base[1:] + ["--alpha-foreground", "--alpha-sub", "4"]) == 0
    fg = image.decode_png((tmp_path / "fg.png").read_bytes())
    assert fg.shape == (32, 48, 4) and (fg[..., 3] == rgba[..., 3]).all()
    assert (fg[..., :3][a == 0] == 0).all() and (rgb[a == 0] > 0).any()
