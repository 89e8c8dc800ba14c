"""The coverage (alpha) pass, host side (no GPU): the march of csrc/vpt_alpha.h -- the code vpt_alpha_kernel runs per
lane -- compiled for the CPU (tests/native/matte_host.cpp, bound by tests/alpha_lib.py) against the float64 optical
depths of tests/analytic_anchor.py, against the integrator's own collision statistics, over the scene-parameter
space; the RGBA PNG path and foreground_film of image.py; the ABI entry vpt_gpu_render_alpha."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import alpha_lib as AL
import analytic_anchor as A
from volume_path_tracer_amd import capi, image
from volume_path_tracer_amd.scenes import SynthGrid, workload

# Tests 1 and 2: the host build's largest relative error against the float64 anchors, measured on exactly these two
# frames: 3.23e-6 on the cube (median 3.2e-7) and 2.80e-5 on the anchor grid (median 9.7e-6; its camera stands
# 50 000 voxels away, where one ulp of t is 2^-8 voxel, so every lattice cut and every tile face sits up to ~0.004
# voxel off -- the integrator's rays have the same resolution).  The bound is four times the larger one: the fp32
# summation error moves about that much between camera poses.  (Above 1e-4 the quadrature would be wrong: fp32
# Simpson with two-level sums over ~13 000 pieces has no business there.)
MEASURED_MAX_REL = 2.80e-5
RTOL = 4 * MEASURED_MAX_REL


def _sigma_t(cfg):
    v = cfg.volume_parameters
    return float(np.float32(v.sigma_a) + np.float32(v.sigma_s))


def cube_config(w=24, h=24, tile=(8, 8)):
    wl = workload("c2", width=w, height=h, spp=1)
    wl.cfg.worker_parameters.use_jitter = 0
    wl.cfg.tile_size[0], wl.cfg.tile_size[1] = tile
    return wl.cfg


def test_cube_optical_depth_matches_float64():
    """C2's constant 128^3 cube, 24x24 pixels, no jitter: tau against sigma_t * cube_od along the float64 camera
    rays, at every pixel (the field is continuous); exactly 0 where the float64 chord is empty by > 1e-3 voxels."""
    cfg = cube_config()
    alpha, tau = AL.render(cfg, SynthGrid(0, 128).grid(), 1, fill=np.nan)
    ys, xs = np.mgrid[0:24, 0:24]
    d = A.camera_dirs(cfg, xs.ravel() + 0.5, ys.ravel() + 0.5)
    o = np.broadcast_to(np.asarray(cfg.camera_parameters.position[:], np.float64) + 64.0, d.shape)  # world -> index
    ref = _sigma_t(cfg) * A.cube_od(o, d, np.full(len(d), -np.inf), np.full(len(d), np.inf))
    c0, c1 = A.cube_chord(o, d)
    got = tau.ravel().astype(np.float64)
    assert np.isfinite(got).all() and (ref > 1.0).sum() > 200
    rel = np.abs(got - ref)[ref > 0] / ref[ref > 0]
    print("cube: max rel", rel.max(), "median", np.median(rel))
    np.testing.assert_allclose(got, ref, rtol=RTOL, atol=0.0)
    empty = (c1 - c0) < -1e-3
    assert empty.sum() > 50 and (got[empty] == 0.0).all() and (alpha.ravel()[empty] == 0.0).all()
    assert not np.signbit(tau).any() and not np.signbit(alpha).any()  # a miss stores +0.0


def test_every_tree_level_matches_float64():
    """The sparse anchor grid (leaves, lower / upper / root tiles, inactive tiles) at 24x24: tau against
    sigma_t * optical_depth, pixels grazing a majorant discontinuity left out by expected_survival's rule."""
    from test_analytic_sparse import expected_survival, sparse_config

    cfg = sparse_config(24, 24, 1).cfg
    alpha, tau = AL.render(cfg, A.anchor_grid(), 1, fill=np.nan)
    t, spread = expected_survival(cfg)
    ys, xs = np.mgrid[0:24, 0:24].astype(np.float64)
    o = np.array(cfg.camera_parameters.position[:], np.float64) - np.array(A.MAP_VEC)
    ref = _sigma_t(cfg) * A.optical_depth(o, A.camera_dirs(cfg, (xs + 0.5).ravel(), (ys + 0.5).ravel()))
    miss = (t == 1.0).ravel()
    use = (spread.ravel() < 1e-3) & ~miss
    assert use.sum() >= 0.7 * use.size, use.sum()
    got = tau.ravel().astype(np.float64)
    assert np.isfinite(got).all() and (got[miss] == 0.0).all()
    rel = np.abs(got - ref)[use] / ref[use]
    print("anchor grid: max rel", rel.max(), "median", np.median(rel), "pixels", use.sum())
    np.testing.assert_allclose(got[use], ref[use], rtol=RTOL, atol=0.0)
    a64 = -np.expm1(-got)
    assert np.abs(alpha.ravel() - a64).max() <= 2.0 ** -22


def test_integrator_collisions_match_the_matte():
    """C3's cloud with its scattering parameters, 16x16 pixels, 64 waves, no jitter: a sample is a hit when the
    oracle logged a real collision for it; per pixel the hit count is Binomial(64, alpha_host)."""
    from scipy.stats import binom

    import oracle_lib as O

    spp = 64
    wl = workload("c3", width=16, height=16, spp=spp, grid_n=64)
    cfg = wl.cfg
    cfg.worker_parameters.use_jitter = 0
    dens = SynthGrid(1, 64).grid()
    alpha, _ = AL.render(cfg, dens, 1)
    T = cfg.jobs_per_wave()
    ev, _ = O.render_jobs_events(cfg, O.OracleGrid(dens, fix_majorants=True), None, 0, spp * T, capacity=1 << 22)
    real = [capi.EVENT_NAMES.index(n) for n in ("scatter_terminated", "scatter", "absorbed")]
    ev = ev[np.isin(ev["type"], real)]
    tw, th = int(cfg.tile_size[0]), int(cfg.tile_size[1])
    ntx = -(-cfg.width // tw)
    tile = (ev["jid"] % T).astype(np.int64)
    x0, y0 = (tile % ntx) * tw, (tile // ntx) * th
    rw = np.minimum(cfg.width - x0, tw)
    pix = ev["pixel"].astype(np.int64)
    px, py = x0 + pix % rw, y0 + pix // rw
    sample = np.unique(np.stack([ev["jid"].astype(np.int64), py * cfg.width + px], 1), axis=0)  # one per (jid, pixel)
    k = np.bincount(sample[:, 1], minlength=cfg.width * cfg.height).astype(np.float64)
    a = alpha.ravel().astype(np.float64)
    assert (k <= spp).all() and ((a > 0.05) & (a < 0.95)).sum() > 30
    p_two = np.minimum(1.0, 2 * np.minimum(binom.cdf(k, spp, a), binom.sf(k - 1, spp, a)))
    assert p_two.min() > 1e-3 / a.size, (p_two.min(), k[p_two.argmin()], a[p_two.argmin()])
    mid = (a > 0) & (a < 1)
    z = (k[mid] / spp - a[mid]) / np.sqrt(a[mid] * (1 - a[mid]) / spp)
    assert abs(z.mean()) < 4.0 / np.sqrt(z.size), (z.mean(), z.size)


def test_footprint():
    """With jitter and sub = 2 a pixel's alpha is the mean of 1 - exp(-tau) over the four raster points
    px + 0.5 + 0.5 * {0.25, 0.75} (2^-22: expf within 2 ulp of a value <= 1, the roundings of the sum and of the
    subtraction); without jitter all sub-rays coincide and sub = 3 is sub = 1 bit for bit."""
    wl = workload("c3", width=24, height=16, spp=1, grid_n=64)
    cfg, dens = wl.cfg, SynthGrid(1, 64).grid()
    assert cfg.worker_parameters.use_jitter
    alpha, tau = AL.render(cfg, dens, 2)
    ys, xs = np.mgrid[0:16, 0:24].astype(np.float32)
    acc, acc_tau = np.zeros((16, 24)), np.zeros((16, 24))
    for oy in (0.25, 0.75):
        for ox in (0.25, 0.75):
            t = AL.tau_at(cfg, dens, xs + np.float32(0.5 + 0.5 * ox), ys + np.float32(0.5 + 0.5 * oy)).reshape(16, 24)
            acc += -np.expm1(-t.astype(np.float64))
            acc_tau += t
    assert 0.05 < alpha.max() <= 1.0 and (alpha == 0).any()
    assert np.abs(alpha - acc / 4).max() <= 2.0 ** -22
    np.testing.assert_allclose(tau, acc_tau / 4, rtol=2.0 ** -22)
    assert AL.render(cfg, dens, 1)[0].tobytes() != alpha.tobytes()  # (the footprint matters on this frame)
    cfg.worker_parameters.use_jitter = 0
    one, three = AL.render(cfg, dens, 1), AL.render(cfg, dens, 3)
    assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes()
    centre = AL.tau_at(cfg, dens, xs + np.float32(0.5), ys + np.float32(0.5)).reshape(16, 24)
    assert centre.tobytes() == one[1].tobytes()


def _param_ids():
    import param_cases as P

    return P.IDS


@pytest.mark.parametrize("case_id", _param_ids())
def test_parameter_space(case_id):
    """Every frame of the scene-parameter space: tau finite and >= 0, alpha in [0, 1]; a camera that looks away
    from the volume sees none of it."""
    import param_cases as P

    wl, dens, _ = P.BY_ID[case_id].build()
    alpha, tau = AL.render(wl.cfg, dens, 2, fill=np.nan)
    assert np.isfinite(tau).all() and (tau >= 0).all()
    assert np.isfinite(alpha).all() and (alpha >= 0).all() and (alpha <= 1).all()
    if case_id == "away":
        assert (alpha == 0).all() and (tau == 0).all()
    elif not case_id.startswith("sigma=(1e-30"):
        assert (tau > 0).any()


def test_png_rgba_and_rgb_bytes():
    rng = np.random.default_rng(5)
    rgba = rng.integers(0, 256, (7, 5, 4), dtype=np.uint8)
    data = image.encode_png(rgba)
    assert data[25] == 6 and data[24] == 8  # IHDR: bit depth, colour type
    back = image.decode_png(data)
    assert back.dtype == np.uint8 and back.shape == (7, 5, 4) and (back == rgba).all()
    rgba16 = rng.integers(0, 65536, (3, 4, 4), dtype=np.uint16)
    assert (image.decode_png(image.encode_png(rgba16)) == rgba16).all()
    # the RGB path, byte for byte: the writer as it was before the alpha channel, restated
    import struct
    import zlib

    rgb = np.ascontiguousarray(rgba[..., :3])
    raw = np.concatenate([np.zeros((7, 1), np.uint8), rgb.reshape(7, -1)], axis=1).tobytes()
    chunk = lambda tag, d: struct.pack(">I", len(d)) + tag + d + struct.pack(">I", zlib.crc32(tag + d) & 0xFFFFFFFF)  # noqa: E731
    want = (b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", 5, 7, 8, 2, 0, 0, 0))
            + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))
    assert image.encode_png(rgb) == want
    assert (image.decode_png(want) == rgb).all()
    with pytest.raises(ValueError):
        image.encode_png(rgba[..., :2])


def test_foreground_film():
    """A synthetic film w * r * ((1 - a) * Le + a * C) gives back C to fp32 rounding; a = 0 gives zeros; w is kept."""
    cfg = workload("c3", width=8, height=6, spp=1, grid_n=64).cfg
    wp = cfg.worker_parameters
    le = np.asarray(wp.infinite_light_xyz[:], np.float64) * float(wp.infinite_light_multiplier)
    assert (le > 0).all()
    r = float(cfg.camera_parameters.imaging_ratio)
    rng = np.random.default_rng(11)
    a = rng.uniform(0.02, 1.0, (6, 8))
    a[0, :4] = 0.0
    a[1, 0] = 1.0
    a[1, 1] = 1.0 / 512.0  # below one 8-bit step: treated as uncovered
    c = rng.uniform(0.05, 3.0, (6, 8, 3))
    w = rng.integers(1, 300, (6, 8)).astype(np.float64)
    film = np.empty((6, 8, 4), np.float32)
    film[..., :3] = (w * r)[..., None] * ((1 - a)[..., None] * le + a[..., None] * c)
    film[..., 3] = w
    out = image.foreground_film(film, a.astype(np.float32), cfg)
    assert out.dtype == np.float32 and (out[..., 3] == film[..., 3]).all()
    cover = a > 1.0 / 255.0
    assert (out[~cover][:, :3] == 0).all() and (~cover).sum() == 5
    got = out[..., :3] / (w * r)[..., None]
    # roundings: film and alpha to fp32 (2^-24 each, of terms up to w r (Le + C)), three fp32 operations; the
    # subtraction's absolute error is divided by alpha
    tol = 8 * 2.0 ** -24 * (le.max() + 3.0) / a[cover]
    assert (np.abs(got - c)[cover] <= tol[:, None]).all(), (np.abs(got - c)[cover] / tol[:, None]).max()
    with pytest.raises(ValueError):
        image.foreground_film(film, a[:3].astype(np.float32), cfg)


def test_render_alpha_abi():
    lib = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT vpt_gpu_render_alpha\b", out)
    assert lib.vpt_abi_version() == 1
    header = (AL.ROOT / "include" / "vpt_gpu.h").read_text()
    assert re.search(r"#define VPT_ABI_VERSION 1\b", header) and re.search(r"VPT_E_INVALID\s*=\s*1\b", header)
    plane = np.zeros(4, np.float32)
    p = plane.ctypes.data_as(C.c_void_p)
    assert lib.vpt_gpu_render_alpha(None, 1, p, None, None) == 1
    assert b"null context" in lib.vpt_last_error()
    assert lib.vpt_gpu_render_alpha(None, 0, None, None, None) == 1
    assert lib.vpt_gpu_render_alpha.argtypes[1] is C.c_uint32


@pytest.mark.parametrize("sanitize", [False, True])
def test_alpha_host_program(tmp_path, sanitize):
    """The stand-alone program marches a fixed ray set -- axis-aligned, in a bbox face, from inside, missing, oblique,
    without a direction -- over the cloud, the cube and voxel sizes 2^-20 and 2^27, and exits 0 when every tau is
    finite and >= 0.  Once more as an AddressSanitizer + UBSan build, run directly as a plain process."""
    extra = ["-O1", "-g", "-DALPHA_HOST_MAIN"]
    if sanitize:
        extra += ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe = AL.compile_host(tmp_path / ("alpha_host_san" if sanitize else "alpha_host"), extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "alpha_host ok" in r.stdout and "FAIL" not in r.stdout
    taus = [float(v) for v in re.findall(r"ray \d+: tau (\S+)", r.stdout)]
    assert len(taus) == 44 and sum(t > 0 for t in taus) >= 20
