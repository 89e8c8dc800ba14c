"""The depth pass, host side (no GPU): the march of csrc/vpt_depth.h -- the code vpt_depth_kernel runs per lane --
compiled for the CPU (tests/native/matte_host.cpp, bound by tests/depth_lib.py) against the float64 inverse of the
analytic anchors' cumulative optical depth, against the matte's tau plane (bit-exact reach equivalence), against its own
march cut at the depth, and against the first real collisions of the reference's paths; the command line's refusals;
the ABI entry vpt_gpu_render_depth."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import alpha_lib as AL
import analytic_anchor as A
import depth_lib as DL
from volume_path_tracer_amd import capi, scenes
from volume_path_tracer_amd.scenes import SynthGrid, workload

LEVELS = (1.0 / 255.0, 0.5, 0.9)

# Test 1: the host build's largest relative error of z against the float64 inverse, measured on exactly these two
# frames (24x24, the three LEVELS): 2.17e-7 on the cube (1200 depths, median 3e-8; z ~ 250, one ulp of z is 6e-8 of z)
# and 2.86e-6 on the anchor grid (909 depths, median 5e-8), whose camera stands 50 000 voxels away: one ulp of t is 2^-8 voxel
# there, and the matte's tau is off by up to 2.8e-5 of itself (test_alpha_host), which moves a depth inside the root
# tile (density 0.01, sigma_t 0.01) by up to ~0.3 voxel of 58 000.  The bar is four times the measured error of each
# frame: 8.7e-7 and 1.14e-5.
MEASURED_CUBE = 2.17e-7
MEASURED_ANCHOR = 2.86e-6


def _sigma_t(cfg):
    v = cfg.volume_parameters
    return float(np.float32(v.sigma_a) + np.float32(v.sigma_s))


def cube_config(w=24, h=24, tile=(8, 8)):
    wl = workload("c2", width=w, height=h, spp=1)
    wl.cfg.worker_parameters.use_jitter = 0
    wl.cfg.tile_size[0], wl.cfg.tile_size[1] = tile
    return wl.cfg


def cloud_config(w=21, h=13):
    """A ragged cloud frame (21x13 in 8x8 tiles), jitter off."""
    wl = workload("c3", width=w, height=h, spp=1, grid_n=64)
    wl.cfg.worker_parameters.use_jitter = 0
    wl.cfg.tile_size[0], wl.cfg.tile_size[1] = 8, 8
    return wl.cfg


def fire_config(w=24, h=16):
    wl = workload("c4", width=w, height=h, spp=1, grid_n=64)
    wl.cfg.worker_parameters.use_jitter = 0
    return wl.cfg


def sparse_cfg(w=24, h=24, spp=1):
    from test_analytic_sparse import sparse_config

    return sparse_config(w, h, spp).cfg


def scenes_under_test():
    """(name, cfg, density grid, rho_max) of the four frames of tests 2 and 3."""
    cloud = SynthGrid(1, 64).grid()
    return [("cube", cube_config(), SynthGrid(0, 128).grid(), 1.0),
            ("anchor", sparse_cfg(), A.anchor_grid(), 0.5),
            ("cloud", cloud_config(), cloud, float(cloud.leaf_values.max())),
            ("fire", fire_config(), cloud, float(cloud.leaf_values.max()))]


_CACHE = {}


def planes(name):
    """(cfg, grid, rho_max, depth [3][H][W], reach, tau plane of the matte at sub = 1), computed once per frame."""
    if name not in _CACHE:
        for n, cfg, g, rho in scenes_under_test():
            if n == name:
                d, r = DL.render(cfg, g, LEVELS, 1, fill=np.nan)
                _, tau = AL.render(cfg, g, 1)
                _CACHE[name] = (cfg, g, rho, d, r, tau)
    return _CACHE[name]


def _invert(cum, lo, hi, target, iters=80):
    """The smallest s in [lo, hi] with cum(s) >= target, per ray (cum non-decreasing), by bisection in float64."""
    lo, hi = lo.copy(), hi.copy()
    for _ in range(iters):
        mid = 0.5 * (lo + hi)
        ok = cum(mid) >= target
        hi = np.where(ok, mid, hi)
        lo = np.where(ok, lo, mid)
    return hi


def _compare(name, cfg, depth, total, zref, measured):
    """depth[k] against zref[k] (float64 inverse; total: the float64 optical depth of the whole ray).  Where the
    float64 total is within 1e-4 of a level, fp32 and float64 may disagree on whether it is reached: the matte's
    tolerance (test_alpha_host.RTOL = 1.1e-4) decides nothing there, so those pixels are compared only if both reach."""
    tk = DL.levels(LEVELS).astype(np.float64)
    worst, n = 0.0, 0
    for k in range(len(LEVELS)):
        got = depth[k].ravel().astype(np.float64)
        clear = np.abs(total - tk[k]) > 2e-4 * tk[k]
        want_reach = total >= tk[k]
        assert ((got > 0) == want_reach)[clear].all(), (name, k)
        both = (got > 0) & want_reach
        rel = np.abs(got[both] - zref[k][both]) / zref[k][both]
        if both.any():
            worst, n = max(worst, rel.max()), n + int(both.sum())
            print(name, "level", k, "pixels", int(both.sum()), "max rel", rel.max(), "median", np.median(rel))
    print(name, "largest relative error of z", worst, "over", n, "depths; bar", 4 * measured)
    assert n > 200
    assert worst <= 4 * measured, (worst, measured)


def test_cube_depths_match_float64_inverse():
    """C2's constant 128^3 cube, 24x24 pixels, no jitter: z_k against the float64 inverse of sigma_t * cube_od along
    the float64 camera rays.  Voxel size 1: index time is world distance, so this is also the check that z is measured
    from the camera position (the cube's near face is ~236 away) with the factor ln.scale."""
    cfg, _, _, depth, reach, _ = planes("cube")
    ys, xs = np.mgrid[0:24, 0:24]
    d = A.camera_dirs(cfg, xs.ravel() + 0.5, ys.ravel() + 0.5)
    o = np.broadcast_to(np.asarray(cfg.camera_parameters.position[:], np.float64) + 64.0, d.shape)  # world -> index
    st = _sigma_t(cfg)
    c0, c1 = A.cube_chord(o, d)
    c1 = np.maximum(c1, c0)
    neg = np.full(len(d), -np.inf)
    total = st * A.cube_od(o, d, neg, np.full(len(d), np.inf))
    tk = DL.levels(LEVELS).astype(np.float64)
    zref = [_invert(lambda s: st * A.cube_od(o, d, neg, s), c0, c1, t) for t in tk]
    _compare("cube", cfg, depth, total, zref, MEASURED_CUBE)
    assert np.isfinite(depth).all() and not np.signbit(depth).any()
    assert ((reach == 0) | (reach == 1)).all() and ((reach == 1) == (depth > 0)).all()


def _anchor_inverse(o, d, targets):
    """Per ray the smallest t at which analytic_anchor's integrand -- rho * [m(floor p) > 0] along o + t d, clipped to
    the index bbox -- has accumulated targets[k]; (total [n], t [K][n]).  analytic_anchor.optical_depth_chunk's pieces
    (cubics of t times a constant indicator: 2-point Gauss-Legendre is exact on any part of one), their running sum,
    and a float64 bisection inside the piece where the sum passes the target."""
    lo = np.array(A.BBOX_MIN, np.float64)
    hi = np.array(A.BBOX_MAX, np.float64) + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (lo - o) * inv, (hi - o) * inv
    t0 = np.nanmax(np.minimum(ta, tb), axis=1)
    t1 = np.maximum(np.nanmin(np.maximum(ta, tb), axis=1), t0)
    pts = [t0[:, None], t1[:, None]]
    for ax in (0, 1):
        a, b = o[ax] + d[:, ax] * t0, o[ax] + d[:, ax] * t1
        n = np.arange(np.floor(np.minimum(a, b)).min(), np.ceil(np.maximum(a, b)).max() + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (n[None, :] - o[ax]) / d[:, ax:ax + 1]
        pts.append(np.where(np.isfinite(t), t, t0[:, None]))
    for za, zb in A.Z_WINDOWS:
        pts.append((np.arange(za, zb + 1)[None, :] - o[2]) / d[:, 2:3])
    for zb in (A.Z_UPPER_TILE, A.Z_ROOT_GAP, A.Z_ROOT_TILE, A.Z_END):
        pts.append((zb - o[2]) / d[:, 2:3])
    t = np.sort(np.clip(np.concatenate(pts, axis=1), t0[:, None], t1[:, None]), axis=1)
    a, b = t[:, :-1], t[:, 1:]
    pm = o + (0.5 * (a + b))[..., None] * d[:, None, :]
    ind = A.majorant_positive(*(np.floor(pm[..., q]).astype(np.int64) for q in range(3)))

    def part(lo_, hi_, ind_, dd):
        half, mid = 0.5 * (hi_ - lo_), 0.5 * (hi_ + lo_)
        s = np.zeros(lo_.shape)
        for x, w in zip(*A.GL2):
            s += w * half * ind_ * A.trilinear(o + (mid + half * x)[..., None] * dd)
        return s

    piece = part(a, b, ind, d[:, None, :])
    cum = np.cumsum(piece, axis=1)
    rows = np.arange(len(d))
    out = []
    for target in targets:
        j = np.minimum((cum < target).sum(axis=1), piece.shape[1] - 1)  # the first piece whose running sum reaches it
        before = np.where(j > 0, cum[rows, np.maximum(j - 1, 0)], 0.0)
        pa, pb, pi = a[rows, j], b[rows, j], ind[rows, j]
        out.append(_invert(lambda s: before + part(pa, s, pi, d), pa, pb, target))
    return cum[:, -1], out


def test_every_tree_level_depths_match_float64_inverse():
    """The sparse anchor grid (leaves, lower / upper / root tiles, inactive tiles; camera 50 000 voxels away) at 24x24:
    z_k against the float64 inverse, pixels grazing a majorant discontinuity left out by expected_survival's rule, as
    test_alpha_host.test_every_tree_level_matches_float64 leaves them out (their fp32 ray sees other tiles)."""
    from test_analytic_sparse import expected_survival

    cfg, _, _, depth, _, _ = planes("anchor")
    t, spread = expected_survival(cfg)
    use = ((spread.ravel() < 1e-3) & ~(t == 1.0).ravel())
    assert use.sum() >= 0.7 * use.size, use.sum()
    ys, xs = np.mgrid[0:24, 0:24].astype(np.float64)
    o = np.array(cfg.camera_parameters.position[:], np.float64) - np.array(A.MAP_VEC)
    d = A.camera_dirs(cfg, (xs + 0.5).ravel(), (ys + 0.5).ravel())[use]
    st = _sigma_t(cfg)
    tk = DL.levels(LEVELS).astype(np.float64)
    total, zref = _anchor_inverse(o, d, tk / st)
    assert np.allclose(total, A.optical_depth(o, d), rtol=1e-12)
    _compare("anchor grid", cfg, depth.reshape(len(LEVELS), -1)[:, use], st * total, zref, MEASURED_ANCHOR)


@pytest.mark.parametrize("name", ["cube", "anchor", "cloud", "fire"])
def test_reach_is_the_mattes_tau_plane(name):
    """depth[k] > 0 exactly where the matte's tau plane (sub = 1) is >= tau_k, bit for bit; +0.0 (sign included)
    elsewhere; depth non-decreasing in k where both levels are reached."""
    cfg, _, _, depth, reach, tau = planes(name)
    tk = DL.levels(LEVELS)
    assert tk.dtype == np.float32 and np.array_equal(tk, (-np.log1p(-np.asarray(LEVELS, np.float32).astype(np.float64))
                                                          ).astype(np.float32))
    assert np.isfinite(depth).all()
    for k in range(len(LEVELS)):
        want = tau >= tk[k]
        assert np.array_equal(depth[k] > 0, want), (name, k, int(((depth[k] > 0) != want).sum()))
        assert (depth[k][~want].view(np.uint32) == 0).all()
        assert np.array_equal(reach[k], want.astype(np.float32))
        if k:
            assert (depth[k][want] >= depth[k - 1][want]).all()
    print(name, "reached per level", [(depth[k] > 0).sum() for k in range(len(LEVELS))], "of", tau.size)
    assert (depth[0] > 0).any() and not (depth[0] > 0).all() or name == "fire"
    assert (depth[1] > 0).any()


@pytest.mark.parametrize("name", ["cube", "anchor", "cloud", "fire"])
def test_depth_is_consistent_with_the_march_cut_there(name):
    """tau(z_k), the same march cut at the world distance z_k, is >= tau_k and exceeds it by at most
    sigma_t * scale * rho_max * h / 2^steps + 4 ulp(tau_k): h = sqrt(3) index units bounds a lattice piece, the
    bisection halves it `steps` times and the field is at most rho_max on what is left (scale = 1: voxel size 1).
    That bound presumes that fp32 resolves the bisection's last interval, h / 2^16 = 2.6e-5 index units.  It about does
    on the cube, the cloud and the fire (one ulp of the ray time is at most 3.1e-5 there), where the bound is applied
    as it stands.  On the anchor grid the camera
    stands 50 000 voxels away and one ulp of the ray time -- and of z itself -- is 2^-8 voxel: the interval cannot
    shrink below one ulp and the cut's time is found from a z that rounds, so there the width is two ulps of the time
    instead (measured: up to 1.16e-5 against 3.9e-5; the bisection-count bound would be 1.3e-7)."""
    cfg, g, rho_max, depth, _, _ = planes(name)
    assert np.array_equal(np.asarray(g.desc.map_mat[:], np.float64).reshape(3, 3), np.eye(3))  # scale == 1
    tk = DL.levels(LEVELS)
    ys, xs = np.mgrid[0:cfg.height, 0:cfg.width]
    for k in range(len(LEVELS)):
        m = depth[k] > 0
        if not m.any():
            continue
        got = DL.tau_upto(cfg, g, xs[m], ys[m], depth[k][m]).astype(np.float64)
        over = got - float(tk[k])
        width = np.sqrt(3.0) / 2.0 ** DL.BISECT_STEPS
        ulp_t = float(np.spacing(depth[k][m].max()))
        if name == "anchor":
            assert ulp_t > width
            width = 2 * ulp_t
        bound = _sigma_t(cfg) * 1.0 * rho_max * width + 4 * float(np.spacing(tk[k]))
        print(name, "level", k, "tau(z) - tau_k in", over.min(), over.max(), "bound", bound)
        assert (over >= 0).all(), (name, k, over.min())
        assert (over <= bound).all(), (name, k, over.max(), bound)


def test_depth_agrees_with_the_references_first_collisions():
    """The sparse anchor scene at 16x16 and 128 waves, jitter off, a = (0.25, 0.5): the oracle's event log gives every
    sample's first real collision on the primary ray; depth_lib.check_first_collisions holds the binomial tests."""
    import oracle_lib as O

    spp, op = 128, (0.25, 0.5)
    cfg = sparse_cfg(16, 16, spp)
    g = A.anchor_grid()
    depth, _ = DL.render(cfg, g, op, 1)
    _, tau = AL.render(cfg, g, 1)
    ev, _ = O.render_jobs_events(cfg, O.OracleGrid(g, fix_majorants=True), None, 0, spp * cfg.jobs_per_wave(),
                                 capacity=1 << 22)
    pixel, dist = DL.first_real_collisions(ev, cfg)
    assert DL.check_first_collisions(cfg, op, depth, tau, pixel, dist, spp) == 2 * 256
    half = depth[1] > 0
    assert half.mean() >= 0.3 and not half.all(), half.mean()  # both branches are exercised


def test_footprint_and_levels():
    """With jitter and sub = 2 a pixel's depth is the mean over the sub-rays that reached the level and reach their
    share; without jitter sub = 3 is sub = 1 bit for bit; 1, 2 and 4 levels give the same planes for the levels they
    share, two levels 1e-6 apart included."""
    wl = workload("c3", width=24, height=16, spp=1, grid_n=64)
    cfg, dens = wl.cfg, SynthGrid(1, 64).grid()
    assert cfg.worker_parameters.use_jitter
    four = (0.25, 0.5, np.float32(0.5) + np.float32(1e-6), 0.9)
    d4, r4 = DL.render(cfg, dens, four, 2)
    assert set(np.unique(r4)) <= {0.0, 0.25, 0.5, 0.75, 1.0} and ((r4 > 0) & (r4 < 1)).any()
    assert ((r4 > 0) == (d4 > 0)).all() and (r4[1:] <= r4[:-1]).all()
    d1, r1 = DL.render(cfg, dens, four[:1], 2)
    d2, r2 = DL.render(cfg, dens, four[1:3], 2)
    assert d1.tobytes() == d4[:1].tobytes() and r1.tobytes() == r4[:1].tobytes()
    assert d2.tobytes() == d4[1:3].tobytes() and r2.tobytes() == r4[1:3].tobytes()
    both = (r4[1] == 1) & (r4[2] == 1)
    assert both.any() and (d4[2][both] >= d4[1][both]).all() and (d4[2][both] - d4[1][both]).max() < 1e-2
    cfg.worker_parameters.use_jitter = 0
    one, three = DL.render(cfg, dens, four, 1), DL.render(cfg, dens, four, 3)
    assert one[0].tobytes() == three[0].tobytes() and one[1].tobytes() == three[1].tobytes()
    # single-pixel mode writes one pixel
    cfg.worker_parameters.single_pixel_enabled = 1
    cfg.worker_parameters.single_pixel_coord[0], cfg.worker_parameters.single_pixel_coord[1] = 11, 7
    sp, _ = DL.render(cfg, dens, four, 1, fill=-1.0)
    assert sp[:, 7, 11].tobytes() == one[0][:, 7, 11].tobytes() and (sp == -1.0).sum() == sp.size - 4


def test_levels_are_checked():
    L = DL.lib()
    fp = C.POINTER(C.c_float)
    out = np.zeros(8, np.float32)
    for bad in ([], [0.0], [1.0], [-0.1], [np.nan], [0.5, 0.5], [0.6, 0.5], [0.1, 0.2, 0.3, 0.4, 0.5], [0.1, np.nan]):
        a = np.asarray(bad, np.float32)
        assert L.vptd_levels(a.size, a.ctypes.data_as(fp), out.ctypes.data_as(fp)) == 1, bad
    assert L.vptd_levels(1, None, out.ctypes.data_as(fp)) == 1


def test_render_depth_abi():
    lib = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True).stdout
    assert re.search(r"\bT vpt_gpu_render_depth\b", out)
    header = (DL.ROOT / "include" / "vpt_gpu.h").read_text()
    assert re.search(r"#define VPT_DEPTH_MAX_LEVELS 4\b", header) and "16 times" in header
    assert str(DL.BISECT_STEPS) in re.search(r"kDepthBisectSteps = (\d+)", (DL.CSRC / "vpt_depth.h").read_text()).group(1)
    plane = np.zeros(4, np.float32)
    op = np.asarray([0.5], np.float32)
    p, o = plane.ctypes.data_as(C.c_void_p), op.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.vpt_gpu_render_depth(None, 1, 1, o, p, None, None) == 1
    assert b"null context" in lib.vpt_last_error()
    assert lib.vpt_gpu_render_depth.argtypes[1] is C.c_uint32 and lib.vpt_gpu_render_depth.argtypes[2] is C.c_uint32


BASE = ["--synthetic", "cloud:64", "--size", "16x8", "--spp", "2"]
REFUSED = [("shutter", ["--shutter-camera", "CAM", "--depth-out", "z.npy"], "--depth-out"),
           ("opacity 0", ["--depth-out", "z.npy", "--depth-opacity", "0,0.5"], "--depth-opacity"),
           ("opacity 1", ["--depth-out", "z.npy", "--depth-opacity", "0.5,1"], "--depth-opacity"),
           ("opacity equal", ["--depth-out", "z.npy", "--depth-opacity", "0.5,0.5"], "--depth-opacity"),
           ("opacity descending", ["--depth-out", "z.npy", "--depth-opacity", "0.6,0.5"], "--depth-opacity"),
           ("opacity nan", ["--depth-out", "z.npy", "--depth-opacity", "nan"], "--depth-opacity"),
           ("opacity five", ["--depth-out", "z.npy", "--depth-opacity", "0.1,0.2,0.3,0.4,0.5"], "--depth-opacity"),
           ("opacity text", ["--depth-out", "z.npy", "--depth-opacity", "half"], "--depth-opacity"),
           ("opacity alone", ["--depth-opacity", "0.5"], "--depth-out"),
           ("sub alone", ["--depth-sub", "2"], "--depth-out"),
           ("reach alone", ["--depth-reach-out", "r.npy"], "--depth-out"),
           ("sequence without %d", ["--frames", "2", "--depth-out", "z.npy"], "--depth-out"),
           ("sequence reach without %d", ["--frames", "2", "--depth-out", "z_%d.npy", "--depth-reach-out", "r.npy"],
            "--depth-reach-out")]


@pytest.mark.parametrize("what,extra,named", REFUSED, ids=[r[0] for r in REFUSED])
def test_cli_refusals(tmp_path, what, extra, named):
    """Exit 1 naming the option, before a device is touched: no device is visible to the child."""
    cam = tmp_path / "close.json"
    cam.write_text(json.dumps({"position": [5.0, 0.0, -100.0], "look": [0.0, 0.0, 0.0]}))
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    extra = [str(cam) if a == "CAM" else (str(tmp_path / a) if a.endswith(".npy") else a) for a in extra]
    out = tmp_path / ("o_%d.png" if "--frames" in extra else "o.png")
    r = subprocess.run([sys.executable, "-m", "volume_path_tracer_amd", str(scenes.SCENE_DIR / "wdas_cloud.json"), str(out),
                        *BASE, *extra], capture_output=True, text=True, env=env, cwd=str(DL.ROOT))
    assert r.returncode == 1, (r.returncode, r.stderr[-2000:])
    assert named in r.stderr and "FATAL" in r.stderr, r.stderr[-2000:]
    if what == "shutter":
        assert "shutter" in r.stderr
    assert not list(tmp_path.glob("*.png")) and not list(tmp_path.glob("*.npy"))


@pytest.mark.parametrize("sanitize", [False, True])
def test_depth_host_program(tmp_path, sanitize):
    """The stand-alone program marches alpha_host's ray set -- axis-aligned, in a bbox face, from inside, missing,
    oblique, without a direction -- with four levels over the cloud, the cube and voxel sizes 2^-20 and 2^27, and exits 0
    when every depth is finite, positive and ascending.  Once more as an AddressSanitizer + UBSan build, run directly as
    a plain process."""
    extra = ["-O1", "-g", "-DDEPTH_HOST_MAIN"]
    if sanitize:
        extra += ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe = DL.compile_host(tmp_path / ("depth_host_san" if sanitize else "depth_host"), extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "depth_host ok" in r.stdout and "FAIL" not in r.stdout
    got = [int(v) for v in re.findall(r"ray \d+: reached (\d)", r.stdout)]
    assert len(got) == 44 and sum(n > 0 for n in got) >= 20 and sum(n == 4 for n in got) >= 8
