"""Oracle-independent expectations for the analytic anchors (tests/test_analytic_sparse.py).

Nothing here calls the oracle or the product library's transport: the camera rays follow
Camera::Camera / generate_ray (src/camera.cpp:45-57, include/vpt/camera.hpp:14-23) in float64, the RNG
is pcg32_fast + MurmurHash64A in Python integers (pinned by the SURVEY §8c KATs, checked below), and
the expected transmittance is an exact float64 integral of NanoVDB's trilinear field over a grid
description written out here.

The sparse anchor grid (index space, world = index + (-64, -64, 0), voxel size 1) puts every NanoVDB
level on one chord along +z:

  z in [0, 128)        lower node L0 (x, y in [0, 128)): 8^3 cells with c = z/8 < 8 are leaves
                       (smooth values in [0.1, 0.4], voxel (0,0,0) = 0.5); 8 <= c < 15 lower-node
                       tiles in a checkerboard, active 0.5 / INACTIVE 0.25 (getValue returns 0.25,
                       the majorant is 0: volume.cpp:28-35); c = 15 active tiles 0.5
  z in [128, 3968)     empty slots of upper node U0 (HDDA dim 128, background 0)
  z in [3968, 4096)    an active upper-node tile 0.3 (x, y in [0, 128))
  z in [4096, 8192)    empty root space (HDDA dim 4096)
  z in [8192, 12288)   an active root tile 0.01 (x, y in [0, 4096))

indexBBox = [0, 4095]^2 x [0, 12287] (it covers the active root tile).

Delta tracking with a piecewise-constant majorant m and sigma_s = 0 absorbs at rate
sigma_a * min(m, rho) (p_a = rho / m, clamped events when rho > m, worker.cpp:148-163, and segments with
m <= 0 skipped without a draw, majorant_transmittance_sampler.cpp:24-36).  The values are chosen so
that rho <= m wherever m > 0 -- tiles hold at least their neighbours' values, leaf majorants are
fixed over the one-voxel shell (volume.cpp:104-160), and the HDDA's lookahead transitions
(volume.cpp:63: the first dim-128 / dim-4096 step after a lower / upper node takes the majorant of the
node block's corner, here always L0's leaf at (0,0,0), whose majorant 0.5 bounds every ramp it
covers) -- so the expectation is exp(-sigma_a * integral of rho * [m(floor p) > 0]) with m the
majorant of the voxel's node (leaf: its fixed max; tile: its value if active, else 0).
"""
from __future__ import annotations

import numpy as np

# ---- RNG: hash(seed, jid) + pcg32_fast + uniform<float> (hash.hpp:20-67, random.hpp:86-115) --------
M64 = (1 << 64) - 1


def murmur_seed(seed: int, jid: int) -> int:
    m = 0xC6A4A7935BD1E995
    h = (seed ^ (8 * m)) & M64
    k = (jid * m) & M64
    k ^= k >> 47
    k = (k * m) & M64
    h ^= k
    h = (h * m) & M64
    h ^= h >> 47
    h = (h * m) & M64
    h ^= h >> 47
    return h


class Pcg32Fast:
    def __init__(self, seed64: int):
        self.state = (seed64 | 3) & M64

    def u32(self) -> int:
        old = self.state
        self.state = (old * 6364136223846793005) & M64
        r = old >> 61
        old ^= old >> 22
        return (old >> (22 + r)) & 0xFFFFFFFF

    def uniform(self) -> np.float32:
        v = np.float32(np.float32(self.u32()) * np.float32(2.0 ** -32))
        return min(v, np.float32(np.nextafter(np.float32(1), np.float32(0))))


# ---- Camera (camera.cpp:45-57, camera.hpp:14-23), float64 -----------------------------------------
def camera_dirs(cfg, px, py):
    """World ray directions for raster points (px, py) (pixel + 0.5 + jitter): M = c2w.linear * s2c *
    r2s applied to (px, py, 0) and normalised, all in float64."""
    cp = cfg.camera_parameters
    pos = np.array(cp.position[:], np.float64)
    look = np.array(cp.look[:], np.float64)
    up = np.array(cp.up[:], np.float64)
    W, H = float(cfg.width), float(cfg.height)
    fwd = (look - pos) / np.linalg.norm(look - pos)
    left = np.cross(up / np.linalg.norm(up), fwd)
    new_up = np.cross(fwd, left)
    t = np.tan(np.pi * float(cp.vfov_deg) / 180.0 / 2.0)
    ar = W / H
    sx = ar * t * (1.0 - 2.0 * np.asarray(px, np.float64) / W)  # screen x (r2s then s2c)
    sy = t * (1.0 - 2.0 * np.asarray(py, np.float64) / H)
    d = sx[..., None] * left + sy[..., None] * new_up + fwd
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---- the sparse anchor grid ------------------------------------------------------------------------
Z_UPPER_TILE, Z_ROOT_GAP, Z_ROOT_TILE, Z_END = 3968, 4096, 8192, 12288
V_ACTIVE_LOWER, V_INACTIVE_LOWER, V_UPPER, V_ROOT = 0.5, 0.25, 0.3, 0.01
BBOX_MIN, BBOX_MAX = (0, 0, 0), (4095, 4095, Z_END - 1)
MAP_VEC = (-64.0, -64.0, 0.0)


def leaf_voxel_value(i, j, k):
    """Leaf voxels of L0 (z < 64): float32 values in [0.1, 0.4]; voxel (0,0,0) = 0.5."""
    i, j, k = (np.asarray(a, np.float64) for a in (i, j, k))
    v = 0.25 + 0.15 * np.sin(0.21 * i + 0.5) * np.sin(0.17 * j + 1.1) * np.sin(0.13 * k + 0.2)
    v = np.where((i == 0) & (j == 0) & (k == 0), 0.5, v)
    return v.astype(np.float32)


def _lower_tile_active(a, b, c):
    return (c == 15) | (((a + b + c) & 1) == 0)


def voxel_value(i, j, k):
    """ReadAccessor::getValue over the anchor grid (float64 of the stored float32 values)."""
    i, j, k = (np.asarray(a, np.int64) for a in (i, j, k))
    out = np.zeros(np.broadcast(i, j, k).shape, np.float64)
    col = (i >= 0) & (i < 128) & (j >= 0) & (j < 128)
    l0 = col & (k >= 0) & (k < 128)
    c = k >> 3
    leaf = l0 & (c < 8)
    tile = l0 & (c >= 8)
    out = np.where(leaf, leaf_voxel_value(i, j, k).astype(np.float64), out)
    act = _lower_tile_active(i >> 3, j >> 3, c)
    out = np.where(tile & act, np.float64(np.float32(V_ACTIVE_LOWER)), out)
    out = np.where(tile & ~act, np.float64(np.float32(V_INACTIVE_LOWER)), out)
    out = np.where(col & (k >= Z_UPPER_TILE) & (k < Z_ROOT_GAP), np.float64(np.float32(V_UPPER)), out)
    root = (i >= 0) & (i < 4096) & (j >= 0) & (j < 4096) & (k >= Z_ROOT_TILE) & (k < Z_END)
    out = np.where(root, np.float64(np.float32(V_ROOT)), out)
    return out


def majorant_positive(i, j, k):
    """m(voxel) > 0: leaves (fixed majorant >= 0.1), active tiles; not inactive tiles or background."""
    i, j, k = (np.asarray(a, np.int64) for a in (i, j, k))
    col = (i >= 0) & (i < 128) & (j >= 0) & (j < 128)
    c = k >> 3
    l0 = col & (k >= 0) & (k < 128)
    pos = l0 & ((c < 8) | _lower_tile_active(i >> 3, j >> 3, c))
    pos |= col & (k >= Z_UPPER_TILE) & (k < Z_ROOT_GAP)
    pos |= (i >= 0) & (i < 4096) & (j >= 0) & (j < 4096) & (k >= Z_ROOT_TILE) & (k < Z_END)
    return pos


def anchor_grid():
    """The anchor grid as a capi.Grid (leaves, level-1/2/3 tiles, explicit bbox)."""
    from volume_path_tracer_amd import capi

    origins, values = [], []
    ii, jj, kk = np.meshgrid(np.arange(8), np.arange(8), np.arange(8), indexing="ij")
    for a in range(16):
        for b in range(16):
            for c in range(8):
                o = (8 * a, 8 * b, 8 * c)
                origins.append(o)
                values.append(leaf_voxel_value(o[0] + ii, o[1] + jj, o[2] + kk).reshape(512))  # n = x<<6|y<<3|z
    values = np.array(values, np.float32)
    t_origin, t_level, t_value, t_active = [], [], [], []
    for a in range(16):
        for b in range(16):
            for c in range(8, 16):
                act = bool(_lower_tile_active(a, b, c))
                t_origin.append((8 * a, 8 * b, 8 * c))
                t_level.append(1)
                t_value.append(V_ACTIVE_LOWER if act else V_INACTIVE_LOWER)
                t_active.append(1 if act else 0)
    t_origin += [(0, 0, Z_UPPER_TILE), (0, 0, Z_ROOT_TILE)]
    t_level += [2, 3]
    t_value += [V_UPPER, V_ROOT]
    t_active += [1, 1]
    return capi.Grid(map_mat=np.eye(3), map_inv_mat=np.eye(3), map_vec=MAP_VEC, background=0.0,
                     bbox_min=BBOX_MIN, bbox_max=BBOX_MAX, leaf_origin=origins, leaf_values=values,
                     leaf_max=values.max(axis=1), tile_origin=t_origin, tile_level=t_level, tile_value=t_value,
                     tile_active=t_active)


Z_WINDOWS = ((0, 129), (Z_UPPER_TILE - 1, Z_UPPER_TILE + 1), (Z_ROOT_GAP - 1, Z_ROOT_GAP + 1),
             (Z_ROOT_TILE - 1, Z_ROOT_TILE + 1), (Z_END - 1, Z_END))
GL2 = (np.array([-1.0, 1.0]) / np.sqrt(3.0), np.array([1.0, 1.0]))


def trilinear(p):
    """NanoVDB SampleFromVoxels<.,1> of the anchor grid at index points p [..., 3] (float64)."""
    f = np.floor(p)
    u = p - f
    i, j, k = (f[..., q].astype(np.int64) for q in range(3))
    out = np.zeros(p.shape[:-1])
    for a in (0, 1):
        wa = u[..., 0] if a else 1.0 - u[..., 0]
        for b in (0, 1):
            wb = u[..., 1] if b else 1.0 - u[..., 1]
            for c in (0, 1):
                wc = u[..., 2] if c else 1.0 - u[..., 2]
                out += wa * wb * wc * voxel_value(i + a, j + b, k + c)
    return out


def optical_depth(o, d, chunk=256):
    """optical_depth_chunk over chunks of rays (neighbouring pixels share their x / y crossings)."""
    return np.concatenate([optical_depth_chunk(o, d[s:s + chunk]) for s in range(0, d.shape[0], chunk)])


def optical_depth_chunk(o, d):
    """Integral of rho * [m(floor p) > 0] along index rays o + t d (|d| = 1, voxel size 1, d_z > 0)
    clipped to the index bbox [min, max + 1] (Ray::clip, volume.cpp:83).  o: [3], d: [n, 3].
    Exact: between integer crossings of x, y and (inside Z_WINDOWS) z the integrand is a cubic of t
    times a constant indicator (outside the windows the voxel values do not depend on z), so
    2-point Gauss-Legendre per piece is exact."""
    lo = np.array(BBOX_MIN, np.float64)
    hi = np.array(BBOX_MAX, np.float64) + 1.0
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (lo - o) * inv, (hi - o) * inv
    t0 = np.nanmax(np.minimum(ta, tb), axis=1)
    t1 = np.nanmin(np.maximum(ta, tb), axis=1)
    assert (d[:, 2] > 0).all()
    t1 = np.maximum(t1, t0)  # a ray that misses the bbox: an empty chord
    pts = [t0[:, None], t1[:, None]]
    for ax in (0, 1):
        a, b = o[ax] + d[:, ax] * t0, o[ax] + d[:, ax] * t1
        lo_i, hi_i = np.floor(np.minimum(a, b)).min(), np.ceil(np.maximum(a, b)).max()
        n = np.arange(lo_i, hi_i + 1)
        with np.errstate(divide="ignore", invalid="ignore"):
            t = (n[None, :] - o[ax]) / d[:, ax:ax + 1]
        pts.append(np.where(np.isfinite(t), t, t0[:, None]))
    for za, zb in Z_WINDOWS:
        pts.append((np.arange(za, zb + 1)[None, :] - o[2]) / d[:, 2:3])
    for zb in (Z_UPPER_TILE, Z_ROOT_GAP, Z_ROOT_TILE, Z_END):
        pts.append((zb - o[2]) / d[:, 2:3])
    t = np.sort(np.clip(np.concatenate(pts, axis=1), t0[:, None], t1[:, None]), axis=1)
    a, b = t[:, :-1], t[:, 1:]
    half, mid = 0.5 * (b - a), 0.5 * (a + b)
    pm = o + mid[..., None] * d[:, None, :]
    ind = majorant_positive(*(np.floor(pm[..., q]).astype(np.int64) for q in range(3)))
    tau = np.zeros(d.shape[0])
    for x, w in zip(*GL2):
        p = o + (mid + half * x)[..., None] * d[:, None, :]
        tau += (w * half * ind * trilinear(p)).sum(axis=1)
    return tau


# ---- the constant cube and the single-scatter expectation ----------------------------
# Density 1 on index voxels [0, 127]^3, background 0, world = index - 64, voxel size 1.  NanoVDB's
# trilinear field inside the clip box [0, 128]^3 (CoordBBox max + 1, volume.cpp:83) is
# prod_axes clip(128 - p, 0, 1): 1 up to 127, the half-voxel ramp to 0 at the max + 1 face.
CUBE_HI = 128.0
GL3 = (np.array([-np.sqrt(0.6), 0.0, np.sqrt(0.6)]), np.array([5.0, 8.0, 5.0]) / 9.0)


def cube_density(p):
    return np.clip(CUBE_HI - p, 0.0, 1.0).prod(axis=-1)


def cube_chord(o, d):
    """Ray::clip against [0, 128]^3 (slab test): (t_enter, t_exit) per row; t_exit < t_enter = miss."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / d
        ta, tb = (0.0 - o) * inv, (CUBE_HI - o) * inv
        t0 = np.nanmax(np.minimum(ta, tb), axis=-1)
        t1 = np.nanmin(np.maximum(ta, tb), axis=-1)
    return t0, t1


def cube_od(o, d, ta, tb):
    """Integral of the cube's density along o + t d for t in [ta, tb] (clipped to the box), exact: the
    integrand is a polynomial of degree <= 3 between the ramp entries (an axis crossing 127), so
    3-point Gauss-Legendre per piece is exact.  o, d: [n, 3] (or broadcastable); ta, tb: [n]."""
    o, d = np.broadcast_arrays(np.asarray(o, np.float64), np.asarray(d, np.float64))
    c0, c1 = cube_chord(o, d)
    a = np.maximum(ta, c0)
    b = np.maximum(np.minimum(tb, c1), a)
    with np.errstate(divide="ignore", invalid="ignore"):
        br = (CUBE_HI - 1.0 - o) / d
    br = np.where(np.isfinite(br), br, a[:, None])
    pts = np.sort(np.concatenate([a[:, None], np.clip(br, a[:, None], b[:, None]), b[:, None]], axis=1), axis=1)
    tau = np.zeros(o.shape[0])
    for k in range(pts.shape[1] - 1):
        lo, hi = pts[:, k], pts[:, k + 1]
        half, mid = 0.5 * (hi - lo), 0.5 * (hi + lo)
        for x, w in zip(*GL3):
            tau += w * half * cube_density(o + (mid + half * x)[:, None] * d)
    return tau


HG_ISOTROPIC_BELOW = 1e-3   # sample_henyey_greenstein's isotropic branch: |g| < 1e-3 (random.hpp:62)


def hg_reference(cos_wwi, g):
    """henyey_greenstein(w.dot(wi), g) as the reference evaluates it in NEE: den = 1 + g^2 + 2 g c with
    the FORWARD ray direction w (utils.hpp:61-66, worker.cpp:88) -- pbrt's phase with the sign mirrored."""
    den = 1.0 + g * g + 2.0 * g * cos_wwi
    return (1.0 - g * g) / (4.0 * np.pi * den * np.sqrt(den))


def hg_cos_cdf(mu, g):
    """CDF of cos(theta) between the incoming direction w and the sampled one under
    sample_henyey_greenstein (random.hpp:56-84): local z = w and cos = (1 + g^2 - ((1 - g^2) /
    (1 + g - 2 g u))^2) / (2 g), i.e. p(mu) = (1 - g^2) / (2 (1 + g^2 - 2 g mu)^1.5), mean g: forward-peaked
    for g > 0, backward-peaked for g < 0 (the same formula: sqrt((1 + g)^2) = 1 + g for g > -1).  For
    |g| < 1e-3 the reference samples isotropically, cos = 1 - 2 u (random.hpp:62-63): the CDF is linear."""
    mu = np.asarray(mu, np.float64)
    if abs(g) < HG_ISOTROPIC_BELOW:
        return 0.5 * (mu + 1.0)
    return (1.0 - g * g) / (2.0 * g) * (1.0 / np.sqrt(1.0 + g * g - 2.0 * g * mu) - 1.0 / (1.0 + g))


def hg_sample_cos(g, u):
    """cos(theta) of sample_henyey_greenstein for the uniform number u (random.hpp:60-68), float64."""
    u = np.asarray(u, np.float64)
    if abs(g) < HG_ISOTROPIC_BELOW:
        return 1.0 - 2.0 * u
    return (1.0 + g * g - ((1.0 - g * g) / (1.0 + g - 2.0 * g * u)) ** 2) / (2.0 * g)


def single_scatter(o, w, wi, sigma_s, sub=48, npts=8, t_shadow0=1e-5):
    """For camera rays o + t w (index space, |w| = 1) through the cube with sigma_a = 0:
    (I, tau) with tau the chord's optical depth / sigma_s and

        I = integral over the chord of sigma_s rho(t) exp(-sigma_s tau(t0, t)) exp(-sigma_s tau_sh(x(t))) dt,

    the probability-weighted shadow transmittance of the first real collision (delta tracking's
    first-scatter density, the shadow ray's expected ratio-tracking-with-RR weight, worker.cpp:52-90).
    tau_sh(x) is the optical depth from x along wi (from t = 1e-5, volume.cpp:79-80) to the box exit.
    The chord is split at the ramp entries and each piece into `sub` intervals of `npts`-point
    Gauss-Legendre (the integrand is smooth there up to the kinks of tau_sh, which are second order)."""
    o = np.asarray(o, np.float64)
    w = np.asarray(w, np.float64)
    n = w.shape[0]
    t0, t1 = cube_chord(np.broadcast_to(o, w.shape), w)
    t0 = np.maximum(t0, 0.0)
    hit = t1 > t0
    t1 = np.where(hit, t1, t0)
    with np.errstate(divide="ignore", invalid="ignore"):
        br = (CUBE_HI - 1.0 - o) / w
    br = np.where(np.isfinite(br), br, t0[:, None])
    edges = np.sort(np.concatenate([t0[:, None], np.clip(br, t0[:, None], t1[:, None]), t1[:, None]], axis=1), axis=1)
    gx, gw = np.polynomial.legendre.leggauss(npts)
    # nodes: [n, pieces, sub, npts]
    lo, hi = edges[:, :-1], edges[:, 1:]
    s = np.arange(sub)
    a = lo[..., None] + (hi - lo)[..., None] * s / sub
    h = ((hi - lo) / sub)[..., None]
    t = (a + 0.5 * h)[..., None] + (0.5 * h)[..., None] * gx
    wt = np.broadcast_to((0.5 * h)[..., None] * gw, t.shape)
    t, wt = t.reshape(n, -1), wt.reshape(n, -1)
    m = t.shape[1]
    x = o + t[..., None] * w[:, None, :]                                   # [n, m, 3]
    rho = cube_density(x)
    tau_cam = cube_od(np.broadcast_to(o, (n * m, 3)), np.repeat(w, m, axis=0), np.repeat(t0, m),
                      t.reshape(-1)).reshape(n, m)
    wi = np.asarray(wi, np.float64)
    tau_sh = cube_od(x.reshape(-1, 3), np.broadcast_to(wi, (n * m, 3)), np.full(n * m, t_shadow0),
                     np.full(n * m, np.inf)).reshape(n, m)
    I = (wt * sigma_s * rho * np.exp(-sigma_s * (tau_cam + tau_sh))).sum(axis=1)
    tau = cube_od(np.broadcast_to(o, (n, 3)), w, t0, t1)
    return np.where(hit, I, 0.0), np.where(hit, tau, 0.0)


# ---- multiple scattering: the survival probability of absorbing paths ----------------
def max_scatters(max_depth):
    """Scatters a path can make: the loop's depth moves twice per scatter (worker.cpp:130 and :169) and its
    body runs while depth < max_depth, so at depths 0, 2, 4, ... -- ceil(max_depth / 2) iterations; the
    scatter check `depth++ >= max_depth` (:169) never fires, since depth < max_depth in the body.  After the
    last one's scatter the loop ends with `terminated` false, and the environment light is added."""
    return (int(max_depth) + 1) // 2


def hg_sample_dirs(d, g, u1, u2):
    """sample_henyey_greenstein (random.hpp:56-84) about the incoming directions d [n, 3]: local z = d,
    cos = (1 + g^2 - ((1 - g^2) / (1 + g - 2 g u1))^2) / (2 g) (1 - 2 u1 for |g| < 1e-3: hg_sample_cos),
    phi = 2 pi u2 (any frame about d: the law is symmetric in phi)."""
    cos = np.clip(hg_sample_cos(g, u1), -1.0, 1.0)
    sin = np.sqrt(np.maximum(0.0, 1.0 - cos * cos))
    a = np.where(np.abs(d[:, :1]) < 0.9, [[1.0, 0.0, 0.0]], [[0.0, 1.0, 0.0]])
    e1 = np.cross(d, a)
    e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(d, e1)
    phi = 2.0 * np.pi * u2
    return (sin * np.cos(phi))[:, None] * e1 + (sin * np.sin(phi))[:, None] * e2 + cos[:, None] * d


def survival_walk(o, w, sigma_s, sigma_a, g, max_depth, rng):
    """Whether each camera path o + t w (index space, |w| = 1) through the cube survives -- is not absorbed
    -- by an analog random walk in float64 written from the reference's semantics, not from the oracle:
    delta tracking against the majorant sigma_t (the cube's density <= 1) inside the clip box [0, 128]^3
    (Ray::clip, volume.cpp:83), a tentative collision real with probability rho(x) (null: same direction,
    majorant_transmittance_sampler.cpp:59-61), a real one absorbing with probability sigma_a / sigma_t and
    otherwise scattering along sample_henyey_greenstein's law (worker.cpp:148-179), the path ending without
    absorption when it leaves the box or after max_scatters(max_depth) scatters.  Returns bool [n]."""
    n = w.shape[0]
    sigma_t = sigma_s + sigma_a
    t0, t1 = cube_chord(np.broadcast_to(o, w.shape), w)
    t0 = np.maximum(t0, 1e-5)
    surv = np.ones(n, bool)
    act = t1 > t0
    p = np.where(act[:, None], o + t0[:, None] * w, 0.0)
    d = w.copy()
    k = np.zeros(n, np.int64)
    kmax = max_scatters(max_depth)
    idx = np.flatnonzero(act)
    while idx.size:
        pi, di = p[idx], d[idx]
        _, te = cube_chord(pi, di)                                 # the box exit from the current point
        dt = -np.log1p(-rng.random(idx.size)) / sigma_t
        esc = dt >= te
        pn = pi + dt[:, None] * di
        real = ~esc & (rng.random(idx.size) < cube_density(pn))
        absorb = real & (rng.random(idx.size) < sigma_a / sigma_t)
        scat = real & ~absorb
        surv[idx[absorb]] = False
        k[idx[scat]] += 1
        p[idx] = np.where(esc[:, None], pi, pn)
        if scat.any():
            s = idx[scat]
            d[s] = hg_sample_dirs(d[s], g, rng.random(s.size), rng.random(s.size))
        done = esc | absorb | (scat & (k[idx] >= kmax))
        idx = idx[~done]
    return surv


def survival_probability(cfg, paths_per_pixel, seed=0, index_of_world=64.0, chunk=1 << 20):
    """Per pixel [H, W]: the survival probability of its camera paths (pixel centres: no jitter) estimated
    with paths_per_pixel walks of survival_walk (in chunks of ~`chunk` paths)."""
    W, H = cfg.width, cfg.height
    v, wp = cfg.volume_parameters, cfg.worker_parameters
    ys, xs = np.mgrid[0:H, 0:W]
    d = camera_dirs(cfg, xs.ravel() + 0.5, ys.ravel() + 0.5)
    o = np.asarray(cfg.camera_parameters.position[:], np.float64) + index_of_world
    rng = np.random.default_rng(seed)
    hits = np.zeros(W * H)
    reps = max(1, chunk // (W * H))
    done = 0
    while done < paths_per_pixel:
        r = min(reps, paths_per_pixel - done)
        surv = survival_walk(o, np.tile(d, (r, 1)), float(v.sigma_s), float(v.sigma_a),
                             float(v.henyey_greenstein_g), int(wp.max_depth), rng)
        hits += surv.reshape(r, W * H).sum(axis=0)
        done += r
    return (hits / paths_per_pixel).reshape(H, W)
