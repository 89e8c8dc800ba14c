"""numpy float32 restatement of the temporal pass (include/vpt_gpu.h, "Temporal"; the code is csrc/vpt_temporal.h).
Every stated operation is a separate fp32 numpy operation (no fused multiply-add, correctly rounded division and square
root) in the stated order, whole planes at a time, so the GPU's and the host build's results can be compared bit for
bit.  Also the hand-made frames and cameras of the bit-exact tests (host build and GPU) and a float64 projection the
motion plane is held against."""
import ctypes as C

import numpy as np

import denoise_ref as DR

F = np.float32
MIN_WEIGHT = F(0.25)
FLT_MAX = F(3.40282347e+38)
DEFAULTS = dict(max_history=64.0, depth_tol=0.1, sigma_r=4.0, rel_floor=1e-3)
CAMERA_KEYS = ("position", "look", "up", "vfov_deg")


def camera_floats(cam, W, H):
    """The 16 camera floats of a camera dict (all four keys) on a W x H raster, by the library's own derivation
    (vpt_shutter_entry: cam_L's rows with cam_t in the fourth lane, then the position)."""
    from volume_path_tracer_amd import capi

    e = capi.ShutterCamera()
    e.position[:], e.look[:], e.up[:], e.vfov_deg = cam["position"], cam["look"], cam["up"], cam["vfov_deg"]
    out = np.zeros(16, np.float32)
    capi.check(capi.lib().vpt_shutter_entry(C.byref(e), W, H, out.ctypes.data_as(C.POINTER(C.c_float))), "vpt_shutter_entry")
    return out


def _cross(u, v):
    return np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], np.float32)


def _dot(u, v):
    return u[..., 0] * v[..., 0] + (u[..., 1] * v[..., 1] + u[..., 2] * v[..., 2])


def prev_constants(prev16):
    """The previous camera's projection constants (temporal_prev_constants), fp32 in the header's order."""
    e = np.asarray(prev16, np.float32)
    c0, c1, t = e[[0, 4, 8]], e[[1, 5, 9]], e[[3, 7, 11]]
    n = _cross(c0, c1)
    nn = _dot(n, n)
    a = (_cross(c1, n) / nn).astype(np.float32)
    b = (_cross(n, c0) / nn).astype(np.float32)
    return dict(n=n, a=a, b=b, tn=_dot(t, n), ta=_dot(t, a), tb=_dot(t, b), pos=e[12:15].copy())


def pick_depth(depth):
    """z(p): depth[k][p] for the largest k with depth[k][p] > 0, +0 where none is."""
    depth = np.asarray(depth, np.float32)
    z = np.zeros(depth.shape[1:], np.float32)
    for k in range(depth.shape[0]):
        z = np.where(depth[k] > F(0), depth[k], z)
    return z.astype(np.float32)


def directions(cur16, W, H):
    """(rx [1][W], ry [H][1], d [H][W][3]): Camera::generate_ray without jitter, the integrator's expressions."""
    e = np.asarray(cur16, np.float32)
    rx = (np.arange(W, dtype=np.float32) + F(0.5))[None, :]
    ry = (np.arange(H, dtype=np.float32) + F(0.5))[:, None]
    with np.errstate(all="ignore"):
        dv = np.stack([e[4 * i + 3] + (e[4 * i] * rx + (e[4 * i + 1] * ry + e[4 * i + 2] * F(0))) for i in range(3)], axis=-1)
        n2 = dv[..., 0] * dv[..., 0] + (dv[..., 1] * dv[..., 1] + dv[..., 2] * dv[..., 2])
        s = np.sqrt(n2)
        d = np.where((n2 > F(0))[..., None], dv / s[..., None], dv).astype(np.float32)
    return rx, ry, d


def temporal(film, m2, depth, cur16, prev16, history=None, max_history=64.0, depth_tol=0.1, sigma_r=4.0, rel_floor=1e-3):
    """vpt_gpu_temporal restated -> (out film [H][W][4], out m2 [H][W], motion [H][W][2], hist_n [H][W]).
    history: None or (film, m2, depth) of the previous frame."""
    film = np.ascontiguousarray(film, np.float32)
    m2 = np.ascontiguousarray(m2, np.float32)
    depth = np.ascontiguousarray(depth, np.float32)
    H, W = m2.shape
    assert film.shape == (H, W, 4) and depth.shape[1:] == (H, W) and 1 <= depth.shape[0] <= 4
    max_history, depth_tol, sigma_r, rel_floor = F(max_history), F(depth_tol), F(sigma_r), F(rel_floor)
    e = np.asarray(cur16, np.float32)
    P = prev_constants(prev16)
    with np.errstate(all="ignore"):
        z = pick_depth(depth)
        fg = z > F(0)
        rx, ry, d = directions(e, W, H)
        q = np.where(fg[..., None], (e[12:15] + z[..., None] * d) - P["pos"], d).astype(np.float32)
        r = np.sqrt(_dot(q, q))
        lam = P["tn"] / _dot(q, P["n"])
        px = lam * _dot(q, P["a"]) - P["ta"]
        py = lam * _dot(q, P["b"]) - P["tb"]
        proj = (lam > F(0)) & (np.abs(lam) <= FLT_MAX) & (np.abs(px) <= FLT_MAX) & (np.abs(py) <= FLT_MAX)
        motion = np.stack([np.where(proj, px - rx, F(np.nan)), np.where(proj, py - ry, F(np.nan))], axis=-1).astype(np.float32)
        zero = np.zeros((H, W), np.float32)
        if history is None:
            return film.copy(), m2.copy(), motion, zero
        hfilm, hm2, hdepth = (np.ascontiguousarray(a, np.float32) for a in history)
        assert hfilm.shape == film.shape and hm2.shape == m2.shape and hdepth.shape == depth.shape
        hz = pick_depth(hdepth)
        nc = film[..., 3]
        fx, fy = px - F(0.5), py - F(0.5)
        inr = proj & (fx > F(-1)) & (fx < F(W)) & (fy > F(-1)) & (fy < F(H))
        x0f, y0f = np.floor(fx), np.floor(fy)
        ax, ay = fx - x0f, fy - y0f
        x0 = np.where(inr, x0f, 0).astype(np.int64)  # (the range is tested before any conversion to an integer)
        y0 = np.where(inr, y0f, 0).astype(np.int64)
        bx, by = F(1) - ax, F(1) - ay
        w4 = [bx * by, ax * by, bx * ay, ax * ay]
        tol = depth_tol * r
        ws, sm, sn = zero.copy(), zero.copy(), zero.copy()
        s = np.zeros((H, W, 3), np.float32)
        for t in range(4):
            tx, ty = x0 + (t & 1), y0 + (t >> 1)
            inimg = inr & (tx >= 0) & (tx < W) & (ty >= 0) & (ty < H)
            txc, tyc = np.clip(tx, 0, W - 1), np.clip(ty, 0, H - 1)
            hf, hm, zq = hfilm[tyc, txc], hm2[tyc, txc], hz[tyc, txc]
            nq = hf[..., 3]
            agree = np.where(fg, (zq > F(0)) & (np.abs(zq - r) <= tol), ~(zq > F(0)))
            ok = inimg & (nq >= F(1)) & agree
            w = w4[t]
            cq, cm = hf[..., :3] / nq[..., None], hm / nq
            ws = np.where(ok, ws + w, ws)
            s = np.where(ok[..., None], s + w[..., None] * cq, s)
            sm = np.where(ok, sm + w * cm, sm)
            sn = np.where(ok, sn + w * nq, sn)
        ch, sh, n0 = s / ws[..., None], sm / ws, sn / ws
        ccy = film[..., 1] / nc
        v = m2 / nc - ccy * ccy
        v = np.where(v > F(0), v, F(0))
        vc = np.where(nc >= F(2), v / (nc - F(1)), ccy * ccy)
        hy = ch[..., 1]
        dh = sh - hy * hy
        dh = np.where(dh > F(0), dh, F(0))
        nm1 = n0 - F(1)
        nm1 = np.where(nm1 > F(1), nm1, F(1))
        vh = dh / nm1
        err = np.abs(ccy - hy) / ((sigma_r * np.sqrt(vc + vh) + rel_floor * ccy) + F(1e-20))
        nm = np.where(n0 < max_history, n0, max_history)
        nh = nm / (F(1) + err * err)
        use = (nc >= F(1)) & inr & (ws >= MIN_WEIGHT) & (nh > F(0))
        acc = np.concatenate([film[..., :3] + nh[..., None] * ch, (nc + nh)[..., None]], axis=-1).astype(np.float32)
        out = np.where(use[..., None], acc, film)
        out_m2 = np.where(use, m2 + nh * sh, m2)
        hist_n = np.where(use, nh, F(0))
    for a in (out, out_m2, hist_n):
        assert a.dtype == np.float32
    return np.ascontiguousarray(out), np.ascontiguousarray(out_m2), motion, np.ascontiguousarray(hist_n)


def project64(cur16, prev16, z, W, H):
    """Float64 projection of the same fp32 camera rows and depths: the raster point [H][W][2] of the previous camera
    that sees each pixel's point (NaN where lambda <= 0), by a 3 x 3 solve per pixel."""
    e, pe = np.asarray(cur16, np.float64), np.asarray(prev16, np.float64)
    rx = (np.arange(W) + 0.5)[None, :] * np.ones((H, 1))
    ry = (np.arange(H) + 0.5)[:, None] * np.ones((1, W))
    dv = np.stack([e[4 * i + 3] + e[4 * i] * rx + e[4 * i + 1] * ry for i in range(3)], axis=-1)
    d = dv / np.sqrt((dv * dv).sum(-1))[..., None]
    z = np.asarray(z, np.float64)
    q = np.where((z > 0)[..., None], e[12:15] + z[..., None] * d - pe[12:15], d)
    c0, c1, t = pe[[0, 4, 8]], pe[[1, 5, 9]], pe[[3, 7, 11]]
    M = np.empty((H, W, 3, 3))
    M[..., 0], M[..., 1], M[..., 2] = c0, c1, -q
    sol = np.linalg.solve(M, np.broadcast_to(-t, (H, W, 3))[..., None])[..., 0]
    out = sol[..., :2].copy()
    out[~(sol[..., 2] > 0)] = np.nan
    return out


# ---- the hand-made frames of the bit-exact tests ----------------------------------------------------------------------

FRAMES = {"37x21": (37, 21), "1x1": (1, 1), "3x70": (3, 70), "130x9": (130, 9)}
LEVELS = (1, 2)
BASE_CAMERA = {"position": [0.0, 0.0, -300.0], "look": [0.0, 0.0, 0.0], "up": [0.0, 1.0, 0.0], "vfov_deg": 30.0}


def _rot_y(v, deg):
    a = np.radians(deg)
    x, y, z = v
    return [float(F(x * np.cos(a) + z * np.sin(a))), float(y), float(F(-x * np.sin(a) + z * np.cos(a)))]


def previous_cameras():
    """The previous cameras of the cases, by name, against BASE_CAMERA as the current one."""
    b = BASE_CAMERA
    return {
        "same": dict(b),
        "orbit2": dict(b, position=_rot_y(b["position"], 2.0)),
        "dolly": dict(b, position=[0.0, 0.0, -220.0]),       # towards the volume: parallax
        "turn120": dict(b, look=[b["position"][i] + v for i, v in enumerate(_rot_y([0.0, 0.0, 300.0], 120.0))]),
        "behind": dict(b, position=[0.0, 0.0, 20.0], look=[0.0, 0.0, 400.0]),  # the volume lies behind it
    }


def sphere_depth(cam16, W, H, radii=(60.0, 35.0), centre=(0.0, 0.0, 0.0)):
    """Depth planes [K][H][W] of concentric spheres about `centre` seen by a camera: the distance along the unit
    camera direction to each sphere (float64, rounded once), +0 where the ray misses; level k + 1's sphere lies inside
    level k's, so the reached levels are a prefix."""
    e = np.asarray(cam16, np.float64)
    rx = (np.arange(W) + 0.5)[None, :] * np.ones((H, 1))
    ry = (np.arange(H) + 0.5)[:, None] * np.ones((1, W))
    dv = np.stack([e[4 * i + 3] + e[4 * i] * rx + e[4 * i + 1] * ry for i in range(3)], axis=-1)
    d = dv / np.sqrt((dv * dv).sum(-1))[..., None]
    oc = e[12:15] - np.asarray(centre, np.float64)
    b = (d * oc).sum(-1)
    out = []
    for R in radii:
        disc = b * b - ((oc * oc).sum() - R * R)
        with np.errstate(all="ignore"):
            t = -b - np.sqrt(disc)
        out.append(np.where((disc > 0) & (t > 0), t, 0.0).astype(np.float32))
    return np.stack(out)


def hand_made_case(W, H, K, prev="orbit2", seed=5, nan_invalid=True):
    """(film, m2, depth, cur16, prev16, (hist film, hist m2, hist depth)) of one case: denoise_ref's hand-made films
    (0, 1 and many samples per pixel, NaN in the unrendered ones) for the frame and, from another seed, its history;
    sphere depths seen by each frame's own camera, so the reprojection meets surfaces that agree and edges that do not.
    A 1 x 1 frame looks at the spheres' centre."""
    cur16 = camera_floats(BASE_CAMERA, W, H)
    prev16 = camera_floats(previous_cameras()[prev], W, H)
    film, m2, _ = DR.hand_made_frame(W, H, 0, seed=seed, nan_invalid=nan_invalid)
    hfilm, hm2, _ = DR.hand_made_frame(W, H, 0, seed=seed + 100, nan_invalid=nan_invalid)
    radii = (60.0, 35.0)[:K]
    depth, hdepth = sphere_depth(cur16, W, H, radii), sphere_depth(prev16, W, H, radii)
    if nan_invalid and W * H > 1:  # (what an unrendered history pixel's depth holds does not matter either)
        hdepth = hdepth.copy()
        hdepth[:, hfilm[..., 3] == 0] = np.nan
    return film, m2, depth, cur16, prev16, (hfilm, hm2, hdepth)
