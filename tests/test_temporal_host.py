"""The temporal pass, host side (no GPU): the ABI entry vpt_gpu_temporal and its argument checks; the numpy restatement
(tests/temporal_ref.py) checked step by step on one pixel; the host build of csrc/vpt_temporal.h's per-pixel function
(tests/native/temporal_host.cpp, bound by tests/temporal_lib.py) against the restatement, byte for byte; the pass's
properties on both; the motion plane against a float64 projection; and its quality on oracle-rendered frames of an
orbit against a 1024-wave reference."""
import ctypes as C

import numpy as np
import pytest

import temporal_lib as TL
import temporal_ref as R
from volume_path_tracer_amd import capi

F = np.float32
VPT_E_INVALID = 1
IMPLS = {"restatement": R.temporal, "host-build": TL.temporal}
CAMERAS = list(R.previous_cameras())


def same_bytes(a, b):
    return all(x.dtype == np.float32 and x.tobytes() == y.tobytes() for x, y in zip(a, b))


# ---------------------------------------------------------------------------------------- 1. exports and arguments

def test_export_abi_and_struct_size():
    L = capi.lib()
    assert hasattr(L, "vpt_gpu_temporal")
    assert L.vpt_abi_version() == 1  # (a symbol was added, nothing changed)
    assert C.sizeof(capi.TemporalParams) == 20
    p = capi.TemporalParams.make(2, 48, 0.05, 3.0, 2e-3)
    assert (p.n_levels, p.max_history, p.depth_tol, p.sigma_r, p.rel_floor) == (2, 48.0, F(0.05), 3.0, F(2e-3))
    d = capi.TemporalParams.make()
    assert (d.n_levels, d.depth_tol, d.sigma_r, d.rel_floor) == (2, F(0.1), 4.0, F(1e-3))


def _camera(**kw):
    cam = dict(R.BASE_CAMERA, **kw)
    e = capi.ShutterCamera()
    e.position[:], e.look[:], e.up[:], e.vfov_deg = cam["position"], cam["look"], cam["up"], cam["vfov_deg"]
    return e


def test_argument_checks_need_no_device():
    """Every VPT_E_INVALID of the header that does not need a context's size: the arguments are checked before the
    context is, so a null context with good arguments is the last refusal."""
    L = capi.lib()
    buf = (C.c_float * 64)()
    a16 = (C.addressof(buf) + 15) // 16 * 16
    ptr = C.c_void_p(a16)
    good, cam = capi.TemporalParams.make(), _camera()

    def call(p=good, film=ptr, m2=ptr, depth=ptr, prev=cam, hf=ptr, hm=ptr, hd=ptr, out=ptr, om=ptr, mv=None, hn=None):
        rc = L.vpt_gpu_temporal(None, C.byref(p) if p is not None else None, film, m2, depth,
                                C.byref(prev) if prev is not None else None, hf, hm, hd, out, om, mv, hn, None)
        return rc, L.vpt_last_error()

    rc, msg = call()
    assert rc == VPT_E_INVALID and b"null context" in msg
    rc, msg = call(hf=None, hm=None, hd=None)  # (no history is a good call)
    assert rc == VPT_E_INVALID and b"null context" in msg
    rc, msg = call(mv=ptr, hn=ptr)
    assert rc == VPT_E_INVALID and b"null context" in msg
    rc, msg = call(p=None)
    assert rc == VPT_E_INVALID and b"null params" in msg
    for kw in ({"film": None}, {"m2": None}, {"depth": None}):
        rc, msg = call(**kw)
        assert rc == VPT_E_INVALID and b"null film, moment plane or depth" in msg, kw
    for kw in ({"out": None}, {"om": None}):
        rc, msg = call(**kw)
        assert rc == VPT_E_INVALID and b"null output" in msg, kw
    rc, msg = call(prev=None)
    assert rc == VPT_E_INVALID and b"null previous camera" in msg
    for kw in ({"hf": None}, {"hm": None}, {"hd": None}, {"hf": None, "hm": None}, {"hm": None, "hd": None},
               {"hf": None, "hd": None}):
        rc, msg = call(**kw)
        assert rc == VPT_E_INVALID and b"all three NULL" in msg, kw
    for k in (0, 5, 0xFFFFFFFF):
        rc, msg = call(p=capi.TemporalParams.make(n_levels=k))
        assert rc == VPT_E_INVALID and b"n_levels" in msg
    for bad in (0.0, -1.0, float("nan")):
        for name in ("max_history", "depth_tol", "sigma_r", "rel_floor"):
            rc, msg = call(p=capi.TemporalParams.make(**{name: bad}))
            assert rc == VPT_E_INVALID and b"must be > 0" in msg, (name, bad)
    # alignment: the films are read and written as float4, the planes as floats
    off4, off8, off2 = C.c_void_p(a16 + 4), C.c_void_p(a16 + 8), C.c_void_p(a16 + 2)
    for kw in ({"film": off4}, {"hf": off8}, {"out": off4}, {"m2": off2}, {"depth": off2}, {"hm": off2}, {"hd": off2},
               {"om": off2}, {"mv": off2}, {"hn": off2}):
        rc, msg = call(**kw)
        assert rc == VPT_E_INVALID and b"aligned" in msg, kw
    for kw in ({"m2": off4}, {"depth": off4}, {"om": off8}, {"mv": off4}, {"hn": off4}):  # (a plane needs 4 bytes only)
        rc, msg = call(**kw)
        assert rc == VPT_E_INVALID and b"null context" in msg, kw
    # the previous camera, by the shutter's rules
    p = R.BASE_CAMERA["position"]
    for why, bad in ((b"not finite", _camera(position=[float("nan"), 0.0, 0.0])),
                     (b"not finite", _camera(up=[0.0, float("inf"), 0.0])),
                     (b"look equals position", _camera(look=p)),
                     (b"up is zero or parallel", _camera(up=[0.0, 0.0, 0.0])),
                     (b"up is zero or parallel", _camera(up=[0.0, 0.0, 2.0])),
                     (b"vfov_deg", _camera(vfov_deg=0.0)), (b"vfov_deg", _camera(vfov_deg=180.0)),
                     (b"vfov_deg", _camera(vfov_deg=float("nan")))):
        rc, msg = call(prev=bad)
        assert rc == VPT_E_INVALID and b"previous camera" in msg and why in msg, (why, msg)


# -------------------------------------------------------------------------------------------------- 2. restatement

def test_constants_of_the_host_build_equal_the_restatement():
    for name, cam in R.previous_cameras().items():
        prev16 = R.camera_floats(cam, 37, 21)
        want, got = R.prev_constants(prev16), TL.constants(prev16)
        for k in ("n", "a", "b", "tn", "ta", "tb"):
            assert np.asarray(want[k], np.float32).tobytes() == np.asarray(got[k], np.float32).tobytes(), (name, k)
        # the constants do what they are for: L0' . a = L1' . b = 1, the cross terms and the normal vanish (float64)
        c0, c1 = prev16[[0, 4, 8]].astype(np.float64), prev16[[1, 5, 9]].astype(np.float64)
        a, b, n = (np.asarray(want[k], np.float64) for k in ("a", "b", "n"))
        assert abs(c0 @ a - 1) < 1e-5 and abs(c1 @ b - 1) < 1e-5
        assert abs(c1 @ a) < 1e-5 and abs(c0 @ b) < 1e-5 and abs(c0 @ n) < 1e-9 and abs(c1 @ n) < 1e-9


def test_restatement_on_a_hand_made_pixel():
    """A 2 x 1 frame, one level, the history's camera a 2-degree orbit away: pixel 0 operation by operation with
    fp32 scalars, in the header's order."""
    W, H = 2, 1
    cur = R.camera_floats(R.BASE_CAMERA, W, H)
    prev = R.camera_floats(R.previous_cameras()["orbit2"], W, H)
    film = np.array([[[2.0, 4.0, 8.0, 4.0], [0.75, 1.5, 3.0, 1.0]]], np.float32)
    m2 = np.array([[4.75, 2.25]], np.float32)
    hfilm = np.array([[[6.0, 12.5, 24.0, 12.0], [3.0, 7.0, 12.0, 6.0]]], np.float32)
    hm2 = np.array([[14.5, 9.0]], np.float32)
    depth = np.array([[[290.0, 291.0]]], np.float32)
    hdepth = np.array([[[290.5, 330.0]]], np.float32)  # (the second tap lies too deep: rejected)
    max_history, depth_tol, sigma_r, rel_floor = F(8.0), F(0.1), F(4.0), F(1e-3)
    # previous camera's constants
    c0, c1, t = prev[[0, 4, 8]], prev[[1, 5, 9]], prev[[3, 7, 11]]
    cross = lambda u, v: np.array([u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]], np.float32)
    dot = lambda u, v: u[0] * v[0] + (u[1] * v[1] + u[2] * v[2])
    n = cross(c0, c1)
    nn = dot(n, n)
    a, b = cross(c1, n) / nn, cross(n, c0) / nn
    tn, ta, tb = dot(t, n), dot(t, a), dot(t, b)
    # pixel (0, 0)
    rx, ry = F(0) + F(0.5), F(0) + F(0.5)
    dv = np.array([cur[4 * i + 3] + (cur[4 * i] * rx + (cur[4 * i + 1] * ry + cur[4 * i + 2] * F(0))) for i in range(3)], np.float32)
    d = dv / np.sqrt(dv[0] * dv[0] + (dv[1] * dv[1] + dv[2] * dv[2]))
    z = depth[0, 0, 0]
    q = (cur[12:15] + z * d) - prev[12:15]
    r = np.sqrt(dot(q, q))
    lam = tn / dot(q, n)
    px, py = lam * dot(q, a) - ta, lam * dot(q, b) - tb
    assert lam > 0 and 0.5 < px < 1.5 and abs(py - 0.5) < 1e-3  # (moved by a fraction of a pixel, along x)
    fx, fy = px - F(0.5), py - F(0.5)
    x0, y0 = np.floor(fx), np.floor(fy)
    ax, ay = fx - x0, fy - y0
    weights = [(F(1) - ax) * (F(1) - ay), ax * (F(1) - ay), (F(1) - ax) * ay, ax * ay]
    ws = sm = sn = F(0)
    s = np.zeros(3, np.float32)
    used = []
    for k, w in enumerate(weights):
        tx, ty = int(x0) + (k & 1), int(y0) + (k >> 1)
        if not (0 <= tx < W and 0 <= ty < H):
            continue
        nq, zq = hfilm[ty, tx, 3], hdepth[0, ty, tx]
        if not (nq >= 1 and zq > 0 and np.abs(zq - r) <= depth_tol * r):
            continue
        used.append((tx, ty))
        ws = ws + w
        s = s + w * (hfilm[ty, tx, :3] / nq)
        sm = sm + w * (hm2[ty, tx] / nq)
        sn = sn + w * nq
    assert used == [(0, 0)] and ws >= F(0.25)  # (one row: the taps of the other row are outside; (1, 0) too deep)
    ch, sh, n0 = s / ws, sm / ws, sn / ws
    assert n0 == 12 and ch[1] == F(12.5) / F(12)  # (one tap: the renormalisation returns it)
    nc = film[0, 0, 3]
    ccy = film[0, 0, 1] / nc
    vc = (m2[0, 0] / nc - ccy * ccy) / (nc - F(1))
    vh = max(sh - ch[1] * ch[1], F(0)) / max(n0 - F(1), F(1))
    e = np.abs(ccy - ch[1]) / ((sigma_r * np.sqrt(vc + vh) + rel_floor * ccy) + F(1e-20))
    nh = min(n0, max_history) / (F(1) + e * e)
    assert 7.9 < nh < 8.0  # (capped at 8, hardly rejected: the means are 1 and 1.04)
    want_film = np.append(film[0, 0, :3] + nh * ch, nc + nh).astype(np.float32)
    want_m2 = m2[0, 0] + nh * sh
    for name, fn in IMPLS.items():
        out, om2, mv, hn = fn(film, m2, depth, cur, prev, (hfilm, hm2, hdepth), max_history=max_history,
                              depth_tol=depth_tol, sigma_r=sigma_r, rel_floor=rel_floor)
        assert out[0, 0].tobytes() == want_film.tobytes(), name
        assert om2[0, 0].tobytes() == F(want_m2).tobytes() and hn[0, 0].tobytes() == F(nh).tobytes(), name
        assert mv[0, 0].tobytes() == np.array([px - rx, py - ry], np.float32).tobytes(), name
        assert out.dtype == om2.dtype == mv.dtype == hn.dtype == np.float32


# ---------------------------------------------------------------------------- 3. host build == restatement, bytes

@pytest.mark.parametrize("prev", CAMERAS)
@pytest.mark.parametrize("K", R.LEVELS)
@pytest.mark.parametrize("frame", list(R.FRAMES))
def test_host_build_equals_restatement(frame, K, prev):
    W, H = R.FRAMES[frame]
    film, m2, depth, cur, prv, hist = R.hand_made_case(W, H, K, prev)
    n = film[..., 3]
    if W * H > 1:
        assert (n == 0).any() and (n == 1).any() and (n > 1).any() and np.isnan(film[n == 0, :3]).all()
        z = R.pick_depth(depth)
        assert (z > 0).any() and (z == 0).any()  # foreground and background
    before = [a.copy() for a in (film, m2, depth, *hist)]
    want = R.temporal(film, m2, depth, cur, prv, hist)
    got = TL.temporal(film, m2, depth, cur, prv, hist)  # (NaN-filled before the call)
    for a, b, what in zip(want, got, ("film", "m2", "motion", "hist_n")):
        assert a.tobytes() == b.tobytes(), (what, int((a.view(np.uint32) != b.view(np.uint32)).sum()))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(before, (film, m2, depth, *hist)))  # the inputs are unchanged
    out, om2, mv, hn = got
    assert np.isfinite(hn).all() and (hn >= 0).all() and (hn <= 64).all()
    used = hn > 0
    assert np.isfinite(out[used]).all() and np.isfinite(om2[used]).all()
    assert out[~used].tobytes() == film[~used].tobytes() and om2[~used].tobytes() == m2[~used].tobytes()
    if prev in ("same", "orbit2", "dolly") and W * H > 1:
        assert used.sum() > 0.3 * W * H  # (it accumulated)
    if prev == "turn120":
        assert used.sum() < 0.3 * W * H and np.isnan(mv).any()  # most history off-screen, some pixels behind
    if prev == "behind":
        assert np.isnan(mv[R.pick_depth(depth) > 0]).all() and not used[R.pick_depth(depth) > 0].any()


# -------------------------------------------------------------------------------------------------- 4. properties

@pytest.mark.parametrize("impl", list(IMPLS))
def test_invalid_pixels_and_rejected_taps_do_not_leak(impl):
    film, m2, depth, cur, prv, (hf, hm, hd) = R.hand_made_case(37, 21, 2, "orbit2", seed=9)
    bad = hf[..., 3] == 0
    assert bad.sum() > 50 and np.isnan(hf[bad, :3]).all() and np.isnan(hm[bad]).all() and np.isnan(hd[:, bad]).all()
    out, om2, mv, hn = IMPLS[impl](film, m2, depth, cur, prv, (hf, hm, hd))
    used = hn > 0
    assert used.sum() > 300 and np.isfinite(out[used]).all() and np.isfinite(om2[used]).all() and np.isfinite(hn).all()
    cur_bad = film[..., 3] == 0
    assert out[cur_bad].tobytes() == film[cur_bad].tobytes() and (hn[cur_bad] == 0).all()  # copied, NaN payloads included
    # what the unrendered history pixels hold does not matter
    hf2, hm2, hd2 = hf.copy(), hm.copy(), hd.copy()
    hf2[bad, :3], hm2[bad], hd2[:, bad] = 1e30, -5.0, 250.0
    assert same_bytes(IMPLS[impl](film, m2, depth, cur, prv, (hf2, hm2, hd2)), (out, om2, mv, hn))
    # nor what a tap rejected by its depth holds: poison every history pixel that is foreground, and ask for agreement
    # no history depth can give (the background pixels still accumulate background)
    fgq = R.pick_depth(hd) > 0
    hf3, hm3 = hf.copy(), hm.copy()
    hf3[fgq, :3], hm3[fgq] = np.nan, np.nan
    hd3 = np.where(hd > 0, hd + F(1000), hd).astype(np.float32)
    out3, om23, _, hn3 = IMPLS[impl](film, m2, depth, cur, prv, (hf3, hm3, hd3))
    fg = R.pick_depth(depth) > 0
    assert (hn3[fg] == 0).all() and out3[fg].tobytes() == film[fg].tobytes()
    assert (hn3[~fg] > 0).any() and np.isfinite(out3[hn3 > 0]).all() and np.isfinite(om23[hn3 > 0]).all()


@pytest.mark.parametrize("impl", list(IMPLS))
def test_no_history_gives_the_inputs_bytes(impl):
    film, m2, depth, cur, prv, _ = R.hand_made_case(37, 21, 2, "orbit2")
    out, om2, mv, hn = IMPLS[impl](film, m2, depth, cur, prv, None)
    assert out.tobytes() == film.tobytes() and om2.tobytes() == m2.tobytes()
    assert hn.tobytes() == np.zeros_like(hn).tobytes()  # (+0)
    assert np.isfinite(mv).all() and np.abs(mv).max() > 0.5  # the motion plane is written all the same


@pytest.mark.parametrize("impl", list(IMPLS))
def test_accumulation_adds_what_the_header_says(impl):
    """The same camera and the same surfaces: every rendered pixel takes its history, the count grows by n_h <=
    min(n_q, max_history), and the output's mean lies between the frame's and the history's."""
    film, m2, depth, cur, prv, (hf, hm, hd) = R.hand_made_case(37, 21, 2, "same", nan_invalid=False)
    hf, hm = hf.copy(), hm.copy()
    hf[hf[..., 3] == 0] = [1.0, 2.0, 4.0, 2.0]  # (every history pixel rendered)
    hm[hm == 0] = 4.5
    out, om2, mv, hn = IMPLS[impl](film, m2, depth, cur, prv, (hf, hm, hd), max_history=16.0)
    ok = film[..., 3] >= 1
    assert (hn[ok] > 0).all() and (hn[~ok] == 0).all()
    # (the motion is ~1e-5 pixels, not 0: the neighbours' counts, up to 39, enter with that weight)
    assert (hn <= 16).all() and (hn <= hf[..., 3] + 1e-2).all()
    assert np.allclose(out[..., 3][ok], film[..., 3][ok] + hn[ok], rtol=1e-6)
    cy, hy, oy = film[..., 1][ok] / film[..., 3][ok], hf[..., 1][ok] / hf[..., 3][ok], out[..., 1][ok] / out[..., 3][ok]
    lo, hi = np.minimum(cy, hy), np.maximum(cy, hy)
    assert (oy >= lo * (1 - 1e-4)).all() and (oy <= hi * (1 + 1e-4)).all()
    # A history whose Y lies 100 above (the same spread: sum += n delta, m2 += 2 delta sum + n delta^2) is rejected,
    # softly.  Where the frame has 8 samples or more, the samples' spread is at most 1.5 (hand_made_frame: 3.5 * 1.5 *
    # 0.29), so sqrt(v_c + v_h) <= 0.8, e >= 100 / 3.3 = 30 and n_h <= 16 / 900.
    hf_far, nq, delta = hf.copy(), hf[..., 3], F(100)
    hf_far[..., 1] = hf[..., 1] + nq * delta
    hm_far = hm + F(2) * delta * hf[..., 1] + nq * delta * delta
    _, _, _, hn_far = IMPLS[impl](film, m2, depth, cur, prv, (hf_far, hm_far, hd), max_history=16.0)
    many = film[..., 3] >= 8
    assert many.sum() > 300 and hn_far[many].max() < 0.02 and (hn_far[ok] < hn[ok]).all()


# --------------------------------------------------------------------------------------------------- 5. geometry

# The motion plane of the host build against a float64 projection of the same fp32 camera rows and depths, in pixels,
# over the hand-made cases: the largest error measured is 5.1e-4 (130 x 9, the 120-degree turn, motion vectors of up to
# 488 pixels; 2.7e-5 over every other case); the bar is four times that.
MOTION_ERROR_MEASURED = 5.1e-4
MOTION_BAR = 4 * MOTION_ERROR_MEASURED


def test_motion_plane_against_a_float64_projection():
    worst = 0.0
    for frame, (W, H) in R.FRAMES.items():
        for prev in CAMERAS:
            film, m2, depth, cur, prv, _ = R.hand_made_case(W, H, 2, prev)
            _, _, mv, _ = TL.temporal(film, m2, depth, cur, prv, None)
            want = R.project64(cur, prv, R.pick_depth(depth), W, H)
            ys, xs = np.mgrid[0:H, 0:W]
            got = mv.astype(np.float64) + np.stack([xs + 0.5, ys + 0.5], -1)
            assert np.array_equal(np.isnan(got).any(-1), np.isnan(want).any(-1)), (frame, prev)
            both = ~np.isnan(want).any(-1)
            err = float(np.abs(got - want)[both].max()) if both.any() else 0.0
            print(f"{frame} {prev}: motion error {err:.3g} px")
            assert err <= MOTION_BAR, (frame, prev, err)
            worst = max(worst, err)
            if prev == "same":  # the current camera as the previous one: nothing moves
                assert np.abs(mv).max() < MOTION_BAR
    print("largest motion error", worst)


# ------------------------------------------------------------------------------------------------------ 6. quality

# Accumulated + denoised over spatially denoised only (the existing code: the yardstick), relative RMSE of Y / W against
# the oracle's 1024-wave frame 3; measured 0.794 (c3) and 0.861 (c4) at the defaults, the bar halfway between that and
# 1 (EXPERIMENTS.md §27).
QUALITY_MEASURED = {"c3": 0.794, "c4": 0.861}
QUALITY_BAR = {name: 0.5 * (r + 1.0) for name, r in QUALITY_MEASURED.items()}


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_quality_on_oracle_frames(name):
    """Frames 0..3 of scenes.orbit(cfg, 120) (3 degrees a frame, seeds seed + k, 64^3 stand-in, 48 x 48, 16 waves) by
    the unchanged oracle, accumulated by the host build.  Measured figures: EXPERIMENTS.md §27."""
    import temporal_quality as Q

    r = Q.measure(name)
    print(name, " ".join(f"{k} {v:.4f}" for k, v in r.items()))
    # the accumulated raw film beats frame 3's own raw film
    assert r["acc"] < r["raw"], r
    # a static camera and four independent frames: two frames' worth is a floor on what four must deliver
    assert r["static_acc"] < r["static_one"] / np.sqrt(2.0), r
    # accumulated + denoised against spatially denoised only
    assert r["ratio"] <= QUALITY_BAR[name], (r["ratio"], QUALITY_BAR[name])
    assert 16 < r["mean_count"] <= 16 + 4 * 16
    # and the restatement gives the host build's bytes on these films too
    s = Q.scene(name)
    (f0, m0, d0, c0), (f1, m1, d1, c1) = s["orbit"][0], s["orbit"][1]
    assert same_bytes(R.temporal(f1, m1, d1, c1, c0, (f0, m0, d0)), TL.temporal(f1, m1, d1, c1, c0, (f0, m0, d0)))


# ------------------------------------------------------------------------------------- 7. the stand-alone program

@pytest.mark.parametrize("sanitize", [False, True])
def test_temporal_host_program(tmp_path, sanitize):
    """The stand-alone program accumulates the four frame sizes at one and two levels through five previous cameras,
    with and without a history (NaN in the unrendered pixels), and exits 0 when every pixel either passed through
    byte for byte or is finite with a grown count.  Once more as an AddressSanitizer + UBSan build, run directly as a
    plain process."""
    import subprocess

    extra = ["-O1", "-g", "-DTEMPORAL_HOST_MAIN"]
    if sanitize:
        extra += ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe = TL.compile_host(tmp_path / ("temporal_host_san" if sanitize else "temporal_host"), extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "temporal_host: 0 bad values" in r.stdout
