"""The denoiser, host side (no GPU): the ABI entry vpt_gpu_denoise and its argument checks; the numpy restatement
(tests/denoise_ref.py) checked by hand on one pixel; the host build of csrc/vpt_denoise.h's per-pixel functions
(tests/native/denoise_host.cpp, bound by tests/denoise_lib.py) against the restatement, byte for byte; the filter's
properties on both; and its quality on oracle-rendered frames against a 1024-wave reference."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_ref as A
import denoise_lib as DL
import denoise_ref as R
from volume_path_tracer_amd import capi

F = np.float32
VPT_E_INVALID = 1
IMPLS = {"restatement": R.denoise, "host-build": DL.denoise}


# ---------------------------------------------------------------------------------------- 1. exports and arguments

def test_export_abi_and_struct_size():
    L = capi.lib()
    assert hasattr(L, "vpt_gpu_denoise")
    assert L.vpt_abi_version() == 1  # (symbols were added, nothing changed)
    assert C.sizeof(capi.DenoiseParams) == 32
    p = capi.DenoiseParams.make(5, 2, 3.0, 2e-3, [0.25, 0.5])
    assert (p.iterations, p.n_guides, p.sigma_l, p.rel_floor) == (5, 2, 3.0, F(2e-3))
    assert list(p.guide_sigma)[:2] == [0.25, 0.5]
    assert list(capi.DenoiseParams.make(4, 3).guide_sigma)[:3] == [F(0.2)] * 3
    with pytest.raises(ValueError):
        capi.DenoiseParams.make(4, 2, guide_sigma=[0.2])


def test_argument_checks_need_no_device():
    """Every VPT_E_INVALID of the header that does not need a context's size: the arguments are checked before the
    context is, so a null context with good arguments is the last refusal."""
    L = capi.lib()
    buf = (C.c_float * 64)()
    ptr = C.c_void_p((C.addressof(buf) + 15) // 16 * 16)  # (16-byte aligned, as the call requires of the films)
    guides = (C.c_void_p * 4)(ptr, ptr, ptr, ptr)

    def call(p, film=ptr, m2=ptr, g=guides, out=ptr):
        rc = L.vpt_gpu_denoise(None, C.byref(p) if p is not None else None, film, m2, g, out, None, None)
        return rc, L.vpt_last_error()

    good = capi.DenoiseParams.make(4, 2)
    rc, msg = call(good)
    assert rc == VPT_E_INVALID and b"null context" in msg
    rc, msg = call(None)
    assert rc == VPT_E_INVALID and b"null params" in msg
    for kw in ({"film": None}, {"m2": None}, {"out": None}):
        rc, msg = call(good, **kw)
        assert rc == VPT_E_INVALID and b"null film, moment plane or output" in msg, kw
    for it in (0, 7, 0xFFFFFFFF):
        rc, msg = call(capi.DenoiseParams.make(it, 0))
        assert rc == VPT_E_INVALID and b"iterations" in msg
    rc, msg = call(capi.DenoiseParams.make(4, 5, guide_sigma=[0.2] * 5))
    assert rc == VPT_E_INVALID and b"at most 4 guides" in msg
    for bad in (0.0, -1.0, float("nan")):
        rc, msg = call(capi.DenoiseParams.make(4, 0, sigma_l=bad))
        assert rc == VPT_E_INVALID and b"sigma_l and rel_floor" in msg
        rc, msg = call(capi.DenoiseParams.make(4, 0, rel_floor=bad))
        assert rc == VPT_E_INVALID and b"sigma_l and rel_floor" in msg
        rc, msg = call(capi.DenoiseParams.make(4, 2, guide_sigma=[0.2, bad]))
        assert rc == VPT_E_INVALID and b"guide_sigma" in msg
    rc, msg = call(capi.DenoiseParams.make(4, 1, guide_sigma=[0.2, float("nan")]))  # (an unused sigma is not read)
    assert rc == VPT_E_INVALID and b"null context" in msg
    rc, msg = call(good, g=None)
    assert rc == VPT_E_INVALID and b"null guide array" in msg
    rc, msg = call(good, g=(C.c_void_p * 4)(ptr, None, ptr, ptr))
    assert rc == VPT_E_INVALID and b"null guide plane" in msg
    rc, msg = call(capi.DenoiseParams.make(4, 0), g=None)  # (no guides: the array may be null)
    assert rc == VPT_E_INVALID and b"null context" in msg
    # alignment: the films are read and written as float4, the planes as floats
    base = C.addressof(buf)  # (not necessarily 16-byte aligned: take the offsets from the next 16-byte point)
    a16 = (base + 15) // 16 * 16
    p16, off4, off2 = C.c_void_p(a16), C.c_void_p(a16 + 4), C.c_void_p(a16 + 2)
    rc, msg = call(good, film=p16, m2=p16, g=(C.c_void_p * 4)(a16, a16, a16, a16), out=p16)
    assert rc == VPT_E_INVALID and b"null context" in msg  # (aligned: passes on to the context check)
    for kw in ({"film": off4}, {"out": off4}, {"film": C.c_void_p(a16 + 8)}, {"m2": off2},
               {"g": (C.c_void_p * 4)(a16, a16 + 2, a16, a16)}):
        args = dict(film=p16, m2=p16, g=(C.c_void_p * 4)(a16, a16, a16, a16), out=p16)
        args.update(kw)
        rc, msg = call(good, **args)
        assert rc == VPT_E_INVALID and b"aligned" in msg, kw
    rc = L.vpt_gpu_denoise(None, C.byref(good), p16, p16, (C.c_void_p * 4)(a16, a16, a16, a16), p16, off2, None)
    assert rc == VPT_E_INVALID and b"aligned" in L.vpt_last_error()  # (the variance plane)


# -------------------------------------------------------------------------------------------------- 2. restatement

def test_restatement_on_a_hand_made_pixel():
    """A 2 x 1 film, one iteration, one guide: pixel 0 (n = 4) by hand, operation by operation; pixel 1 has n = 1."""
    film = np.array([[[2.0, 4.0, 8.0, 4.0], [0.75, 1.5, 3.0, 1.0]]], np.float32)
    m2 = np.array([[4.75, 2.25]], np.float32)
    g = np.array([[0.25, 0.75]], np.float32)
    sg, sigma_l, rel_floor = F(0.5), F(4.0), F(1e-3)
    # prepare
    c0 = film[0, 0, :3] / F(4)                        # (0.5, 1, 2)
    v0 = (F(4.75) / F(4) - c0[1] * c0[1]) / (F(4) - F(1))
    assert v0 == F(0.1875) / F(3)
    c1 = film[0, 1, :3] / F(1)
    v1 = c1[1] * c1[1]                                # one sample: its own square
    assert v1 == F(2.25)
    # gv: row-major over the valid in-image neighbours of pixel 0: itself (1/2 * 1/2) and pixel 1 (1/2 * 1/4)
    gs = F(0) + (F(0.5) * F(0.5)) * v0
    gw = F(0) + F(0.5) * F(0.5)
    gs = gs + (F(0.5) * F(0.25)) * v1
    gw = gw + F(0.5) * F(0.25)
    gv = gs / gw
    den = (sigma_l * np.sqrt(gv) + rel_floor * c0[1]) + F(1e-20)
    # taps: the centre (dy 0, dx 0) then pixel 1 (dy 0, dx +1)
    d = np.abs(c0[1] - c0[1]) / den
    w = (F(0.375) * F(0.375)) / (F(1) + d * d)
    e = (g[0, 0] - g[0, 0]) / sg
    w = w / (F(1) + e * e)
    acc = F(0) + w * c0
    accv = F(0) + (w * w) * v0
    ws = F(0) + w
    d = np.abs(c0[1] - c1[1]) / den
    w = (F(0.375) * F(0.25)) / (F(1) + d * d)
    e = (g[0, 0] - g[0, 1]) / sg
    w = w / (F(1) + e * e)
    acc = acc + w * c1
    accv = accv + (w * w) * v1
    ws = ws + w
    want_c, want_v = acc / ws, accv / (ws * ws)
    for name, fn in IMPLS.items():
        out, var = fn(film, m2, [g], [sg], iterations=1, sigma_l=sigma_l, rel_floor=rel_floor)
        assert out.dtype == np.float32 and var.dtype == np.float32
        assert out[0, 0].tobytes() == np.append(want_c * F(4), F(4)).astype(np.float32).tobytes(), name
        assert var[0, 0].tobytes() == F(want_v).tobytes(), name
        assert out[0, 1, 3] == 1 and 1.0 < out[0, 1, 1] < 1.5  # (pulled toward its neighbour, within the range)
    assert 1.0 < want_c[1] < 1.5 and v0 < want_v < v1  # (the second tap counted, with its one-sample variance)


# ---------------------------------------------------------------------------- 3. host build == restatement, bytes

@pytest.mark.parametrize("n_guides", R.GUIDE_COUNTS)
@pytest.mark.parametrize("frame", list(R.FRAMES))
def test_host_build_equals_restatement(frame, n_guides):
    W, H, K = R.FRAMES[frame]
    film, m2, guides = R.hand_made_frame(W, H, n_guides)
    n = film[..., 3]
    if W * H > 1:
        assert (n == 0).any() and (n == 1).any() and (n > 1).any()
    sg = R.GUIDE_SIGMA[:n_guides]
    want, want_v = R.denoise(film, m2, guides, sg, iterations=K)
    got, got_v = DL.denoise(film, m2, guides, sg, iterations=K)  # (NaN-filled before the call)
    assert got.tobytes() == want.tobytes(), int((got.view(np.uint32) != want.view(np.uint32)).sum())
    assert got_v.tobytes() == want_v.tobytes()
    assert np.isfinite(got_v).all() and np.isfinite(got[n >= 1]).all()
    if W * H > 1:
        assert (got[n >= 1] != film[n >= 1]).any()  # (it filtered)


# -------------------------------------------------------------------------------------------------- 4. properties

@pytest.mark.parametrize("impl", list(IMPLS))
def test_invalid_pixels_do_not_leak(impl):
    film, m2, guides = R.hand_made_frame(37, 21, 2, seed=9, nan_invalid=True)
    bad = film[..., 3] == 0
    assert bad.sum() > 50 and np.isnan(film[bad, :3]).all() and np.isnan(m2[bad]).all() and np.isnan(guides[1][bad]).all()
    out, var = IMPLS[impl](film, m2, guides, [0.2, 0.2], iterations=5)
    assert out[bad].tobytes() == film[bad].tobytes()  # copied, NaN payloads included
    assert np.isfinite(out[~bad]).all() and np.isfinite(var).all() and (var[bad] == 0).all()
    # and what the unrendered pixels hold does not matter
    film2, m22, guides2 = film.copy(), m2.copy(), [g.copy() for g in guides]
    film2[bad, :3], m22[bad] = 1e30, -5.0
    for g in guides2:
        g[bad] = 77.0
    out2, var2 = IMPLS[impl](film2, m22, guides2, [0.2, 0.2], iterations=5)
    assert out2[~bad].tobytes() == out[~bad].tobytes() and var2.tobytes() == var.tobytes()


@pytest.mark.parametrize("impl", list(IMPLS))
def test_guide_edge_keeps_the_halves_apart(impl):
    """Means 1 (left half) and 2 (right half) with noise, a guide plane with a unit step between them and
    guide_sigma 1e-3: a tap across the edge weighs 1e-6, so each half stays within its own input range."""
    rng = np.random.default_rng(3)
    H, W, n = 24, 40, 16
    left = np.arange(W)[None, :] < W // 2
    mean = np.where(left, F(1), F(2)) * np.ones((H, 1), np.float32)
    y = mean[..., None] * (F(0.8) + F(0.4) * rng.random((H, W, n), np.float32))
    film = np.zeros((H, W, 4), np.float32)
    film[..., 1] = y.sum(-1, dtype=np.float32)
    film[..., 0], film[..., 2], film[..., 3] = film[..., 1] * F(0.5), film[..., 1] * F(2), n
    m2 = (y * y).sum(-1, dtype=np.float32)
    guide = np.where(left, F(0), F(1)) * np.ones((H, 1), np.float32)
    out, _ = IMPLS[impl](film, m2, [guide], [1e-3], iterations=5)
    cin, cout = film[..., 1] / film[..., 3], out[..., 1] / out[..., 3]
    for half in (left * np.ones((H, 1), bool), ~left * np.ones((H, 1), bool)):
        lo, hi = cin[half].min(), cin[half].max()
        assert cout[half].min() >= lo * (1 - 1e-3) and cout[half].max() <= hi * (1 + 1e-3), (lo, hi)
    assert cout[:, : W // 2].max() < 1.3 and cout[:, W // 2:].min() > 1.6  # (1.2 < 1.6: the halves never met)
    assert cout[:, : W // 2].std() < 0.5 * cin[:, : W // 2].std()  # and each half was smoothed


@pytest.mark.parametrize("impl", list(IMPLS))
def test_zero_variance_film_passes_through(impl):
    """m2 = n * mean^2: the samples of a pixel were all equal, so the film carries no noise; the filter changes it by
    at most 1e-2 relative per pixel (rel_floor alone sets the scale)."""
    film, _, _ = R.hand_made_frame(37, 21, 0, seed=2, nan_invalid=False)
    n = film[..., 3]
    ok = n >= 1
    with np.errstate(all="ignore"):
        mean = film[..., 1] / n
    m2 = np.where(ok, n * (mean * mean), 0).astype(np.float32)
    m2[n == 1] = (mean * mean)[n == 1]
    # (a pixel with one sample claims v = mean^2: give those pixels two, or they are noise by definition)
    film[n == 1] *= F(2)
    m2[n == 1] *= F(2)
    out, var = IMPLS[impl](film, m2, iterations=4)
    rel = np.abs(out[ok][:, :3] - film[ok][:, :3]) / film[ok][:, :3]
    print("zero variance: max relative change", rel.max())
    assert rel.max() <= 1e-2
    assert (out[..., 3] == film[..., 3]).all()


@pytest.mark.parametrize("impl", list(IMPLS))
@pytest.mark.parametrize("n_guides", (0, 2))
def test_output_means_stay_in_the_input_range(impl, n_guides):
    film, m2, guides = R.hand_made_frame(37, 21, n_guides, seed=4)
    out, _ = IMPLS[impl](film, m2, guides, iterations=5)
    ok = film[..., 3] >= 1
    for ch in range(3):
        cin, cout = film[ok][:, ch] / film[ok][:, 3], out[ok][:, ch] / out[ok][:, 3]
        assert cout.min() >= cin.min() * (1 - 1e-6) and cout.max() <= cin.max() * (1 + 1e-6), ch


# ------------------------------------------------------------------------------------------------------ 5. quality

QUALITY_BAR = 0.75  # denoised relative RMSE of Y / W over the noisy film's, against the 1024-wave reference


@functools.lru_cache(maxsize=None)
def oracle_frames(name):
    """(16-wave film, its plane, 1024-wave pool film, [alpha, tau / (1 + tau)] of the host coverage pass) of a 64^3
    stand-in at 48 x 48; computed once, read-only."""
    import alpha_lib as AL
    import oracle_lib as O
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    waves = 16
    wl = workload(name, width=48, height=48, spp=waves, grid_n=64)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
    T = wl.cfg.jobs_per_wave()
    f, rec, _ = O.render_jobs(wl.cfg, od, ot, 0, waves * T, records=True)
    films, m2s = A.accumulate(wl.cfg, A.records_to_samples(wl.cfg, rec, 0, waves))
    assert films[waves].tobytes() == f.tobytes()
    ref, _, _ = O.render_pool(wl.cfg, od, ot, 1024, 16)
    alpha, tau = AL.render(wl.cfg, dens, 1)
    guides = [alpha, (tau / (F(1) + tau)).astype(np.float32)]
    for a in [f, m2s[waves], ref] + guides:
        a.setflags(write=False)
    return f, m2s[waves], ref, guides


@pytest.mark.parametrize("name", ["c3", "c4", "c2"])
def test_quality_on_oracle_frames(name):
    """Defaults, without and with the matte's guides.  Measured ratios (denoised / noisy): see EXPERIMENTS.md §18."""
    film, m2, ref, guides = oracle_frames(name)
    noisy = R.rel_rmse_y(film, ref)
    for label, g in (("no guides", []), ("guides", guides)):
        out, var = R.denoise(film, m2, g)
        den = R.rel_rmse_y(out, ref)
        print(f"{name} {label}: noisy {noisy:.4f} denoised {den:.4f} ratio {den / noisy:.3f}")
        assert den <= QUALITY_BAR * noisy, (label, noisy, den)
        assert np.isfinite(var).all() and (out[..., 3] == film[..., 3]).all()
        host, _ = DL.denoise(film, m2, g)
        assert host.tobytes() == out.tobytes()


# ------------------------------------------------------------------------------------- 6. the stand-alone program

@pytest.mark.parametrize("sanitize", [False, True])
def test_denoise_host_program(tmp_path, sanitize):
    """The stand-alone program filters the four frame sizes with 0, 2 and 4 guides (five iterations, NaN in the
    unrendered pixels) and exits 0 when every rendered pixel is finite and every other is copied.  Once more as an
    AddressSanitizer + UBSan build, run directly as a plain process."""
    import subprocess

    extra = ["-O1", "-g", "-DDENOISE_HOST_MAIN"]
    if sanitize:
        extra += ["-Xarch_host", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    exe = DL.compile_host(tmp_path / ("denoise_host_san" if sanitize else "denoise_host"), extra)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "denoise_host: 0 bad values" in r.stdout
