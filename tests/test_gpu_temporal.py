"""The temporal pass on the GPU (include/vpt_gpu.h, "Temporal"): vpt_temporal_kernel against the numpy restatement
(tests/temporal_ref.py), BYTE FOR BYTE, on hand-made frames and on production films (uniform, with a temperature grid,
fused adaptive, single-pixel mode), with history of history; side effects and state rules; the command line."""
import ctypes as C

import numpy as np
import pytest

import denoise_ref as DR
import temporal_ref as R
from volume_path_tracer_amd import capi, image, scenes
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, workload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VPT_E_INVALID = 1
GRID_N = 64
LEVELS = (1.0 / 255.0, 0.5)


def _integrator(wl):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(wl.cfg, SynthGrid(wl.density_kind, wl.grid_n).grid(),
                      SynthGrid(2, wl.grid_n).grid() if wl.temperature else None, device=0)


def _dev(it, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(it.dev) if a is not None else None


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _entry(cam):
    e = capi.ShutterCamera()
    e.position[:], e.look[:], e.up[:], e.vfov_deg = cam["position"], cam["look"], cam["up"], cam["vfov_deg"]
    return e


def device_temporal(it, film, m2, depth, prev_cam, history=None, optional=True, **params):
    """(film, m2, motion, hist_n) through the C ABI on NaN-filled outputs (a pixel the kernel skipped stays NaN;
    optional=False: the two optional outputs are not passed and stay NaN), and the inputs as they are after the call."""
    ins = [_dev(it, a) for a in (film, m2, depth)] + [_dev(it, a) for a in (history or (None, None, None))]
    H, W = m2.shape
    outs = [torch.full(s, float("nan"), dtype=torch.float32, device=it.dev) for s in ((H, W, 4), (H, W), (H, W, 2), (H, W))]
    torch.cuda.synchronize()
    kw = dict(R.DEFAULTS, **params)
    p = capi.TemporalParams.make(depth.shape[0], **kw)
    cam = _entry(prev_cam)
    capi.check(capi.lib().vpt_gpu_temporal(it.h, C.byref(p), _ptr(ins[0]), _ptr(ins[1]), _ptr(ins[2]), C.byref(cam),
                                           _ptr(ins[3]), _ptr(ins[4]), _ptr(ins[5]), _ptr(outs[0]), _ptr(outs[1]),
                                           _ptr(outs[2]) if optional else None, _ptr(outs[3]) if optional else None,
                                           C.c_void_p(it.stream_handle())), "vpt_gpu_temporal")
    capi.check(capi.lib().vpt_gpu_sync(it.h), "sync")  # (vpt_gpu_sync covers the pass: no other wait before the copies)
    return [o.cpu().numpy() for o in outs], [None if t is None else t.cpu().numpy() for t in ins]


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
    assert a.shape == b.shape and (a == b).all(), f"{what}: {int((a != b).sum())} of {a.size} words differ"


NAMES = ("film", "plane", "motion", "hist_n")


# ------------------------------------------------------------------------------------------------ 1. bit-exact cases

@pytest.mark.parametrize("frame", list(R.FRAMES))
def test_device_equals_restatement(frame):
    W, H = R.FRAMES[frame]
    it = _integrator(workload("c3", width=W, height=H, spp=1, grid_n=GRID_N))
    it.set_camera(**R.BASE_CAMERA)  # (the current camera is the context's scene camera)
    for K in R.LEVELS:
        for prev, cam in R.previous_cameras().items():
            film, m2, depth, cur, prv, hist = R.hand_made_case(W, H, K, prev)
            want = R.temporal(film, m2, depth, cur, prv, hist)
            got, after = device_temporal(it, film, m2, depth, cam, hist)
            for a, b, n in zip(got, want, NAMES):
                _same(a, b, f"{frame} K={K} {prev}: {n}")
            for a, b in zip(after, (film, m2, depth, *hist)):
                _same(a, b, "an input")  # (NaN payloads of the unrendered pixels included)
    # the optional outputs omitted: the same film and plane; no history: the inputs' bytes and the motion all the same
    got2, _ = device_temporal(it, film, m2, depth, cam, hist, optional=False)
    _same(got2[0], want[0], "film without the optional outputs")
    _same(got2[1], want[1], "plane without the optional outputs")
    assert np.isnan(got2[2]).all() and np.isnan(got2[3]).all()
    got3, _ = device_temporal(it, film, m2, depth, cam, None)
    for a, b, n in zip(got3, R.temporal(film, m2, depth, cur, prv, None), NAMES):
        _same(a, b, f"no history: {n}")
    _same(got3[0], film, "no history: the film's bytes")
    # other parameters
    kw = dict(max_history=5.0, depth_tol=0.02, sigma_r=2.0, rel_floor=1e-2)
    film, m2, depth, cur, prv, hist = R.hand_made_case(W, H, 2, "dolly", seed=7)
    got4, _ = device_temporal(it, film, m2, depth, R.previous_cameras()["dolly"], hist, **kw)
    for a, b, n in zip(got4, R.temporal(film, m2, depth, cur, prv, hist, **kw), NAMES):
        _same(a, b, f"other parameters: {n}")


# ----------------------------------------------------------------------------------------------- 2. production films

def _orbit_frames(it, cfgs):
    """[(film, m2, depth, camera)] of the frames `cfgs` on one context: render_uniform and render_depth, host arrays."""
    from volume_path_tracer_amd.render import render_uniform

    out = []
    for c in cfgs:
        it.set_scene(c)
        film, m2 = render_uniform(it)
        out.append((film.cpu().numpy(), m2.cpu().numpy(), it.render_depth(LEVELS, sub=1), scenes.camera_of(c)))
    return out


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_production_orbit(name):
    """Three frames of a 3-degree-per-frame orbit (seeds seed + k) through render_uniform and render_depth: the device's
    accumulated film equals the restatement's on those inputs, vpt_gpu_denoise on it equals denoise_ref, and the
    second accumulation, whose history is itself accumulated, still equals the restatement.  c4: a temperature grid."""
    from volume_path_tracer_amd.render import TemporalState, render_uniform

    W, H, waves = 37, 21, 16
    wl = workload(name, width=W, height=H, spp=waves, grid_n=GRID_N)
    cfgs = scenes.orbit(wl.cfg, 3, 9.0)
    for k, c in enumerate(cfgs):
        c.seed = (int(wl.cfg.seed) + k) & 0xFFFFFFFF
    it = _integrator(wl)
    frames = _orbit_frames(it, cfgs)
    assert (frames[0][0] != frames[1][0]).any() and (frames[0][2] != frames[1][2]).any()
    floats = [R.camera_floats(cam, W, H) for *_, cam in frames]
    hist, acc_dev = None, None
    state = TemporalState(it)
    for k, (film, m2, depth, cam) in enumerate(frames):
        it.set_scene(cfgs[k])
        prev = frames[k - 1][3] if k else cam
        want = R.temporal(film, m2, depth, floats[k], floats[k - 1] if k else floats[k], hist, max_history=4.0 * waves)
        got = it.temporal(film, m2, depth, prev, hist, motion=True, hist_n=True)  # numpy in, numpy out; the defaults
        assert all(isinstance(a, np.ndarray) for a in got)
        for a, b, n in zip(got, want, NAMES):
            _same(a, b, f"{name} frame {k}: {n}")
        if k:
            fg = R.pick_depth(depth) > 0
            assert fg.any() and (want[3][fg] > 0).mean() > 0.5 and want[3].max() <= 4 * waves  # (it accumulated)
            assert 0.05 < np.nanmax(np.abs(want[2][fg])) < 10.0  # the cloud moved by about a pixel
        else:
            _same(got[0], film, "frame 0: no history, the film's bytes")
        # the same through the state's two buffer sets, tensors in and out
        acc_dev = state.accumulate(it, torch.from_numpy(film).to(it.dev), torch.from_numpy(m2).to(it.dev), depth=depth)
        assert acc_dev[0].is_cuda and len(acc_dev) == 2
        _same(acc_dev[0].cpu().numpy(), want[0], f"{name} frame {k}: TemporalState film")
        _same(acc_dev[1].cpu().numpy(), want[1], f"{name} frame {k}: TemporalState plane")
        hist = (want[0], want[1], depth)
    assert hist[0][..., 3].max() > 2 * waves  # history of history: more than two frames' samples somewhere
    # the accumulated film is an ordinary film: the denoiser takes it
    dn_want, _ = DR.denoise(hist[0], hist[1])
    _same(it.denoise(acc_dev[0], acc_dev[1]).cpu().numpy(), dn_want, "denoised accumulated film")
    state.reset()
    assert state.history is None and state.camera is None


def test_fused_adaptive_film_as_input_and_as_history():
    """Fused adaptive films whose tiles stopped at different wave counts, as the frame and as its history."""
    from volume_path_tracer_amd.render import render_adaptive

    W, H = 37, 21
    wl = workload("c3", width=W, height=H, spp=32, grid_n=GRID_N)
    cfgs = scenes.orbit(wl.cfg, 2, 6.0)
    cfgs[1].seed = int(wl.cfg.seed) + 1
    it = _integrator(wl)
    frames = []
    for c in cfgs:
        it.set_scene(c)
        film, waves, err, info, m2 = render_adaptive(it, 0.1, min_waves=8, step_waves=8, max_waves=32, fused=True,
                                                     return_moments=True)
        assert waves.min() < waves.max()
        frames.append((film, m2, it.render_depth(LEVELS, sub=1), scenes.camera_of(c)))
    (f0, m0, d0, c0), (f1, m1, d1, c1) = frames
    want = R.temporal(f1, m1, d1, R.camera_floats(c1, W, H), R.camera_floats(c0, W, H), (f0, m0, d0))
    got, _ = device_temporal(it, f1, m1, d1, c0, (f0, m0, d0))
    for a, b, n in zip(got, want, NAMES):
        _same(a, b, f"adaptive: {n}")
    assert (want[3] > 0).sum() > 100 and len(np.unique(f1[..., 3])) >= 2


def test_single_pixel_mode_needs_no_special_case():
    """Only the single pixel holds samples and a depth: every other pixel passes through."""
    from volume_path_tracer_amd.render import render_uniform

    W, H = 37, 21
    wl = workload("c3", width=W, height=H, spp=8, grid_n=GRID_N)
    wp = wl.cfg.worker_parameters
    wp.single_pixel_enabled = 1
    wp.single_pixel_coord[0], wp.single_pixel_coord[1] = 17, 9
    it = _integrator(wl)
    film, m2 = (t.cpu().numpy() for t in render_uniform(it))
    depth = it.render_depth(LEVELS, sub=1)
    only = np.zeros((H, W), bool)
    only[9, 17] = True
    assert (film[..., 3][~only] == 0).all() and film[9, 17, 3] == 8 and (depth[:, ~only] == 0).all()
    cam = scenes.camera_of(wl.cfg)
    cur = R.camera_floats(cam, W, H)
    got, _ = device_temporal(it, film, m2, depth, cam, (film, m2, depth))
    want = R.temporal(film, m2, depth, cur, cur, (film, m2, depth))
    for a, b, n in zip(got, want, NAMES):
        _same(a, b, f"single pixel: {n}")
    _same(got[0][~only], film[~only], "the other pixels")
    assert (got[3][~only] == 0).all() and 7.9 < got[3][9, 17] <= 8.0 and 15.9 < got[0][9, 17, 3] <= 16.0


# ------------------------------------------------------------------------------------------ 3. side effects and state

def test_aliased_outputs_are_refused():
    W, H = 37, 21
    it = _integrator(workload("c3", width=W, height=H, spp=1, grid_n=GRID_N))
    it.set_camera(**R.BASE_CAMERA)
    film, m2, depth, cur, prv, hist = R.hand_made_case(W, H, 2, "orbit2")
    f, m, d, hf, hm, hd = (_dev(it, a) for a in (film, m2, depth, *hist))
    out, om = torch.full_like(f, 7.0), torch.full_like(m, 7.0)
    mv, hn = torch.full((H, W, 2), 7.0, device=it.dev), torch.full_like(m, 7.0)
    big = torch.full((H * W * 8,), 7.0, dtype=torch.float32, device=it.dev)
    torch.cuda.synchronize()
    p, cam, L = capi.TemporalParams.make(2), _entry(R.previous_cameras()["orbit2"]), capi.lib()

    def raw(po, pm, pv, pn):
        return L.vpt_gpu_temporal(it.h, C.byref(p), _ptr(f), _ptr(m), _ptr(d), C.byref(cam), _ptr(hf), _ptr(hm), _ptr(hd),
                                  C.c_void_p(po), C.c_void_p(pm), C.c_void_p(pv) if pv else None,
                                  C.c_void_p(pn) if pn else None, C.c_void_p(it.stream_handle()))

    o, q, v, n = out.data_ptr(), om.data_ptr(), mv.data_ptr(), hn.data_ptr()
    cases = {
        "out is the film": (f.data_ptr(), q, v, n), "out is the history": (hf.data_ptr(), q, v, n),
        "out overlaps the film's tail": (f.data_ptr() + 16 * (H * W - 1), q, v, n),
        "plane is the plane": (o, m.data_ptr(), v, n), "plane is the history's": (o, hm.data_ptr(), v, n),
        "plane inside the depth": (o, d.data_ptr() + 4 * H * W, v, n), "plane inside the history's depth": (o, hd.data_ptr(), v, n),
        "plane inside out": (o, o + 64, v, n), "motion is the film": (o, q, f.data_ptr(), n),
        "motion inside out": (o, q, o + 16, n), "hist_n is the plane out": (o, q, v, q),
        "hist_n inside the motion": (o, q, v, v + 4 * H * W), "hist_n is the history's plane": (o, q, None, hm.data_ptr()),
    }
    for what, ptrs in cases.items():
        assert raw(*ptrs) == VPT_E_INVALID, what
        assert b"overlaps" in L.vpt_last_error(), what
    torch.cuda.synchronize()
    assert all((t == 7).all() for t in (out, om, mv, hn, big))  # a refused call writes nothing
    _same(f.cpu().numpy(), film, "film")
    # adjacent is not aliased: the four outputs back to back in one buffer
    b0 = big.data_ptr()
    assert raw(b0, b0 + 16 * H * W, b0 + 20 * H * W, b0 + 28 * H * W) == capi.VPT_OK
    capi.check(L.vpt_gpu_sync(it.h), "sync")
    want = R.temporal(film, m2, depth, cur, prv, hist)
    got = big.cpu().numpy()
    N = H * W
    for a, b, n_ in zip((got[:4 * N], got[4 * N:5 * N], got[5 * N:7 * N], got[7 * N:]), want, NAMES):
        _same(a.reshape(b.shape), b, f"{n_} in the shared buffer")


# ----------------------------------------------------------------------------------------------------------- 4. CLI

def test_cli_temporal(tmp_path, capsys):
    from volume_path_tracer_amd.__main__ import main
    from volume_path_tracer_amd.scenes import read_configuration

    scene = str(SCENE_DIR / "wdas_cloud.json")
    base = ["--synthetic", "cloud:64", "--size", "37x21", "--spp", "16", "--frames", "3", "--orbit", "9"]
    t = lambda n: str(tmp_path / n)  # noqa: E731
    assert main([scene, t("t_%d.png")] + base + ["--temporal", "--denoise", "--denoise-no-guides", "--film-out", t("tf_%d.npy"),
                                                  "--accumulated-film-out", t("acc_%d.npy"), "--motion-out", t("mv_%d.npy"),
                                                  "--denoised-film-out", t("dn_%d.npy"), "--depth-out", t("z_%d.npy"),
                                                  "--moments-out", t("tm_%d.npy")]) == 0
    err = capsys.readouterr().err
    assert err.count("Accumulated in") == 3 and "history adds 0.00 x" in err
    for k in range(3):
        for n in ("t_%d.png", "tf_%d.npy", "acc_%d.npy", "mv_%d.npy", "dn_%d.npy", "z_%d.npy"):
            assert (tmp_path / (n % k)).exists(), (n, k)
    # the same sequence without --temporal (one seed for every frame, as before)
    assert main([scene, t("p_%d.png")] + base + ["--denoise", "--denoise-no-guides", "--film-out", t("pf_%d.npy"),
                                                  "--denoised-film-out", t("pd_%d.npy"), "--moments-out", t("pm_%d.npy")]) == 0
    assert "Accumulated" not in capsys.readouterr().err
    # frame 0 has no history: every file of it equals the run without --temporal
    for a, b in (("t_0.png", "p_0.png"), ("tf_0.npy", "pf_0.npy"), ("dn_0.npy", "pd_0.npy"), ("tm_0.npy", "pm_0.npy")):
        assert (tmp_path / a).read_bytes() == (tmp_path / b).read_bytes(), (a, b)
    _same(np.load(t("acc_0.npy")), np.load(t("tf_0.npy")), "frame 0: the accumulated film is the raw film")
    # later frames: independent seeds, and the saved accumulated film is the restatement of the saved inputs
    f1, f2 = np.load(t("tf_1.npy")), np.load(t("pf_1.npy"))
    assert (f1 != f2).any() and (f1[..., 3] == 16).all()
    cfg = read_configuration(SCENE_DIR / "wdas_cloud.json")
    cfg.output_size[0], cfg.output_size[1] = 37, 21
    cams = [scenes.camera_of(c) for c in scenes.orbit(cfg, 3, 9.0)]
    acc = [np.load(t("acc_%d.npy") % k) for k in range(3)]
    assert acc[2][..., 3].max() > 32 and (acc[1][..., 3] >= 16).all()
    mv = np.load(t("mv_1.npy"))
    assert mv.shape == (21, 37, 2) and 0.1 < np.nanmax(np.abs(mv)) < 8
    dn = np.load(t("dn_2.npy"))
    _same(dn, DR.denoise(acc[2], np.load(t("tm_2.npy")))[0], "frame 2: the denoiser ran on the accumulated film and plane")
    png = image.decode_png((tmp_path / "t_2.png").read_bytes())
    assert (png == image.film_to_image(dn)).all()
    assert len(cams) == 3
    # without --denoise the PNG shows the accumulated film
    assert main([scene, t("a_%d.png")] + base + ["--temporal", "--accumulated-film-out", t("a_%d.npy"),
                                                  "--temporal-history", "8", "--temporal-depth-tol", "0.05",
                                                  "--temporal-sigma", "2"]) == 0
    a2 = np.load(t("a_2.npy"))
    assert a2[..., 3].max() <= 16 + 8 and (image.decode_png((tmp_path / "a_2.png").read_bytes()) == image.film_to_image(a2)).all()


@pytest.mark.parametrize("extra, why", [
    (["--temporal"], "needs --frames or --camera-path"),
    (["--temporal", "--frames", "2", "--shutter", "0.5"], "shutter"),
    (["--temporal", "--shutter-camera", "cam.json"], "needs --frames"),
    (["--temporal", "--frames", "2", "--volume-sequence", "v_%d.npz"], "volume-sequence"),
    (["--temporal", "--frames", "2", "--light-groups"], "light-groups"),
    (["--temporal", "--frames", "2", "--relight", "sun=2"], "light-groups"),
    (["--temporal", "--frames", "2", "--rng-mode", "pixel"], "rng-mode pixel"),
    (["--frames", "2", "--temporal-history", "8"], "--temporal-history needs --temporal"),
    (["--frames", "2", "--temporal-depth-tol", "0.1"], "--temporal-depth-tol needs --temporal"),
    (["--frames", "2", "--temporal-sigma", "4"], "--temporal-sigma needs --temporal"),
    (["--frames", "2", "--motion-out", "mv_%d.npy"], "--motion-out needs --temporal"),
    (["--frames", "2", "--accumulated-film-out", "acc_%d.npy"], "--accumulated-film-out needs --temporal"),
    (["--temporal", "--frames", "2", "--motion-out", "mv.npy"], "--motion-out 'mv.npy'"),
    (["--temporal", "--frames", "2", "--accumulated-film-out", "acc.npy"], "--accumulated-film-out 'acc.npy'"),
    (["--temporal", "--frames", "2", "--temporal-history", "0"], "--temporal-history wants a number > 0"),
])
def test_cli_refusals_exit_1(tmp_path, capsys, extra, why):
    """Each refusal exits 1 with one line saying why, before a device is touched (the scene file is not even read)."""
    from volume_path_tracer_amd.__main__ import main

    assert main([str(tmp_path / "no_such_scene.json"), str(tmp_path / "o_%d.png")] + extra) == 1
    err = capsys.readouterr().err
    assert "FATAL" in err and why in err and "no_such_scene" not in err, err
