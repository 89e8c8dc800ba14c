"""The denoiser on the GPU (include/vpt_gpu.h, "Denoise"): the vpt_denoise kernels against the numpy restatement
(tests/denoise_ref.py), BYTE FOR BYTE, on hand-made frames and on production films (uniform, adaptive, with a
temperature grid); side effects and state rules; the command line."""
import ctypes as C
import functools

import numpy as np
import pytest

import adaptive_ref as A
import denoise_ref as R
import oracle_lib as O
from volume_path_tracer_amd import capi, image
from volume_path_tracer_amd.scenes import SCENE_DIR, SynthGrid, workload

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

VPT_E_INVALID, VPT_E_STATE = 1, 6
GRID_N = 64


def _grids(wl):
    return SynthGrid(wl.density_kind, wl.grid_n).grid(), (SynthGrid(2, wl.grid_n).grid() if wl.temperature else None)


def _integrator(wl):
    from volume_path_tracer_amd.render import Integrator

    return Integrator(wl.cfg, *_grids(wl), device=0)


def _sized(w, h, name="c3", waves=1):
    return _integrator(workload(name, width=w, height=h, spp=waves, grid_n=GRID_N))


def _dev(it, a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(it.dev)


def device_denoise(it, film, m2, guides=(), guide_sigma=None, iterations=4, sigma_l=4.0, rel_floor=1e-3, var=True):
    """(out film, var) through the C ABI on NaN-filled outputs (a pixel the kernels skipped stays NaN), and the
    inputs as they are after the call."""
    f, m, gs = _dev(it, film), _dev(it, m2), [_dev(it, g) for g in guides]
    out = torch.full_like(f, float("nan"))
    v = torch.full_like(m, float("nan"))
    torch.cuda.synchronize()
    p = capi.DenoiseParams.make(iterations, len(gs), sigma_l, rel_floor, guide_sigma)
    gp = (C.c_void_p * max(1, len(gs)))(*[g.data_ptr() for g in gs])
    capi.check(capi.lib().vpt_gpu_denoise(it.h, C.byref(p), C.c_void_p(f.data_ptr()), C.c_void_p(m.data_ptr()),
                                          gp if gs else None, C.c_void_p(out.data_ptr()),
                                          C.c_void_p(v.data_ptr()) if var else None, C.c_void_p(it.stream_handle())),
               "vpt_gpu_denoise")
    capi.check(capi.lib().vpt_gpu_sync(it.h), "sync")  # (vpt_gpu_sync covers the filter)
    return out.cpu().numpy(), v.cpu().numpy(), (f.cpu().numpy(), m.cpu().numpy(), [g.cpu().numpy() for g in gs])


def _same(a, b, what):
    a, b = np.ascontiguousarray(a, np.float32).view(np.uint32), np.ascontiguousarray(b, np.float32).view(np.uint32)
    assert a.shape == b.shape and (a == b).all(), f"{what}: {int((a != b).sum())} of {a.size} words differ"


# ------------------------------------------------------------------------------------------------ 6. bit-exact cases

@pytest.mark.parametrize("frame", list(R.FRAMES))
def test_device_equals_restatement(frame):
    W, H, K = R.FRAMES[frame]
    it = _sized(W, H)
    for n_guides in R.GUIDE_COUNTS:
        film, m2, guides = R.hand_made_frame(W, H, n_guides)
        sg = R.GUIDE_SIGMA[:n_guides]
        want, want_v = R.denoise(film, m2, guides, sg, iterations=K)
        got, got_v, (f2, m22, g2) = device_denoise(it, film, m2, guides, sg, iterations=K)
        _same(got, want, f"{frame} G={n_guides}: film")
        _same(got_v, want_v, f"{frame} G={n_guides}: var")
        _same(f2, film, "input film")  # (NaN payloads of the unrendered pixels included)
        _same(m22, m2, "input plane")
        for a, b in zip(g2, guides):
            _same(a, b, "input guide")
    # the variance plane may be omitted: the same film
    got2, v2, _ = device_denoise(it, film, m2, guides, sg, iterations=K, var=False)
    _same(got2, want, "film without a variance plane")
    assert np.isnan(v2).all()


# ----------------------------------------------------------------------------------------------- 7. production films

@functools.lru_cache(maxsize=None)
def _oracle_uniform(name, w, h, waves):
    """(film, plane) after `waves` waves from the oracle's per-sample records; read-only."""
    wl = workload(name, width=w, height=h, spp=waves, grid_n=GRID_N)
    dens, temp = _grids(wl)
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
    T = wl.cfg.jobs_per_wave()
    f, rec, _ = O.render_jobs(wl.cfg, od, ot, 0, waves * T, records=True)
    films, m2s = A.accumulate(wl.cfg, A.records_to_samples(wl.cfg, rec, 0, waves))
    assert films[waves].tobytes() == f.tobytes()
    for a in films + m2s:
        a.setflags(write=False)
    return wl, films, m2s


@pytest.mark.parametrize("name", ["c3", "c4"])
def test_uniform_production_film(name):
    """render_uniform's film is the oracle's and its plane the restatement's; Integrator.denoise with the matte's
    guides is the restatement fed the same planes.  c4: with a temperature grid."""
    from volume_path_tracer_amd.render import matte_guides, render_uniform

    waves = 16
    wl, films, m2s = _oracle_uniform(name, 37, 21, waves)
    it = _integrator(wl)
    film, m2 = render_uniform(it)
    assert film.is_cuda and m2.is_cuda and getattr(it, "_m2", None) is None  # (the attachment was restored)
    _same(film.cpu().numpy(), films[waves], "film vs the oracle")
    _same(m2.cpu().numpy(), m2s[waves], "plane vs the restatement")
    guides = matte_guides(it)
    assert len(guides) == 2 and guides[0].max() > 0.05 and 0 < guides[1].max() < 1
    a, t = it.render_alpha(sub=1, tau=True)
    _same(guides[0], a, "guide 0 is alpha")
    _same(guides[1], t / (np.float32(1) + t), "guide 1 is tau / (1 + tau)")
    want, want_v = R.denoise(films[waves], m2s[waves], guides)
    out, var = it.denoise(film, m2, guides, variance=True)
    assert out.is_cuda and var.is_cuda  # tensors in, tensors out
    _same(out.cpu().numpy(), want, "denoised film")
    _same(var.cpu().numpy(), want_v, "variance plane")
    out_np = it.denoise(films[waves], m2s[waves], guides)  # numpy in, numpy out
    assert isinstance(out_np, np.ndarray)
    _same(out_np, want, "denoised film (numpy)")
    # other parameters through the Python call
    want5, _ = R.denoise(films[waves], m2s[waves], guides[:1], [0.05], iterations=5, sigma_l=2.0, rel_floor=1e-2)
    _same(it.denoise(film, m2, guides[:1], guide_sigma=0.05, iterations=5, sigma_l=2.0, rel_floor=1e-2).cpu().numpy(),
          want5, "five iterations, one guide")
    assert (want != films[waves]).any()
    with pytest.raises(ValueError):
        it.denoise(film, m2, iterations=7)


def test_adaptive_film_with_different_wave_counts():
    """A fused adaptive film whose tiles stopped at 8, 16, 24 and 32 waves (target 0.1, chosen on the oracle)."""
    from volume_path_tracer_amd.render import matte_guides, render_adaptive

    wl, films, m2s = _oracle_uniform("c3", 37, 21, 32)
    e_film, e_m2, e_waves, _ = A.emulate_adaptive(wl.cfg, films, m2s, 0.1, 1e-3, 8, 8, 32)
    it = _integrator(wl)
    film, waves, err, info, m2 = render_adaptive(it, 0.1, min_waves=8, step_waves=8, max_waves=32, fused=True,
                                                 return_moments=True)
    assert waves.min() < waves.max() and (waves == e_waves).all()
    _same(film, e_film, "adaptive film")
    _same(m2, e_m2, "adaptive plane")
    assert len(render_adaptive(it, 0.1, min_waves=8, step_waves=8, max_waves=32, fused=True)) == 4  # (the default)
    guides = matte_guides(it)
    want, want_v = R.denoise(film, m2, guides)
    out, var = it.denoise(film, m2, guides, variance=True)
    _same(out, want, "denoised adaptive film")
    _same(var, want_v, "variance plane")
    assert len(np.unique(out[..., 3])) >= 3  # (the counts of the tiles' own waves pass through)


# ------------------------------------------------------------------------------------------ 8. side effects and state

def _raw(it, p, f, m, gp, out, var):
    return capi.lib().vpt_gpu_denoise(it.h, C.byref(p), C.c_void_p(f), C.c_void_p(m), gp, C.c_void_p(out),
                                      C.c_void_p(var) if var else None, C.c_void_p(it.stream_handle()))


def test_aliased_outputs_are_refused():
    W, H = 37, 21
    it = _sized(W, H)
    film, m2, guides = R.hand_made_frame(W, H, 1)
    f, m, g = _dev(it, film), _dev(it, m2), _dev(it, guides[0])
    out, var = torch.full_like(f, 7.0), torch.full_like(m, 7.0)
    big = torch.full((H * W * 5,), 7.0, dtype=torch.float32, device=it.dev)  # an output film and a plane inside it
    torch.cuda.synchronize()
    p = capi.DenoiseParams.make(4, 1)
    gp = (C.c_void_p * 1)(g.data_ptr())
    L = capi.lib()
    cases = {
        "out is the film": (f.data_ptr(), m.data_ptr(), f.data_ptr(), var.data_ptr()),
        "out overlaps the film's tail": (f.data_ptr(), m.data_ptr(), f.data_ptr() + 16 * (H * W - 1), var.data_ptr()),
        "out is the plane": (f.data_ptr(), out.data_ptr(), out.data_ptr(), var.data_ptr()),
        "out is the guide": (f.data_ptr(), m.data_ptr(), g.data_ptr(), var.data_ptr()),
        "var is the plane": (f.data_ptr(), m.data_ptr(), out.data_ptr(), m.data_ptr()),
        "var is the guide": (f.data_ptr(), m.data_ptr(), out.data_ptr(), g.data_ptr()),
        "var inside the film": (f.data_ptr(), m.data_ptr(), out.data_ptr(), f.data_ptr() + 64),
        "var inside out": (f.data_ptr(), m.data_ptr(), big.data_ptr(), big.data_ptr() + 4 * (H * W * 4 - 1)),
    }
    for what, (pf, pm, po, pv) in cases.items():
        assert _raw(it, p, pf, pm, gp, po, pv) == VPT_E_INVALID, what
        assert b"overlaps" in L.vpt_last_error(), what
    torch.cuda.synchronize()
    assert (out == 7).all() and (var == 7).all() and (big == 7).all()  # a refused call writes nothing
    _same(f.cpu().numpy(), film, "film")
    # adjacent is not aliased: the plane right behind the output film
    assert _raw(it, p, f.data_ptr(), m.data_ptr(), gp, big.data_ptr(), big.data_ptr() + 16 * H * W) == capi.VPT_OK
    capi.check(L.vpt_gpu_sync(it.h), "sync")
    want, want_v = R.denoise(film, m2, guides)
    got = big.cpu().numpy()
    _same(got[: H * W * 4].reshape(H, W, 4), want, "film in the shared buffer")
    _same(got[H * W * 4:].reshape(H, W), want_v, "plane in the shared buffer")


def test_open_feed_refuses_the_filter():
    """While a feed of the context is launched and not closed the call returns VPT_E_STATE and writes nothing; after
    the close it filters."""
    waves = 16
    wl = workload("c3", width=64, height=48, spp=waves, grid_n=GRID_N)
    it = _integrator(wl)
    it.set_tuning(grid_blocks=2)  # 512 lanes: the feed launches once 512 of the 768 jobs are pushed
    it.tile_costs()
    L = capi.lib()
    T = wl.cfg.jobs_per_wave()
    film, m2, _ = R.hand_made_frame(64, 48, 0)
    f, m = _dev(it, film), _dev(it, m2)
    out = torch.full_like(f, float("nan"))
    feed_film = torch.zeros_like(it.film)
    torch.cuda.synchronize()
    s, fd = C.c_void_p(), C.c_void_p()
    capi.check(L.vpt_gpu_stream_create(it.h, C.byref(s)), "stream")
    capi.check(L.vpt_gpu_feed_open(it.h, C.c_void_p(feed_film.data_ptr()), s, 1024, C.byref(fd)), "open")
    jids = np.arange(waves * T, dtype=np.uint64)
    capi.check(L.vpt_gpu_feed_push(fd, jids.ctypes.data_as(C.POINTER(C.c_uint64)), jids.size), "push")  # launched
    p = capi.DenoiseParams.make(4, 0)
    assert _raw(it, p, f.data_ptr(), m.data_ptr(), None, out.data_ptr(), None) == VPT_E_STATE
    assert b"feed" in L.vpt_last_error()
    capi.check(L.vpt_gpu_feed_close(fd), "close")
    capi.check(L.vpt_gpu_feed_destroy(fd), "destroy")
    capi.check(L.vpt_gpu_sync(it.h), "sync after the close")
    capi.check(L.vpt_gpu_stream_destroy(it.h, s), "stream destroy")
    assert torch.isnan(out).all()  # the refused call wrote nothing
    assert _raw(it, p, f.data_ptr(), m.data_ptr(), None, out.data_ptr(), None) == capi.VPT_OK
    capi.check(L.vpt_gpu_sync(it.h), "sync")
    _same(out.cpu().numpy(), R.denoise(film, m2)[0], "after the feed")


def test_scratch_is_reused_across_calls():
    """One context: no guides then four (the scratch grows), six iterations then one (it is reused); each result is
    what a fresh context gives, and the restatement's."""
    W, H = 130, 9
    it = _sized(W, H)
    film, m2, guides = R.hand_made_frame(W, H, 4, seed=11)
    calls = [(0, 6), (4, 2), (0, 1), (4, 6), (1, 3)]
    for G, K in calls:
        sg = R.GUIDE_SIGMA[:G]
        got, got_v, _ = device_denoise(it, film, m2, guides[:G], sg, iterations=K)
        fresh, fresh_v, _ = device_denoise(_sized(W, H), film, m2, guides[:G], sg, iterations=K)
        want, want_v = R.denoise(film, m2, guides[:G], sg, iterations=K)
        _same(got, fresh, f"G={G} K={K}: reused vs fresh")
        _same(got_v, fresh_v, f"G={G} K={K}: var, reused vs fresh")
        _same(got, want, f"G={G} K={K}: vs the restatement")
        _same(got_v, want_v, f"G={G} K={K}: var vs the restatement")


def test_calls_on_two_streams_share_the_scratch_in_order():
    """Every call of a context uses the same packed planes.  Calls issued back to back on two streams, with no
    synchronisation between them, are serialised by the library (an event after a call's last iteration, which the
    next call's stream waits for): each result is the restatement's.  Two different films alternate, so a call that
    read planes another call was writing would show; the same through Integrator.denoise(stream=)."""
    W, H, K = 480, 270, 5
    it = _sized(W, H)
    frames = [R.hand_made_frame(W, H, 2, seed=21), R.hand_made_frame(W, H, 2, seed=22)]
    wants = [R.denoise(f, m, g, iterations=K) for f, m, g in frames]
    assert (wants[0][0] != wants[1][0]).any()
    dev = [(_dev(it, f), _dev(it, m), [_dev(it, x) for x in g]) for f, m, g in frames]
    streams = [torch.cuda.Stream(device=it.dev), torch.cuda.Stream(device=it.dev)]
    rounds = 4
    outs = [(torch.full_like(dev[i % 2][0], float("nan")), torch.full_like(dev[i % 2][1], float("nan")))
            for i in range(2 * rounds)]
    torch.cuda.synchronize()  # (the inputs are ready on every stream)
    p = capi.DenoiseParams.make(K, 2)
    L = capi.lib()
    for i, (o, v) in enumerate(outs):  # frame 0 on stream 0, frame 1 on stream 1, ...: nothing waits in between
        f, m, g = dev[i % 2]
        gp = (C.c_void_p * 2)(g[0].data_ptr(), g[1].data_ptr())
        capi.check(L.vpt_gpu_denoise(it.h, C.byref(p), C.c_void_p(f.data_ptr()), C.c_void_p(m.data_ptr()), gp,
                                     C.c_void_p(o.data_ptr()), C.c_void_p(v.data_ptr()),
                                     C.c_void_p(int(streams[i % 2].cuda_stream))), "vpt_gpu_denoise")
    capi.check(L.vpt_gpu_sync(it.h), "sync")  # (covers both streams)
    for i, (o, v) in enumerate(outs):
        _same(o.cpu().numpy(), wants[i % 2][0], f"call {i}: film")
        _same(v.cpu().numpy(), wants[i % 2][1], f"call {i}: var")
    # the Python call, tensors in and out, alternating streams; then a smaller guide count on the other stream
    res = [it.denoise(*dev[i % 2], iterations=K, stream=streams[i % 2]) for i in range(4)]
    res0 = it.denoise(dev[0][0], dev[0][1], iterations=2, stream=streams[1])
    torch.cuda.synchronize()
    for i, o in enumerate(res):
        _same(o.cpu().numpy(), wants[i % 2][0], f"Integrator.denoise call {i}")
    _same(res0.cpu().numpy(), R.denoise(frames[0][0], frames[0][1], iterations=2)[0], "no guides, other stream")


def test_single_pixel_mode_needs_no_special_case():
    """Only the single pixel holds samples: every other pixel is copied (n = 0), and the single pixel, whose only tap
    is itself, comes back as (xyz / n * w / w) * n: four roundings of 2^-24 away from its input, (1 + u)^4 - 1 < 5 u."""
    from volume_path_tracer_amd.render import render_uniform

    wl = workload("c3", width=37, height=21, spp=8, grid_n=GRID_N)
    wp = wl.cfg.worker_parameters
    wp.single_pixel_enabled = 1
    wp.single_pixel_coord[0], wp.single_pixel_coord[1] = 17, 9
    it = _integrator(wl)
    film, m2 = render_uniform(it)
    fh, mh = film.cpu().numpy(), m2.cpu().numpy()
    only = np.zeros((21, 37), bool)
    only[9, 17] = True
    assert (fh[..., 3][~only] == 0).all() and fh[9, 17, 3] == 8 and fh[9, 17, 1] > 0
    out, var, _ = device_denoise(it, fh, mh)
    want, want_v = R.denoise(fh, mh)
    _same(out, want, "film")
    _same(var, want_v, "var")
    _same(out[~only], fh[~only], "the other pixels")
    np.testing.assert_allclose(out[9, 17], fh[9, 17], rtol=5 * 2.0 ** -24, atol=0)
    assert var[9, 17] >= 0 and (var[~only] == 0).all()


# ----------------------------------------------------------------------------------------------------------- 9. CLI

def test_cli_denoise(tmp_path, capsys):
    from volume_path_tracer_amd.__main__ import main
    from volume_path_tracer_amd.render import Integrator, matte_guides
    from volume_path_tracer_amd.scenes import read_configuration

    # in-process: the test runner's own GPU context (one process on the card)
    scene = str(SCENE_DIR / "wdas_cloud.json")
    base = ["--synthetic", "cloud:64", "--size", "37x21", "--spp", "16"]
    p = {k: str(tmp_path / k) for k in ("dn.png", "raw.png", "film.npy", "m2.npy", "dn.npy", "a.npy", "raw.npy")}
    assert main([scene, p["dn.png"]] + base + ["--denoise", "--film-out", p["film.npy"], "--moments-out", p["m2.npy"],
                                               "--denoised-film-out", p["dn.npy"], "--alpha-out", p["a.npy"]]) == 0
    err = capsys.readouterr().err
    assert "Denoised in" in err and "4 iterations, 2 guides" in err
    film, m2, dn, alpha = (np.load(p[k]) for k in ("film.npy", "m2.npy", "dn.npy", "a.npy"))
    assert film.shape == (21, 37, 4) and m2.shape == (21, 37) and (film[..., 3] == 16).all()
    cfg = read_configuration(SCENE_DIR / "wdas_cloud.json")
    cfg.num_waves = 16
    cfg.output_size[0], cfg.output_size[1] = 37, 21
    it = Integrator(cfg, SynthGrid(1, 64).grid(), None, device=0)
    guides = matte_guides(it, sub=1)
    _same(alpha, guides[0], "the saved matte is the guides' pass")
    want, _ = R.denoise(film, m2, guides)
    _same(dn, want, "saved denoised film vs the restatement of the saved inputs")
    assert (dn != film).any()
    png = image.decode_png((tmp_path / "dn.png").read_bytes())
    assert png.shape == (21, 37, 3) and (png == image.film_to_image(dn)).all()
    # without --denoise: the path and the PNG of before
    assert main([scene, p["raw.png"]] + base + ["--film-out", p["raw.npy"]]) == 0
    assert "Denoised" not in capsys.readouterr().err
    raw = np.load(p["raw.npy"])
    rpng = image.decode_png((tmp_path / "raw.png").read_bytes())
    assert (rpng == image.film_to_image(raw)).all() and (rpng != png).any()
    # --alpha-foreground: the denoised film first, then the environment light removed
    assert main([scene, str(tmp_path / "fg.png")] + base + ["--denoise", "--alpha-foreground", "--denoise-iters", "5",
                                                            "--denoise-sigma", "3"]) == 0
    fg = image.decode_png((tmp_path / "fg.png").read_bytes())
    dn5, _ = R.denoise(film, m2, guides, iterations=5, sigma_l=3.0)
    assert fg.shape == (21, 37, 4)
    assert (fg[..., :3] == image.film_to_image(image.foreground_film(dn5, guides[0], cfg))).all()
    assert (fg[..., 3] == np.rint(np.float32(255.0) * guides[0]).astype(np.uint8)).all()
    # --denoise-no-guides; the outputs need --denoise
    assert main([scene, str(tmp_path / "ng.png")] + base + ["--denoise", "--denoise-no-guides", "--denoised-film-out",
                                                            p["dn.npy"]]) == 0
    assert "0 guides" in capsys.readouterr().err
    _same(np.load(p["dn.npy"]), R.denoise(film, m2)[0], "no guides")
    with pytest.raises(SystemExit):
        main([scene, str(tmp_path / "x.png")] + base + ["--moments-out", p["m2.npy"]])
