"""What the temporal pass costs and what it buys -- the measurements of EXPERIMENTS.md §27.

  python tools/temporal_ab.py [--config c3] [--reps 5] [--size WxH] [--spp 256] [--low-spp 64] [--frames 8]
                              [--degrees 3] [--ref-spp 1024] [--no-quality]

Cost.  Times vpt_gpu_temporal (the C-ABI call on caller-owned buffers, so no allocation or read-back is inside a timing;
two depth levels, a full history, both optional outputs) with HIP events on the context's stream, `reps` times after a
warm-up call, interleaved rep by rep with vpt_gpu_render_depth (the reprojection's two levels, one sub-ray),
vpt_gpu_denoise (four iterations, the matte's two guides), the uniform frame at --low-spp and the uniform frame at
--spp, so all share the session's clocks.  Reports best and worst of the repetitions (measuring-on-mi355x: warm up,
repeat, report the spread) and the pass's ratio to its byte floor: the current film, plane and depth planes read once,
the history the same, the film and plane written (2 x (16 + 4 + 4 K) + 20 bytes per pixel) at the 8 TB/s of HBM.

Quality.  An orbit of --frames frames, --degrees per frame, frame k with seed + k at --low-spp, accumulated by
render.TemporalState; the last frame's accumulated + denoised film, its spatially denoised film and the raw --spp frame
of the same camera, each as relative RMSE of Y / W against an independent --ref-spp frame.  Prints one JSON line last.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))
HBM_BYTES_PER_MS = 8.0e9  # 8 TB/s


def stats(v):
    return {"best_ms": round(min(v), 4), "worst_ms": round(max(v), 4), "runs_ms": [round(x, 4) for x in v]}


def rel_rmse_y(film, ref):
    import numpy as np

    with np.errstate(all="ignore"):
        a = film[..., 1].astype(np.float64) / film[..., 3]
        b = ref[..., 1].astype(np.float64) / ref[..., 3]
    ok = np.isfinite(a) & np.isfinite(b)
    return float(np.sqrt(np.mean((a[ok] - b[ok]) ** 2)) / np.mean(b[ok]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--spp", type=int, default=256)
    ap.add_argument("--low-spp", type=int, default=64)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--degrees", type=float, default=3.0, help="orbit per frame")
    ap.add_argument("--ref-spp", type=int, default=1024)
    ap.add_argument("--no-quality", action="store_true")
    args = ap.parse_args()

    import numpy as np
    import torch

    from volume_path_tracer_amd import capi, scenes
    from volume_path_tracer_amd.render import (TEMPORAL_DEPTH_LEVELS, Integrator, TemporalState, matte_guides,
                                               render_uniform)
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    kw = {}
    if args.size:
        kw["width"], kw["height"] = (int(v) for v in args.size.lower().split("x"))
    wl = workload(args.config, spp=args.low_spp, **kw)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    n = args.frames
    if n < 2:
        sys.exit("--frames: at least two (a frame and its history)")
    cfgs = scenes.orbit(wl.cfg, n, args.degrees * n)
    for k, c in enumerate(cfgs):
        c.seed = (int(wl.cfg.seed) + k) & 0xFFFFFFFF
    it = Integrator(cfgs[0], dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    L = capi.lib()
    H, W = wl.cfg.height, wl.cfg.width
    s = C.c_void_p(it.stream_handle())
    out = {"config": args.config, "size": [W, H], "grid_n": wl.grid_n, "reps": args.reps, "spp": args.spp,
           "low_spp": args.low_spp, "frames": n, "degrees_per_frame": args.degrees}

    # ---- quality (and the buffers the cost part times on: the last two frames of the orbit)
    state = TemporalState(it)
    acc = None
    for k, c in enumerate(cfgs):
        if k:
            it.set_scene(c)
        film, m2 = render_uniform(it)
        prev = None if state.history is None else dict(state.sets[state.history])
        prev_cam = state.camera
        depth = torch.from_numpy(it.render_depth(TEMPORAL_DEPTH_LEVELS, sub=1)).to(it.dev)
        acc = state.accumulate(it, film, m2, depth=depth, hist_n=True)
    torch.cuda.synchronize()
    last = cfgs[-1]
    if not args.no_quality:
        guides = matte_guides(it, sub=1)
        dn_acc = it.denoise(acc[0], acc[1], guides).cpu().numpy()
        dn_one = it.denoise(film, m2, guides).cpu().numpy()
        hi = last.copy()
        hi.num_waves, hi.seed = args.spp, (int(wl.cfg.seed) + 5000) & 0xFFFFFFFF
        it.set_scene(hi)
        raw_hi, m2_hi = (t.cpu().numpy() for t in render_uniform(it))
        dn_hi = it.denoise(raw_hi, m2_hi, guides)
        ref = last.copy()
        ref.num_waves, ref.seed = args.ref_spp, (int(wl.cfg.seed) + 9000) & 0xFFFFFFFF
        it.set_scene(ref)
        ref_film = render_uniform(it, moments=False).cpu().numpy()
        it.set_scene(last)
        q = {"raw_low": rel_rmse_y(film.cpu().numpy(), ref_film), "accumulated": rel_rmse_y(acc[0].cpu().numpy(), ref_film),
             "denoised_low": rel_rmse_y(dn_one, ref_film), "accumulated_denoised": rel_rmse_y(dn_acc, ref_film),
             "raw_high": rel_rmse_y(raw_hi, ref_film), "denoised_high": rel_rmse_y(dn_hi, ref_film),
             "mean_history_count": float(acc[2].mean()), "mean_count": float(acc[0][..., 3].mean())}
        q["ratio_to_denoised_low"] = q["accumulated_denoised"] / q["denoised_low"]
        out["quality"] = {k: round(v, 5) for k, v in q.items()}

    # ---- cost: frame n - 1 onto frame n - 2's history, as the sequence ran it
    K = len(TEMPORAL_DEPTH_LEVELS)
    op = np.ascontiguousarray(TEMPORAL_DEPTH_LEVELS, np.float32)
    p = capi.TemporalParams.make(K, 4.0 * args.low_spp)
    cam = scenes.shutter_entries(last, [prev_cam])
    o_film, o_m2 = torch.empty_like(film), torch.empty_like(m2)
    o_mv = torch.empty((H, W, 2), dtype=torch.float32, device=it.dev)
    o_hn = torch.empty_like(m2)
    d_out = torch.zeros_like(depth)
    dn_out = torch.empty_like(film)
    g_dev = [torch.from_numpy(g).to(it.dev) for g in matte_guides(it, sub=1)]
    gp = (C.c_void_p * 2)(*[g.data_ptr() for g in g_dev])
    dp = capi.DenoiseParams.make(4, 2)
    scratch = torch.zeros_like(it.film)
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame(spp):
        def run():
            scratch.zero_()
            it.render_jobs(0, spp * it.jobs_per_wave, film=scratch)
        return run

    def planes():
        capi.check(L.vpt_gpu_render_depth(it.h, 1, K, op.ctypes.data_as(C.POINTER(C.c_float)), ptr(d_out), None, s),
                   "vpt_gpu_render_depth")

    def filt():
        capi.check(L.vpt_gpu_denoise(it.h, C.byref(dp), ptr(acc[0]), ptr(acc[1]), gp, ptr(dn_out), None, s), "vpt_gpu_denoise")

    def temporal():
        capi.check(L.vpt_gpu_temporal(it.h, C.byref(p), ptr(film), ptr(m2), ptr(depth), cam, ptr(prev["film"]),
                                      ptr(prev["m2"]), ptr(prev["depth"]), ptr(o_film), ptr(o_m2), ptr(o_mv), ptr(o_hn), s),
                   "vpt_gpu_temporal")

    hi_cfg = last.copy()
    hi_cfg.num_waves = args.spp
    it.set_scene(hi_cfg)  # (job space for the larger frame; the camera is the last frame's)
    names = ("frame_low", "frame_high", "depth", "denoise", "temporal")
    fns = (frame(args.low_spp), frame(args.spp), planes, filt, temporal)
    runs = {k: [] for k in names}
    for rep in range(args.reps + 1):  # (rep 0 warms up: the frame's first call sizes the sample buffer)
        for name, fn in zip(names, fns):
            ms = timed(fn)
            if rep:
                runs[name].append(ms)
    for name in names:
        out[name] = stats(runs[name])
    _same = torch.equal(o_film, acc[0]) and torch.equal(o_m2, acc[1])
    out["timed_call_equals_the_sequence's"] = bool(_same)
    floor_bytes = W * H * (2 * (16 + 4 + 4 * K) + 20)
    out["temporal"]["bytes_per_pixel_floor"] = 2 * (16 + 4 + 4 * K) + 20
    out["temporal"]["floor_ms"] = round(floor_bytes / HBM_BYTES_PER_MS, 4)
    out["temporal"]["over_floor"] = round(out["temporal"]["best_ms"] / (floor_bytes / HBM_BYTES_PER_MS), 2)
    for other in ("depth", "denoise", "frame_low", "frame_high"):
        out["temporal"]["of_" + other] = round(out["temporal"]["best_ms"] / out[other]["best_ms"], 5)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
