"""What the denoiser costs and buys beside a frame -- the measurements of EXPERIMENTS.md §18.

  python tools/denoise_ab.py [--config c3] [--reps 5] [--size WxH] [--spp N] [--grid-n N] [--no-quality] [--no-adaptive]
                             [--targets a,b,..] [--min-waves N] [--step-waves N]

Timing.  vpt_gpu_denoise (the C-ABI call on caller-owned tensors, so no allocation or read-back is inside a timing;
the context's scratch is sized by the warm-up call) at 4 and 5 iterations without guides and with the matte's two,
with HIP events on the context's stream, `reps` times after a warm-up, interleaved rep by rep with the config's
uniform frame (render_jobs of all its waves) and a one-sub-ray coverage pass, so all share the session's clocks.
Reports best and worst of the repetitions (measuring-on-mi355x: warm up, repeat, report the spread), the time against
the algorithm's byte floor (per iteration one packed read and one packed write per pixel: 32 B, 48 B with guides, at
8 TB/s) and as a share of the frame.

Quality.  One ordered render with a moment plane, stopped at 16, 64 and 256 waves, against an independent 1024-wave
frame of the same session (waves 1025..2048): relative RMSE of Y / W of the raw and of the denoised film (defaults,
without and with guides).

What it buys.  vpt_gpu_render_adaptive_fused (--min-waves, --step-waves, cap `spp` waves) at a ladder of targets: frame
time, rendered share, and the denoised film's error, beside the uniform frame's raw error at `spp` waves and the time
and errors of a uniform frame of --min-waves waves.

Prints one JSON line last.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

HBM_BYTES_PER_S = 8e12


def stats(v):
    return {"best_ms": round(min(v), 3), "worst_ms": round(max(v), 3), "runs_ms": [round(x, 3) for x in v]}


def rel_rmse_y(film, ref):
    import numpy as np

    a = film[..., 1].astype(np.float64) / film[..., 3]
    b = ref[..., 1].astype(np.float64) / ref[..., 3]
    return float(np.sqrt(np.mean((a - b) ** 2)) / np.mean(b))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--config", default="c3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--size", default=None, help="WxH (default: the config's)")
    ap.add_argument("--spp", type=int, default=None, help="the uniform frame's waves (default: the config's)")
    ap.add_argument("--grid-n", type=int, default=None)
    ap.add_argument("--no-quality", action="store_true")
    ap.add_argument("--no-adaptive", action="store_true")
    ap.add_argument("--targets", default="0.05,0.1,0.15,0.2,0.3,0.5")
    ap.add_argument("--min-waves", type=int, default=64, help="adaptive: waves of the first group")
    ap.add_argument("--step-waves", type=int, default=64,
                    help="adaptive: waves per later group (the one-launch driver wants a multiple of 64)")
    args = ap.parse_args()

    import numpy as np
    import torch

    from volume_path_tracer_amd import capi
    from volume_path_tracer_amd.render import Integrator, matte_guides
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    kw = {}
    if args.size:
        kw["width"], kw["height"] = (int(v) for v in args.size.lower().split("x"))
    if args.spp:
        kw["spp"] = args.spp
    if args.grid_n:
        kw["grid_n"] = args.grid_n
    wl = workload(args.config, **kw)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    it = Integrator(wl.cfg, dens, temp, device=0)
    it.tile_costs()  # (the cost pass, outside every timing)
    L = capi.lib()
    H, W = wl.cfg.height, wl.cfg.width
    T = it.jobs_per_wave
    s = C.c_void_p(it.stream_handle())
    film = torch.zeros_like(it.film)
    m2 = torch.zeros((H, W), dtype=torch.float32, device=it.dev)
    alpha, tau = torch.zeros_like(m2), torch.zeros_like(m2)
    out_film, var = torch.empty_like(film), torch.empty_like(m2)
    guides_np = matte_guides(it, sub=1)
    guides = [torch.from_numpy(g).to(it.dev) for g in guides_np]
    gp = (C.c_void_p * 2)(*[g.data_ptr() for g in guides])

    def timed(fn):
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    def frame():
        it.render_jobs(0, wl.spp * T, film=film)

    def clear():  # (outside every timing: timed() synchronises before its first event)
        film.zero_()
        m2.zero_()

    def matte():
        capi.check(L.vpt_gpu_render_alpha(it.h, 1, C.c_void_p(alpha.data_ptr()), C.c_void_p(tau.data_ptr()), s), "alpha")

    def denoise(K, G, src=None, plane=None):
        p = capi.DenoiseParams.make(K, G)
        capi.check(L.vpt_gpu_denoise(it.h, C.byref(p), C.c_void_p((film if src is None else src).data_ptr()),
                                     C.c_void_p((m2 if plane is None else plane).data_ptr()), gp if G else None,
                                     C.c_void_p(out_film.data_ptr()), C.c_void_p(var.data_ptr()), s), "vpt_gpu_denoise")

    variants = [(4, 0), (5, 0), (4, 2), (5, 2)]
    out = {"config": args.config, "size": [W, H], "spp": wl.spp, "grid_n": wl.grid_n, "reps": args.reps, "frame": [],
           "alpha_sub1": [], "denoise": {f"K{K}_G{G}": [] for K, G in variants}}
    it.set_film_moments(m2)  # (the frame keeps its plane, as render_uniform's does)
    for rep in range(args.reps + 1):  # (rep 0 warms up: the frame's first call sizes the sample buffer, the filter's the scratch)
        clear()
        ms = timed(frame)
        if rep:
            out["frame"].append(ms)
        ms = timed(matte)
        if rep:
            out["alpha_sub1"].append(ms)
        for K, G in (variants[::-1] if rep == 0 else variants):  # (warm-up: the largest scratch first)
            ms = timed(lambda: denoise(K, G))
            if rep:
                out["denoise"][f"K{K}_G{G}"].append(ms)
    out["frame"], out["alpha_sub1"] = stats(out["frame"]), stats(out["alpha_sub1"])
    for K, G in variants:
        d = stats(out["denoise"][f"K{K}_G{G}"])
        # prepare (film 16 + plane 4 + G guides 4 each in, packed 16 (+16) out), K iterations, the last one's film read
        floor_iter = K * (48 if G else 32) * H * W / HBM_BYTES_PER_S * 1e3
        d["floor_ms_iterations"] = round(floor_iter, 4)
        d["over_floor"] = round(d["best_ms"] / floor_iter, 2)
        d["of_frame"] = round(d["best_ms"] / out["frame"]["best_ms"], 5)
        out["denoise"][f"K{K}_G{G}"] = d

    def errors(f, m, ref):
        row = {"raw": rel_rmse_y(f.cpu().numpy(), ref)}
        for label, G in (("denoised", 0), ("denoised_guides", 2)):
            denoise(4, G, f, m)
            torch.cuda.synchronize()
            row[label] = rel_rmse_y(out_film.cpu().numpy(), ref)
            row[label + "_ratio"] = round(row[label] / row["raw"], 4)
        return {k: round(v, 5) for k, v in row.items()}

    ref = None
    if not args.no_quality or not args.no_adaptive:
        it.set_film_moments(None)
        rf = torch.zeros_like(film)
        it.render_waves(1025, 1024, film=rf)  # an independent reference: other job ids, other random streams
        torch.cuda.synchronize()
        ref = rf.cpu().numpy()
        del rf
    if not args.no_quality:
        film.zero_()
        m2.zero_()
        it.set_film_moments(m2)
        out["quality"] = {}
        done = 0
        for n in (16, 64, 256):
            it.render_waves(done + 1, n - done, film=film)
            done = n
            torch.cuda.synchronize()
            out["quality"][str(n)] = errors(film, m2, ref)
        it.set_film_moments(None)
    if not args.no_adaptive:
        film.zero_()
        m2.zero_()
        it.set_film_moments(m2)
        it.render_waves(1, wl.spp, film=film)
        torch.cuda.synchronize()
        it.set_film_moments(None)
        out["uniform_raw_error"] = round(rel_rmse_y(film.cpu().numpy(), ref), 5)
        mn = min(args.min_waves, wl.spp)
        it.set_film_moments(m2)
        short = []
        for _ in range(3):  # (a uniform frame of the first group's waves alone; the first run warms up)
            film.zero_()
            m2.zero_()
            short.append(timed(lambda: it.render_jobs(0, mn * T, film=film)))
        it.set_film_moments(None)
        out["uniform_min_waves"] = {"waves": mn, "frame_ms": round(min(short[1:]), 2), **errors(film, m2, ref)}
        out["adaptive_fused"] = []
        wv, er = np.zeros(T, np.uint32), np.zeros(T, np.float32)
        for target in [float(v) for v in args.targets.split(",")]:
            p = capi.AdaptiveParams(target, 1e-3, mn, args.step_waves, wl.spp)
            res = capi.AdaptiveResult()
            best = None
            for _ in range(2):  # (the second run is warm)
                film.zero_()
                m2.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                capi.check(L.vpt_gpu_render_adaptive_fused(it.h, C.byref(p), C.c_void_p(film.data_ptr()),
                                                           C.c_void_p(m2.data_ptr()),
                                                           wv.ctypes.data_as(C.POINTER(C.c_uint32)),
                                                           er.ctypes.data_as(C.POINTER(C.c_float)), C.byref(res), s),
                           "vpt_gpu_render_adaptive_fused")
                best = (time.perf_counter() - t0) * 1e3
            info = res.as_dict()
            row = {"target": target, "frame_ms": round(best, 2),
                   "jobs_share": round(info["jobs_rendered"] / info["jobs_uniform"], 4)}
            row.update(errors(film, m2, ref))
            out["adaptive_fused"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
