"""The quality harness of the temporal pass on the CPU (tests/test_temporal_host.py and EXPERIMENTS.md §27): frames of an
orbit rendered by the unchanged oracle (64^3 stand-ins, 48 x 48, 16 waves, frame k with seed + k), their moment planes
from the per-sample records, their depth planes and guides from the host builds of the depth and coverage passes, the
host build of the temporal pass over them, and relative RMSE of Y / W against the oracle's 1024-wave frame.

    python tests/temporal_quality.py        prints the measurements and the depth_tol x sigma_r sweep of §27
"""
import functools
import sys
from pathlib import Path

import numpy as np

if __name__ == "__main__":  # (the tests' conftest puts the repository on the path; a direct run does it here)
    sys.path[:0] = [str(Path(__file__).resolve().parents[1])]

import adaptive_ref as A
import denoise_ref as DR
import temporal_lib as TL
import temporal_ref as R

WAVES, SIZE, GRID_N, FRAMES, ORBIT_FRAMES = 16, 48, 64, 4, 120  # frames 0..3 of scenes.orbit(cfg, 120): 3 degrees each
LEVELS = (1.0 / 255.0, 0.5)
REF_WAVES, REF_SEED_OFFSET = 1024, 1000  # the reference frame's samples are independent of every test frame's


def _seeded(cfg, k):
    c = cfg.copy()
    c.seed = (int(cfg.seed) + k) & 0xFFFFFFFF
    return c


@functools.lru_cache(maxsize=None)
def scene(name):
    """-> dict: "orbit": frames 0..3 as (film, m2, depth, cam16); "static": four frames of frame 3's camera with seeds
    seed + 0..3, the last one being the orbit's frame 3; "ref": the 1024-wave film of frame 3's camera; "guides": frame
    3's [alpha, tau / (1 + tau)].  Computed once, read-only."""
    import alpha_lib as AL
    import depth_lib as DL
    import oracle_lib as O
    from volume_path_tracer_amd import scenes
    from volume_path_tracer_amd.scenes import SynthGrid, workload

    wl = workload(name, width=SIZE, height=SIZE, spp=WAVES, grid_n=GRID_N)
    dens = SynthGrid(wl.density_kind, wl.grid_n).grid()
    temp = SynthGrid(2, wl.grid_n).grid() if wl.temperature else None
    od = O.OracleGrid(dens, fix_majorants=True)
    ot = O.OracleGrid(temp, fix_majorants=False) if temp is not None else None
    T = wl.cfg.jobs_per_wave()

    def frame(cfg):
        f, rec, _ = O.render_jobs(cfg, od, ot, 0, WAVES * T, records=True)
        films, m2s = A.accumulate(cfg, A.records_to_samples(cfg, rec, 0, WAVES))
        assert films[WAVES].tobytes() == f.tobytes()
        depth, _ = DL.render(cfg, dens, LEVELS, sub=1)
        return f, m2s[WAVES], depth, R.camera_floats(scenes.camera_of(cfg), SIZE, SIZE)

    cams = scenes.orbit(wl.cfg, ORBIT_FRAMES)[:FRAMES]
    orbit = [frame(_seeded(c, k)) for k, c in enumerate(cams)]
    static = [frame(_seeded(cams[-1], k)) for k in range(FRAMES - 1)] + [orbit[-1]]
    ref, _, _ = O.render_pool(_seeded(cams[-1], REF_SEED_OFFSET), od, ot, REF_WAVES, 16)
    alpha, tau = AL.render(cams[-1], dens, 1)
    out = {"orbit": orbit, "static": static, "ref": ref,
           "guides": [alpha, (tau / (np.float32(1) + tau)).astype(np.float32)]}
    for fr in orbit + static:
        for a in fr:
            a.setflags(write=False)
    ref.setflags(write=False)
    return out


def accumulate(frames, **params):
    """The host build over the frames in turn, each frame's history the previous output -> the last (film, m2)."""
    hist, prev16 = None, None
    for film, m2, depth, cam16 in frames:
        kw = dict(max_history=4.0 * WAVES)
        kw.update(params)
        out, om2, _, _ = TL.temporal(film, m2, depth, cam16, cam16 if prev16 is None else prev16, hist, **kw)
        hist, prev16 = (out, om2, depth), cam16
    return hist[0], hist[1]


def measure(name, **params):
    """-> dict of relative RMSEs against the reference: raw (frame 3), acc (orbit, accumulated), static_one / static_acc,
    denoised (frame 3, spatial only), acc_denoised, and ratio = acc_denoised / denoised."""
    s = scene(name)
    ref, guides = s["ref"], s["guides"]
    film3, m23 = s["orbit"][-1][0], s["orbit"][-1][1]
    acc, acc_m2 = accumulate(s["orbit"], **params)
    st, _ = accumulate(s["static"], **params)
    r = {"raw": DR.rel_rmse_y(film3, ref), "acc": DR.rel_rmse_y(acc, ref),
         "static_one": DR.rel_rmse_y(s["static"][-1][0], ref), "static_acc": DR.rel_rmse_y(st, ref),
         "denoised": DR.rel_rmse_y(DR.denoise(film3, m23, guides)[0], ref),
         "acc_denoised": DR.rel_rmse_y(DR.denoise(acc, acc_m2, guides)[0], ref),
         "mean_count": float(acc[..., 3].mean())}
    r["ratio"] = r["acc_denoised"] / r["denoised"]
    return r


if __name__ == "__main__":
    import time

    for name in ("c3", "c4"):
        t0 = time.time()
        r = measure(name)
        print(name, " ".join(f"{k} {v:.4f}" for k, v in r.items()), f"({time.time() - t0:.1f} s)")
    for name in ("c3", "c4"):
        print(f"{name}: ratio acc_denoised / denoised (acc / raw) by depth_tol (rows) and sigma_r (columns 2, 4, 8)")
        for tol in (0.02, 0.05, 0.1, 0.2):
            row = [measure(name, depth_tol=tol, sigma_r=sr) for sr in (2.0, 4.0, 8.0)]
            print(f"  {tol:5.2f} " + "  ".join(f"{r['ratio']:.3f} ({r['acc'] / r['raw']:.3f})" for r in row))
