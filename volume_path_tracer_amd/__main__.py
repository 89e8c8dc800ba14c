"""Headless renderer: ``python -m volume_path_tracer_amd config_path output_path``.

The reference's main (src/main.cpp:26-146) without the raylib window: read the scene, load the
volume (relative to the scene file), render every wave on the GPU through the drop-in integrator,
convert the film to 8-bit sRGB (film_to_image) and save a PNG.

``--synthetic cloud|constant|fire[:N]`` replaces the volume file by a generated stand-in (the
reference's volumes are not shipped).  ``--spp`` overrides num_waves; ``--size WxH`` overrides
output_size.  ``--adaptive ERR`` renders until every tile's error estimate is at most ERR
(render.render_adaptive): ``--spp`` becomes the cap, ``--min-spp`` / ``--spp-step`` the first round and
the later rounds' waves, ``--waves-out`` saves the per-tile wave map, ``--adaptive-fused`` runs the
one-launch driver (the same bytes).  ``--alpha`` writes an RGBA PNG: the same RGB bytes plus the coverage
matte (Integrator.render_alpha) as A = round(255 * alpha); ``--alpha-foreground`` (implies ``--alpha``) first
removes the environment light seen through the medium (image.foreground_film; straight alpha);
``--alpha-sub N`` sets the matte's sub-rays per axis, ``--alpha-out`` saves the alpha plane (.npy).
``--denoise`` writes the PNG from the denoised film (Integrator.denoise: the variance-guided a-trous filter over the
film and its moment plane, guided by the matte's alpha and tau / (1 + tau) unless ``--denoise-no-guides``): the
uniform frame is then rendered as one ordered launch with a moment plane (render.render_uniform: the reference's film
bit for bit) instead of through the feed, the guides come from one coverage pass with ``--alpha-sub`` (default 1)
sub-rays, which also serves ``--alpha``, and ``--alpha-foreground`` applies to the denoised film.
``--denoise-iters N`` and ``--denoise-sigma S`` set the iterations (1..6, default 4) and the Y scale (default 4);
``--denoised-film-out`` and ``--moments-out`` save the denoised film and the moment plane (.npy); ``--film-out``
still saves the raw film.  Exits 1 on a fatal error, like vptFATAL.
"""
from __future__ import annotations

import argparse
import sys
import time
from pathlib import Path


def _parse_synth(spec: str):
    kind, _, n = spec.partition(":")
    kinds = {"constant": (0, False), "cloud": (1, False), "fire": (1, True)}
    if kind not in kinds:
        raise ValueError(f"--synthetic wants constant|cloud|fire[:N], got {spec!r}")
    return kinds[kind][0], int(n or (128 if kind == "constant" else 512)), kinds[kind][1]


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(prog="python -m volume_path_tracer_amd", description=__doc__.splitlines()[0])
    ap.add_argument("config_path")
    ap.add_argument("output_path")
    ap.add_argument("--synthetic", default=None, help="constant|cloud|fire[:N] stand-in volume")
    ap.add_argument("--spp", type=int, default=None, help="override num_waves")
    ap.add_argument("--size", default=None, help="override output_size, WxH")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--batch-jobs", type=int, default=4096, help="tokens taken per push into the running launch")
    ap.add_argument("--film-out", default=None, help="also save the raw XYZW film (.npy)")
    ap.add_argument("--event-log", default=None,
                    help="write the Logger event log (log.csv format) of the first --event-jobs jobs")
    ap.add_argument("--event-jobs", type=int, default=1)
    ap.add_argument("--adaptive", type=float, default=None, metavar="ERR",
                    help="adaptive sampling: render each tile until its error estimate is <= ERR (--spp is the cap)")
    ap.add_argument("--min-spp", type=int, default=64, help="adaptive: waves of the first round")
    ap.add_argument("--spp-step", type=int, default=64, help="adaptive: waves per later round")
    ap.add_argument("--adaptive-fused", action="store_true",
                    help="adaptive: the one-launch driver (vpt_gpu_render_adaptive_fused; tiles of at most 256 pixels)")
    ap.add_argument("--waves-out", default=None, help="adaptive: save the per-tile wave map (.npy, uint32[T])")
    ap.add_argument("--alpha", action="store_true", help="write an RGBA PNG: A = round(255 * coverage)")
    ap.add_argument("--alpha-foreground", action="store_true",
                    help="implies --alpha: RGB of the medium alone (environment light removed), straight alpha")
    ap.add_argument("--alpha-sub", type=int, default=None, metavar="N",
                    help="alpha: N x N sub-rays per pixel, 1..8 (default 4 with jitter, 1 without)")
    ap.add_argument("--alpha-out", default=None, help="alpha: save the alpha plane (.npy, float32 [H][W])")
    ap.add_argument("--denoise", action="store_true", help="write the PNG from the denoised film (Integrator.denoise)")
    ap.add_argument("--denoise-iters", type=int, default=4, metavar="N", help="denoise: a-trous iterations, 1..6")
    ap.add_argument("--denoise-sigma", type=float, default=4.0, metavar="S",
                    help="denoise: Y distance scale in local standard deviations (sigma_l)")
    ap.add_argument("--denoise-no-guides", action="store_true", help="denoise: do not guide by the matte's planes")
    ap.add_argument("--denoised-film-out", default=None, help="denoise: save the denoised XYZW film (.npy)")
    ap.add_argument("--moments-out", default=None, help="denoise: save the film's moment plane (.npy, float32 [H][W])")
    args = ap.parse_args(argv)
    if (args.denoised_film_out or args.moments_out) and not args.denoise:
        ap.error("--denoised-film-out and --moments-out need --denoise")

    from . import image, traces, volumes
    from .render import Integrator, TileProvider, matte_guides, render_adaptive, render_uniform, run
    from .scenes import SynthGrid, read_configuration

    try:
        config_path = Path(args.config_path).resolve(strict=True)
        cfg = read_configuration(config_path)
        if args.spp is not None:
            cfg.num_waves = int(args.spp)
        if args.size:
            w, h = (int(v) for v in args.size.lower().split("x"))
            cfg.output_size[0], cfg.output_size[1] = w, h
        keep = []
        if args.synthetic:
            kind, n, with_temp = _parse_synth(args.synthetic)
            sd = SynthGrid(kind, n)
            st = SynthGrid(2, n) if with_temp else None
            keep += [sd, st]
            dens, temp = sd.grid(copy=False), (st.grid(copy=False) if st else None)
        else:
            vol = config_path.parent / cfg.volume_path.decode()
            dens, temp = volumes.read_grids(vol)
        if temp is not None and temp.leaf_count:
            print(f"TempMin: {float(temp.leaf_values.min())}, TempMax: {float(temp.leaf_values.max())}")

        it = Integrator(cfg, dens, temp, device=args.device)
        t0 = time.perf_counter()
        m2 = None
        if args.adaptive is not None:
            film, waves, err, info, *plane = render_adaptive(it, args.adaptive, min_waves=min(args.min_spp, cfg.num_waves),
                                                             step_waves=args.spp_step, max_waves=cfg.num_waves,
                                                             fused=args.adaptive_fused, return_moments=args.denoise)
            m2 = plane[0] if plane else None
            ms = (time.perf_counter() - t0) * 1e3
            driver = "one launch (fused)" if args.adaptive_fused else "rounds"
            print(f"[vpt] Adaptive rendering ({driver} driver) complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, "
                  f"target {args.adaptive:g}, "
                  f"{int(waves.min())}-{int(waves.max())} spp): {info['jobs_rendered']} of {info['jobs_uniform']} jobs "
                  f"({info['jobs_rendered'] / info['jobs_uniform']:.3f}), {info['rounds']} rounds, "
                  f"{info['tiles_at_max']} tiles at the cap, max tile error {info['max_error']:.4g}", file=sys.stderr)
            if args.waves_out:
                import numpy as np

                np.save(args.waves_out, waves)
        elif args.denoise:  # the ordered frame with its moment plane (the feed keeps none)
            film, m2 = (t.cpu().numpy() for t in render_uniform(it))
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp)",
                  file=sys.stderr)
        else:
            tp = TileProvider(cfg.output_size, cfg.num_waves, cfg.tile_size)
            tp.reset_eta()
            film = run(cfg, it, tp, batch_jobs=args.batch_jobs)
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp)",
                  file=sys.stderr)
        if args.event_log:
            scratch = it.torch.zeros_like(it.film)  # the traced jobs are not part of the image
            traces.write_event_log(it.trace_jobs(0, args.event_jobs, film=scratch), args.event_log)
        if args.film_out:
            import numpy as np

            np.save(args.film_out, film)
        if args.alpha or args.alpha_foreground or args.alpha_out:
            import numpy as np

            if args.denoise and not args.denoise_no_guides:  # one pass serves the matte and the guides
                guides = matte_guides(it, sub=args.alpha_sub or 1)
                alpha = guides[0]
            else:
                alpha = it.render_alpha(sub=args.alpha_sub)
            if args.alpha_out:
                np.save(args.alpha_out, alpha)
        if args.denoise:
            import numpy as np

            if args.denoise_no_guides:
                guides = []
            elif not (args.alpha or args.alpha_foreground or args.alpha_out):
                guides = matte_guides(it, sub=args.alpha_sub or 1)
            if args.moments_out:
                np.save(args.moments_out, m2)
            t1 = time.perf_counter()
            film = it.denoise(film, m2, guides, iterations=args.denoise_iters, sigma_l=args.denoise_sigma)
            ms = (time.perf_counter() - t1) * 1e3
            print(f"[vpt] Denoised in {ms:.1f} ms ({args.denoise_iters} iterations, {len(guides)} guides, "
                  f"sigma {args.denoise_sigma:g})", file=sys.stderr)
            if args.denoised_film_out:
                np.save(args.denoised_film_out, film)
        if args.alpha or args.alpha_foreground:
            rgb = image.film_to_image(image.foreground_film(film, alpha, cfg) if args.alpha_foreground else film)
            a8 = np.rint(np.float32(255.0) * alpha).astype(np.uint8)
            image.save_png(args.output_path, np.concatenate([rgb, a8[..., None]], axis=2))
        else:
            image.save_png(args.output_path, image.film_to_image(film))
    except Exception as e:  # vptFATAL: message and exit(1)
        print(f"[vpt] FATAL: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
