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
still saves the raw film.
``--frames N`` renders a sequence on one context (Integrator.set_scene / set_volume between frames, DESIGN.md section
13): ``--orbit DEG`` (default 360) turns the camera about ``look`` around ``up``, ``--camera-path FILE.json`` gives one
camera per frame ({position, look, up?, vfov_deg?}), ``--volume-sequence PATTERN`` renders the volume file
``PATTERN % k`` in frame k (read while frame k - 1 is written).  Every output path given must then hold exactly one
``%d``-style field for the frame index; each frame runs the single frame's code path with the same flags, its files are
written on a second thread while the next frame renders, and a closing line reports the update time and the total.
``--light-groups`` renders with light-group planes attached (Integrator.set_light_groups: the emission, the distant
light and the infinite light each in a film of its own, from the one set of paths) and writes ``<out>.emission.png``,
``<out>.sun.png`` and ``<out>.sky.png`` next to the beauty PNG, whose bytes do not change; the uniform frame is then
one ordered launch (render.render_uniform), the adaptive one the rounds driver.  ``--groups-out g.npy`` saves the planes
(float32 [3][H][W][4]).  ``--relight emission=K,sun=K,sky=K`` (implies ``--light-groups``; each K one number or X:Y:Z,
an absent group keeps 1) writes the output PNG from the relit film (Integrator.relight) instead; ``--film-out`` still
saves the raw film.  ``--relight-from g.npy`` relights a saved file with the same arithmetic in numpy (image.relight)
and opens no device: the configuration is not read.  Not with ``--denoise``, ``--alpha-foreground`` or
``--adaptive-fused``.
``--shutter-camera FILE.json`` renders camera motion blur (Integrator.set_shutter): the file holds
one camera object (a ``--camera-path`` entry), the camera at shutter close; the scene's camera is the camera at shutter
open, and wave k renders through the camera at the k-th time of scenes.shutter_times between them.
``--shutter-samples N`` sets the number of cameras (default ``num_waves``, at most 65536).  In a sequence with a moving
camera (``--frames`` with an orbit, or ``--camera-path``) ``--shutter F`` (0 < F <= 1) blurs frame k from its own camera
by the fraction F towards frame k + 1's; the last frame of a camera path extrapolates its previous step, the last
frame of an orbit uses the rotation at index ``frames``.  The uniform frame is then one ordered launch
(render.render_uniform), the adaptive one the rounds driver; ``--light-groups``, ``--relight`` and ``--denoise
--denoise-no-guides`` work.  Not with ``--alpha``, ``--alpha-foreground``, ``--alpha-out``, ``--depth-out``, ``--denoise``
guided by the matte, ``--adaptive-fused``, ``--rng-mode pixel`` or ``--event-log``: exit 1 before a device is touched.
``--depth-out z.npy`` saves the depth planes (Integrator.render_depth; float32 [K][H][W]): per
opacity of ``--depth-opacity A[,A...]`` (1..4 ascending values in (0, 1), default ``0.00392157,0.5``: the 8-bit matte's front
surface and the median free-flight depth) the distance from the camera at which a pixel's optical depth first reaches
that opacity, 0 where it never does.  ``--depth-sub N`` sets the sub-rays per axis (default 1), ``--depth-reach-out r.npy``
saves the fraction of sub-rays that reached each level.  One deterministic pass after the frame, with every driver and in
sequences; not with a shutter, and the other three flags need ``--depth-out``: exit 1 before a device is touched.
``--temporal`` (sequences only) accumulates the frames: after frame k is rendered (one ordered launch
with its moment plane, or either adaptive driver) and its depth planes are computed (the ``--depth-out`` call when that
runs at the default levels and one sub-ray), Integrator.temporal reprojects frame k - 1's accumulated film through the
depth planes and adds it; ``--denoise`` then filters the accumulated film and plane, and the PNG is written from the
result.  Frame k renders with seed ``seed + k`` (mod 2^32): with one seed every frame reuses the same job streams, the
noise of consecutive frames is correlated in screen space and accumulation gains nothing.  Frame 0 has no history: its
files equal the run without ``--temporal``.  ``--temporal-history N`` caps the history's sample count per pixel (default
4 x num_waves), ``--temporal-depth-tol T`` (default 0.1) and ``--temporal-sigma S`` (default 4) set the depth tolerance
and the rejection scale; ``--motion-out mv_%03d.npy`` saves the motion plane (float32 [H][W][2], pixels; NaN where a
point has no projection), ``--accumulated-film-out acc_%03d.npy`` the accumulated film; ``--film-out`` still saves the raw
film, and ``--moments-out`` saves the plane the denoiser read: the accumulated one.  Not without ``--frames`` / ``--camera-path``, nor with a shutter, ``--volume-sequence``, ``--light-groups`` /
``--relight`` or ``--rng-mode pixel``, and the other five flags need ``--temporal``: exit 1 before a device is touched.
``--rng-mode pixel`` renders the plain uniform frame in the pixel RNG mode (one stream per pixel sample; not the
reference's samples).
Exits 1 on a fatal error, like vptFATAL.
"""
from __future__ import annotations

import argparse
import re
import sys
import time
from pathlib import Path


def _parse_synth(spec: str):
    kind, _, n = spec.partition(":")
    kinds = {"constant": (0, False), "cloud": (1, False), "fire": (1, True)}
    if kind not in kinds:
        raise ValueError(f"--synthetic wants constant|cloud|fire[:N], got {spec!r}")
    return kinds[kind][0], int(n or (128 if kind == "constant" else 512)), kinds[kind][1]


_FIELD = re.compile(r"%0?\d*d")
_DEPTH_OPACITY = "0.00392157,0.5"


def _parse_depth_opacity(spec: str):
    """--depth-opacity's levels: 1..4 strictly ascending numbers in (0, 1), as float32 (what the library compares)."""
    import numpy as np

    try:
        a = np.array([float(x) for x in spec.split(",")], dtype=np.float32)
    except ValueError:
        raise ValueError(f"--depth-opacity wants A[,A...], got {spec!r}") from None
    if not 1 <= a.size <= 4:
        raise ValueError(f"--depth-opacity wants 1..4 opacities, got {a.size}")
    if not bool(np.all((a > 0) & (a < 1))):  # (also a NaN)
        raise ValueError(f"--depth-opacity: every opacity lies in (0, 1), got {spec!r}")
    if not bool(np.all(a[1:] > a[:-1])):
        raise ValueError(f"--depth-opacity: the opacities ascend strictly, got {spec!r}")
    return a
_GROUPS = ("emission", "sun", "sky")


def _parse_relight(spec: str):
    """--relight's gains: 'emission=K,sun=K,sky=K', each K a number or X:Y:Z -> 3 x 3 floats [group][XYZ]."""
    k = [[1.0, 1.0, 1.0] for _ in _GROUPS]
    for part in filter(None, (spec or "").split(",")):
        name, eq, val = part.partition("=")
        if not eq or name.strip() not in _GROUPS:
            raise ValueError(f"--relight wants emission=K,sun=K,sky=K (K a number or X:Y:Z), got {part!r}")
        v = [float(x) for x in val.split(":")]
        if len(v) not in (1, 3):
            raise ValueError(f"--relight {name}: one number or X:Y:Z, got {val!r}")
        k[_GROUPS.index(name.strip())] = v * 3 if len(v) == 1 else v
    return k


def _group_path(output_path: str, name: str) -> str:
    """<out>.<group>.png next to the beauty PNG <out>.png."""
    stem = output_path[:-4] if output_path.lower().endswith(".png") else output_path
    return f"{stem}.{name}.png"


def _frame_path(pattern: str, k: int) -> str:
    return pattern % k


def _sequence_problem(args, outputs) -> str:
    """What is wrong with a sequence's arguments ('' if nothing), from the arguments alone."""
    if args.frames is not None and args.frames < 1:
        return "--frames wants at least one frame"
    if args.frames is None and args.camera_path is None:
        return "--volume-sequence needs --frames N (or a --camera-path, one camera per frame)"
    if args.orbit is not None and args.camera_path is not None:
        return "--orbit and --camera-path both move the camera: give one"
    if args.volume_sequence is not None and args.synthetic:
        return "--volume-sequence and --synthetic both name the volume: give one"
    named = dict(outputs)
    named["--volume-sequence"] = args.volume_sequence
    for name, p in named.items():
        if p is None:
            continue
        fields = _FIELD.findall(p)
        if len(fields) != 1 or "%" in _FIELD.sub("", p, count=1):
            return (f"{name} {p!r}: in a sequence every path holds exactly one %d-style field for the frame index "
                    f"(e.g. frame_%04d.png)")
    return ""


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
    ap.add_argument("--frames", type=int, default=None, metavar="N",
                    help="a sequence of N frames on one context (every output path holds one %%d-style field)")
    ap.add_argument("--orbit", type=float, default=None, metavar="DEG",
                    help="sequence: the camera orbits `look` about `up` by DEG degrees over the frames (default 360)")
    ap.add_argument("--camera-path", default=None, metavar="FILE.json",
                    help="sequence: one camera per frame, a JSON list of {position, look, up?, vfov_deg?}")
    ap.add_argument("--volume-sequence", default=None, metavar="PATTERN",
                    help="sequence: frame k renders the volume file PATTERN %% k (.nvdb or .npz), swapped in place")
    ap.add_argument("--light-groups", action="store_true",
                    help="also write <out>.emission.png, <out>.sun.png, <out>.sky.png: one film per light source")
    ap.add_argument("--groups-out", default=None, help="light groups: save the planes (.npy, float32 [3][H][W][4])")
    ap.add_argument("--relight", default=None, metavar="emission=K,sun=K,sky=K",
                    help="implies --light-groups: the output PNG from the relit film; K a number or X:Y:Z")
    ap.add_argument("--relight-from", default=None, metavar="G.npy",
                    help="relight saved planes (--groups-out) into output_path; opens no device")
    ap.add_argument("--shutter-camera", default=None, metavar="FILE.json",
                    help="motion blur: the camera at shutter close, one {position, look, up?, vfov_deg?} object")
    ap.add_argument("--shutter-samples", type=int, default=None, metavar="N",
                    help="motion blur: cameras across the shutter (default num_waves, at most 65536)")
    ap.add_argument("--shutter", type=float, default=None, metavar="F",
                    help="sequence: blur frame k by the fraction F (0 < F <= 1) of the move to frame k + 1's camera")
    ap.add_argument("--depth-out", default=None, help="save the depth planes (.npy, float32 [K][H][W])")
    ap.add_argument("--depth-opacity", default=None, metavar="A[,A...]",
                    help=f"depth: 1..4 ascending opacities in (0, 1) (default {_DEPTH_OPACITY})")
    ap.add_argument("--depth-sub", type=int, default=None, metavar="N", help="depth: N x N sub-rays per pixel, 1..8 (default 1)")
    ap.add_argument("--depth-reach-out", default=None,
                    help="depth: save the fraction of sub-rays that reached each level (.npy, float32 [K][H][W])")
    ap.add_argument("--temporal", action="store_true",
                    help="sequence: add the previous frame's accumulated film, reprojected by depth (Integrator.temporal)")
    ap.add_argument("--temporal-history", type=float, default=None, metavar="N",
                    help="temporal: cap of the history's sample count per pixel (default 4 x num_waves)")
    ap.add_argument("--temporal-depth-tol", type=float, default=None, metavar="T",
                    help="temporal: relative depth tolerance of a history tap (default 0.1)")
    ap.add_argument("--temporal-sigma", type=float, default=None, metavar="S",
                    help="temporal: Y rejection scale in standard deviations (default 4)")
    ap.add_argument("--motion-out", default=None, help="temporal: save the motion plane (.npy, float32 [H][W][2])")
    ap.add_argument("--accumulated-film-out", default=None, help="temporal: save the accumulated XYZW film (.npy)")
    ap.add_argument("--rng-mode", choices=("reference", "pixel"), default="reference",
                    help="pixel: one RNG stream per pixel sample (the plain uniform frame only)")
    args = ap.parse_args(argv)
    if (args.denoised_film_out or args.moments_out) and not args.denoise:
        ap.error("--denoised-film-out and --moments-out need --denoise")
    want_groups = bool(args.light_groups or args.groups_out or args.relight is not None)
    try:
        gains = _parse_relight(args.relight)
    except ValueError as e:
        print(f"[vpt] FATAL: {e}", file=sys.stderr)
        return 1
    if want_groups or args.relight_from:
        for flag, on in (("--denoise", args.denoise), ("--alpha-foreground", args.alpha_foreground),
                         ("--adaptive-fused", args.adaptive_fused)):
            if on:
                print(f"[vpt] FATAL: {flag} does not combine with --light-groups / --relight (out of scope: README, "
                      f"Light groups)", file=sys.stderr)
                return 1
    depth_opacity = None
    if args.depth_out is None:
        for flag, given in (("--depth-opacity", args.depth_opacity), ("--depth-sub", args.depth_sub),
                            ("--depth-reach-out", args.depth_reach_out)):
            if given is not None:
                print(f"[vpt] FATAL: {flag} needs --depth-out", file=sys.stderr)
                return 1
    else:
        try:
            depth_opacity = _parse_depth_opacity(_DEPTH_OPACITY if args.depth_opacity is None else args.depth_opacity)
        except ValueError as e:
            print(f"[vpt] FATAL: {e}", file=sys.stderr)
            return 1
        if args.depth_sub is not None and not 1 <= args.depth_sub <= 8:
            print("[vpt] FATAL: --depth-sub wants 1 .. 8 sub-rays per axis", file=sys.stderr)
            return 1
    want_shutter = args.shutter_camera is not None or args.shutter is not None
    if want_shutter:  # (checked before anything touches a device: these would render the still camera, or raise late)
        for flag, on in (("--alpha", args.alpha), ("--alpha-foreground", args.alpha_foreground),
                         ("--alpha-out", args.alpha_out), ("--depth-out", args.depth_out),
                         ("--denoise", args.denoise and not args.denoise_no_guides),
                         ("--adaptive-fused", args.adaptive_fused), ("--rng-mode pixel", args.rng_mode == "pixel"),
                         ("--event-log", args.event_log), ("--relight-from", args.relight_from)):
            if on:
                why = " (its matte guides are the still camera's: add --denoise-no-guides)" if flag == "--denoise" else ""
                print(f"[vpt] FATAL: {flag} does not combine with a shutter (--shutter-camera / --shutter){why}: README, "
                      f"Motion blur", file=sys.stderr)
                return 1
        if args.shutter is not None and not 0.0 < args.shutter <= 1.0:
            print("[vpt] FATAL: --shutter wants a fraction F with 0 < F <= 1", file=sys.stderr)
            return 1
        if args.shutter_samples is not None and not 1 <= args.shutter_samples <= 65536:
            print("[vpt] FATAL: --shutter-samples wants 1 .. 65536 cameras", file=sys.stderr)
            return 1
    elif args.shutter_samples is not None:
        ap.error("--shutter-samples needs --shutter-camera or --shutter")
    if not args.temporal:
        for flag, given in (("--temporal-history", args.temporal_history), ("--temporal-depth-tol", args.temporal_depth_tol),
                            ("--temporal-sigma", args.temporal_sigma), ("--motion-out", args.motion_out),
                            ("--accumulated-film-out", args.accumulated_film_out)):
            if given is not None:
                print(f"[vpt] FATAL: {flag} needs --temporal", file=sys.stderr)
                return 1
    else:  # (checked before anything touches a device)
        for why, on in (("it accumulates the frames of a sequence: it needs --frames or --camera-path",
                         args.frames is None and args.camera_path is None),
                        ("not with a shutter (--shutter / --shutter-camera): the depth pass refuses one", want_shutter),
                        ("not with --volume-sequence: the medium moves and has no motion vectors", args.volume_sequence),
                        ("not with --light-groups / --relight: the group planes have no history",
                         want_groups or args.relight_from),
                        ("not with --rng-mode pixel: that mode keeps no moment plane", args.rng_mode == "pixel")):
            if on:
                print(f"[vpt] FATAL: --temporal: {why} (README, Temporal accumulation)", file=sys.stderr)
                return 1
        for flag, v in (("--temporal-history", args.temporal_history), ("--temporal-depth-tol", args.temporal_depth_tol),
                        ("--temporal-sigma", args.temporal_sigma)):
            if v is not None and not v > 0.0:  # (also a NaN)
                print(f"[vpt] FATAL: {flag} wants a number > 0", file=sys.stderr)
                return 1
    if args.rng_mode == "pixel" and (args.adaptive is not None or args.denoise or want_groups):
        print("[vpt] FATAL: --rng-mode pixel renders the plain uniform frame only (not with --adaptive, --denoise or "
              "--light-groups)", file=sys.stderr)
        return 1
    if args.relight_from:  # host work only: no device, no configuration
        try:
            import numpy as np

            from . import image

            image.save_png(args.output_path, image.film_to_image(image.relight(np.load(args.relight_from), gains)))
        except Exception as e:
            print(f"[vpt] FATAL: {e}", file=sys.stderr)
            return 1
        return 0

    # ---- sequences: every output path is a pattern over the frame index (checked before anything touches a device)
    sequence = args.frames is not None or args.camera_path is not None or args.volume_sequence is not None
    outputs = {"output_path": args.output_path, "--film-out": args.film_out, "--alpha-out": args.alpha_out,
               "--waves-out": args.waves_out, "--denoised-film-out": args.denoised_film_out,
               "--moments-out": args.moments_out, "--event-log": args.event_log, "--groups-out": args.groups_out,
               "--depth-out": args.depth_out, "--depth-reach-out": args.depth_reach_out,
               "--motion-out": args.motion_out, "--accumulated-film-out": args.accumulated_film_out}
    if sequence:
        problem = _sequence_problem(args, outputs)
        if problem:
            print(f"[vpt] FATAL: {problem}", file=sys.stderr)
            return 1
    elif args.orbit is not None:
        ap.error("--orbit needs --frames")
    if args.shutter is not None and (not sequence or (args.frames is None and args.camera_path is None)
                                     or (args.volume_sequence and args.orbit is None and args.camera_path is None)):
        print("[vpt] FATAL: --shutter blurs a sequence's frames towards the next frame's camera: it needs --frames with "
              "an orbit, or --camera-path (a single frame takes --shutter-camera)", file=sys.stderr)
        return 1
    if args.shutter_camera is not None and (sequence or args.shutter is not None):
        print("[vpt] FATAL: --shutter-camera is the single frame's camera at shutter close; a sequence takes --shutter F",
              file=sys.stderr)
        return 1

    from . import image, traces, volumes
    from .render import (Integrator, TemporalState, TileProvider, matte_guides, render_adaptive, render_sequence,
                         render_uniform, run)
    from .scenes import (SynthGrid, camera_of, lerp_camera, orbit, read_camera, read_camera_path, read_configuration,
                         shutter_cameras, with_camera)

    # --temporal reprojects through the default --depth-out planes, so that one call serves both when the user keeps them
    temporal_levels = _parse_depth_opacity(_DEPTH_OPACITY) if args.temporal else None
    temporal_state = []  # (the sequence's TemporalState, once its Integrator exists)

    def render_frame(it, tag="", paths=None):
        """One frame's device work, as the single-frame program does it -> what write_frame saves (host arrays).
        paths (the single-frame program): each file is written as soon as its data exists, as it always was -- the raw
        film is on disk before the alpha and denoise passes run; a sequence leaves the files to its writer thread."""
        cfg = it.cfg
        res = {"cfg": cfg}

        def emit(piece):
            if paths is not None:
                write_piece(piece, res, paths)

        t0 = time.perf_counter()
        m2 = None
        if args.adaptive is not None:
            film, waves, err, info, *plane = render_adaptive(it, args.adaptive, min_waves=min(args.min_spp, cfg.num_waves),
                                                             step_waves=args.spp_step, max_waves=cfg.num_waves,
                                                             fused=args.adaptive_fused,
                                                             return_moments=args.denoise or args.temporal,
                                                             groups=want_groups)
            if want_groups:
                res["groups"] = plane.pop()
            m2 = plane[0] if plane else None
            ms = (time.perf_counter() - t0) * 1e3
            driver = "one launch (fused)" if args.adaptive_fused else "rounds"
            print(f"[vpt] {tag}Adaptive rendering ({driver} driver) complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, "
                  f"target {args.adaptive:g}, "
                  f"{int(waves.min())}-{int(waves.max())} spp): {info['jobs_rendered']} of {info['jobs_uniform']} jobs "
                  f"({info['jobs_rendered'] / info['jobs_uniform']:.3f}), {info['rounds']} rounds, "
                  f"{info['tiles_at_max']} tiles at the cap, max tile error {info['max_error']:.4g}", file=sys.stderr)
            res["waves"] = waves
            emit("waves")
        elif args.rng_mode == "pixel":  # (feeds run the reference RNG mode: plain launches, film atomics)
            dev_film = it.torch.zeros_like(it.film)
            it.render_waves(1, int(cfg.num_waves), film=dev_film)
            film = dev_film.cpu().numpy()
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] {tag}Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp, pixel RNG mode)",
                  file=sys.stderr)
        elif args.denoise or args.temporal:  # the ordered frame with its moment plane (the feed keeps none)
            film, m2 = (t.cpu().numpy() for t in render_uniform(it))
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] {tag}Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp)",
                  file=sys.stderr)
        elif want_groups:  # the ordered frame with its group planes (the feed writes none)
            film, res["groups"] = (t.cpu().numpy() for t in render_uniform(it, moments=False, groups=True))
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] {tag}Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp, light groups)",
                  file=sys.stderr)
        elif want_shutter:  # the ordered frame: a feed's launch does not honour the shutter
            film = render_uniform(it, moments=False).cpu().numpy()
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] {tag}Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp, a shutter "
                  f"of {it.shutter_info()} cameras)", file=sys.stderr)
        else:
            tp = TileProvider(cfg.output_size, cfg.num_waves, cfg.tile_size)
            tp.reset_eta()
            film = run(cfg, it, tp, batch_jobs=args.batch_jobs)
            ms = (time.perf_counter() - t0) * 1e3
            print(f"[vpt] {tag}Rendering complete in {ms:.0f} ms ({cfg.width}x{cfg.height}, {cfg.num_waves} spp)",
                  file=sys.stderr)
        if args.event_log:
            scratch = it.torch.zeros_like(it.film)  # the traced jobs are not part of the image
            res["events"] = it.trace_jobs(0, args.event_jobs, film=scratch)
            emit("events")
        res["film"] = film
        emit("film")
        if want_groups:
            emit("groups")
            if args.relight is not None:
                res["relit"] = it.relight(res["groups"], gains)
        if args.alpha or args.alpha_foreground or args.alpha_out:
            if args.denoise and not args.denoise_no_guides:  # one pass serves the matte and the guides
                guides = matte_guides(it, sub=args.alpha_sub or 1)
                alpha = guides[0]
            else:
                alpha = it.render_alpha(sub=args.alpha_sub)
            res["alpha"] = alpha
            emit("alpha")
        if args.depth_out:
            res["depth"], res["reach"] = it.render_depth(depth_opacity, sub=args.depth_sub or 1, reach=True)
            emit("depth")
        if args.temporal:
            import numpy as np

            shared = (args.depth_out and (args.depth_sub or 1) == 1 and depth_opacity.tobytes() == temporal_levels.tobytes())
            tdepth = res["depth"] if shared else it.render_depth(temporal_levels, sub=1)
            t1 = time.perf_counter()
            acc = temporal_state[0].accumulate(it, film, m2, depth=tdepth, motion=bool(args.motion_out), hist_n=True)
            res["acc_film"], res["acc_m2"] = acc[0], acc[1]
            if args.motion_out:
                res["motion"] = acc[2]
            ms = (time.perf_counter() - t1) * 1e3
            n_cur, n_hist = float(np.nansum(film[..., 3])), float(acc[-1].sum())
            print(f"[vpt] {tag}Accumulated in {ms:.1f} ms: history adds {n_hist / max(n_cur, 1.0):.2f} x the frame's own "
                  f"samples", file=sys.stderr)
            emit("acc")
            film, m2 = res["acc_film"], res["acc_m2"]  # (what --denoise filters and the PNG shows)
        if args.denoise:
            if args.denoise_no_guides:
                guides = []
            elif not (args.alpha or args.alpha_foreground or args.alpha_out):
                guides = matte_guides(it, sub=args.alpha_sub or 1)
            res["m2"] = m2
            emit("m2")
            t1 = time.perf_counter()
            res["denoised"] = it.denoise(film, m2, guides, iterations=args.denoise_iters, sigma_l=args.denoise_sigma)
            ms = (time.perf_counter() - t1) * 1e3
            print(f"[vpt] {tag}Denoised in {ms:.1f} ms ({args.denoise_iters} iterations, {len(guides)} guides, "
                  f"sigma {args.denoise_sigma:g})", file=sys.stderr)
            emit("denoised")
        emit("png")
        return res

    PIECES = ("waves", "events", "film", "groups", "alpha", "depth", "acc", "m2", "denoised", "png")

    def write_piece(piece, res, paths):
        """One of a frame's files, from what render_frame has produced (host work only)."""
        import numpy as np

        if piece == "waves" and "waves" in res and paths["--waves-out"]:
            np.save(paths["--waves-out"], res["waves"])
        elif piece == "events" and "events" in res:
            traces.write_event_log(res["events"], paths["--event-log"])
        elif piece == "film" and paths["--film-out"]:
            np.save(paths["--film-out"], res["film"])
        elif piece == "groups" and "groups" in res:
            if paths["--groups-out"]:
                np.save(paths["--groups-out"], res["groups"])
            for name, plane in zip(_GROUPS, res["groups"]):
                image.save_png(_group_path(paths["output_path"], name), image.film_to_image(plane))
        elif piece == "alpha" and "alpha" in res and paths["--alpha-out"]:
            np.save(paths["--alpha-out"], res["alpha"])
        elif piece == "depth" and "depth" in res:
            np.save(paths["--depth-out"], res["depth"])
            if paths["--depth-reach-out"]:
                np.save(paths["--depth-reach-out"], res["reach"])
        elif piece == "acc" and "acc_film" in res:
            if paths["--accumulated-film-out"]:
                np.save(paths["--accumulated-film-out"], res["acc_film"])
            if paths["--motion-out"]:
                np.save(paths["--motion-out"], res["motion"])
        elif piece == "m2" and args.denoise and paths["--moments-out"]:
            np.save(paths["--moments-out"], res["m2"])
        elif piece == "denoised" and args.denoise and paths["--denoised-film-out"]:
            np.save(paths["--denoised-film-out"], res["denoised"])
        elif piece == "png":
            film = res["denoised"] if args.denoise else res.get("relit", res.get("acc_film", res["film"]))
            if args.alpha or args.alpha_foreground:
                alpha = res["alpha"]
                rgb = image.film_to_image(image.foreground_film(film, alpha, res["cfg"]) if args.alpha_foreground else film)
                a8 = np.rint(np.float32(255.0) * alpha).astype(np.uint8)
                image.save_png(paths["output_path"], np.concatenate([rgb, a8[..., None]], axis=2))
            else:
                image.save_png(paths["output_path"], image.film_to_image(film))

    def write_frame(res, paths):
        """A frame's files, in the single frame's order (a sequence runs this on its writer thread)."""
        for piece in PIECES:
            write_piece(piece, res, paths)

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
        elif args.volume_sequence:
            dens, temp = volumes.read_grids(_frame_path(args.volume_sequence, 0))
        else:
            vol = config_path.parent / cfg.volume_path.decode()
            dens, temp = volumes.read_grids(vol)
        if temp is not None and temp.leaf_count:
            print(f"TempMin: {float(temp.leaf_values.min())}, TempMax: {float(temp.leaf_values.max())}")

        n_shutter = min(int(cfg.num_waves), 65536) if args.shutter_samples is None else args.shutter_samples
        if not sequence:
            close = read_camera(args.shutter_camera) if args.shutter_camera is not None else None
            it = Integrator(cfg, dens, temp, device=args.device)
            if args.rng_mode == "pixel":
                it.set_rng_mode(1)
            if close is not None:
                it.set_shutter(shutter_cameras(camera_of(cfg), camera_of(with_camera(cfg, **close)), n_shutter))
            render_frame(it, paths=outputs)
            return 0

        # ---- a sequence: one Integrator, updated in place between frames (Integrator.set_scene / set_volume)
        if args.camera_path:
            cams = read_camera_path(args.camera_path)
            if args.frames is not None and args.frames != len(cams):
                raise ValueError(f"--frames {args.frames} but {args.camera_path} holds {len(cams)} cameras")
            cfgs = [with_camera(cfg, **c) for c in cams]
            # (--shutter: the last frame closes where its previous step, repeated, would lead; one frame: nowhere)
            last, prev = camera_of(cfgs[-1]), camera_of(cfgs[-2] if len(cfgs) > 1 else cfgs[-1])
            closing = lerp_camera(prev, last, 2.0)
        elif args.orbit is not None or not args.volume_sequence:
            cfgs = orbit(cfg, args.frames, 360.0 if args.orbit is None else args.orbit, closing=args.shutter is not None)
            closing = camera_of(cfgs.pop()) if args.shutter is not None else None
        else:
            cfgs = [None] * args.frames  # (the volume alone changes)
        nframes = len(cfgs)
        if args.temporal:  # independent noise per frame: with one seed every frame reuses the same job streams
            for k, c in enumerate(cfgs):
                c.seed = (int(cfg.seed) + k) & 0xFFFFFFFF
        shutters = None
        if args.shutter is not None:  # frame k: from its own camera by the fraction F towards frame k + 1's
            opens = [camera_of(c) for c in cfgs]
            shutters = [shutter_cameras(a, lerp_camera(a, b, args.shutter), n_shutter)
                        for a, b in zip(opens, opens[1:] + [closing])]
        it = Integrator(cfgs[0] if cfgs[0] is not None else cfg, dens, temp, device=args.device)
        if args.rng_mode == "pixel":
            it.set_rng_mode(1)
        if args.temporal:
            temporal_state.append(TemporalState(it, levels=int(temporal_levels.size), max_history=args.temporal_history,
                                                depth_tol=0.1 if args.temporal_depth_tol is None else args.temporal_depth_tol,
                                                sigma_r=4.0 if args.temporal_sigma is None else args.temporal_sigma))
        t_seq = time.perf_counter()

        def frames():
            yield None, None  # (frame 0: the Integrator as created)
            for k in range(1, nframes):
                # (frame k's volume is read here, while the writer thread still saves frame k - 1)
                vol = volumes.read_grids(_frame_path(args.volume_sequence, k)) if args.volume_sequence else None
                yield cfgs[k], vol

        count = iter(range(nframes))

        def sequence_frame(i):
            k = next(count)
            if shutters is not None:
                i.set_shutter(shutters[k])
            return render_frame(i, f"frame {k}: ")

        stats = render_sequence(it, frames(), sequence_frame,
                                lambda k, res: write_frame(res, {n: (_frame_path(p, k) if p else p)
                                                                 for n, p in outputs.items()}))
        total = (time.perf_counter() - t_seq) * 1e3
        print(f"[vpt] Sequence complete: {stats['frames']} frames in {total:.0f} ms; scene / volume updates "
              f"{sum(stats['update_ms']):.1f} ms in all (largest {max(stats['update_ms']):.1f} ms), tile-cost passes "
              f"{it.setup_timings()['tile_costs']:.1f} ms", file=sys.stderr)
    except Exception as e:  # vptFATAL: message and exit(1)
        print(f"[vpt] FATAL: {e}", file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
