"""Sequences on one context, the host side: the exports and argument checks of vpt_gpu_set_scene / vpt_gpu_set_grids,
scenes.orbit, scenes.read_camera_path and the command line's pattern check.  No test here needs a device."""
import ctypes as C
import json

import numpy as np
import pytest

from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import SCENE_DIR, orbit, read_camera_path, scene, with_camera

VPT_E_INVALID, VPT_E_STATE = 1, 6


def _bits(v):
    return np.asarray(v[:], np.float32).view(np.uint32).tolist()


def test_library_exports_the_update_calls():
    """The two calls exist, the ABI version is still 1, and null arguments are VPT_E_INVALID (checked before any
    device call, so this runs without one)."""
    L = capi.lib()
    assert hasattr(L, "vpt_gpu_set_scene") and hasattr(L, "vpt_gpu_set_grids")
    assert L.vpt_abi_version() == 1
    cfg = scene("wdas_cloud")
    assert L.vpt_gpu_set_scene(None, C.byref(cfg)) == VPT_E_INVALID
    assert b"vpt_gpu_set_scene" in L.vpt_last_error()
    assert L.vpt_gpu_set_grids(None, None) == VPT_E_INVALID
    assert b"vpt_gpu_set_grids" in L.vpt_last_error()
    # a context is needed even with grids in hand
    g = C.c_void_p()
    from volume_path_tracer_amd.scenes import SynthGrid

    sg = SynthGrid(0, 16)
    capi.check(L.vpt_grids_flatten(C.byref(sg.desc), None, C.byref(g)), "vpt_grids_flatten")
    try:
        assert L.vpt_gpu_set_grids(None, g) == VPT_E_INVALID
    finally:
        L.vpt_grids_free(g)


@pytest.mark.parametrize("frames", [1, 4, 7])
def test_orbit(frames):
    cfg = scene("wdas_cloud")          # an oblique up vector that is not normalised
    cfg.num_waves = 3
    out = orbit(cfg, frames)
    assert len(out) == frames
    cp = cfg.camera_parameters
    assert _bits(out[0].camera_parameters.position) == _bits(cp.position)
    look = np.asarray(cp.look[:], np.float64)
    d0 = np.linalg.norm(np.asarray(cp.position[:], np.float64) - look)
    seen = set()
    for c in out:
        q = c.camera_parameters
        assert _bits(q.look) == _bits(cp.look) and _bits(q.up) == _bits(cp.up)
        assert _bits([q.vfov_deg]) == _bits([cp.vfov_deg]) and _bits([q.imaging_ratio]) == _bits([cp.imaging_ratio])
        assert c.num_waves == 3 and c.seed == cfg.seed
        # each component is rounded once to float32 (relative 2^-24 of a component <= the distance): the distance
        # moves by at most sqrt(3) * 2^-24 * max|component|, a few ulps of d0
        d = np.linalg.norm(np.asarray(q.position[:], np.float64) - look)
        bound = np.sqrt(3.0) * 2.0 ** -24 * np.abs(np.asarray(q.position[:], np.float64)).max() + 4 * np.spacing(np.float32(d0))
        assert abs(d - d0) <= bound, (d, d0)
        seen.add(tuple(_bits(q.position)))
    assert len(seen) == frames, "a full turn's frames are distinct (frame 0 is not repeated at the end)"
    # the orbit is a rotation about up: the height of the camera along up never changes, and frame k is at k / N turns
    up = np.asarray(cp.up[:], np.float64)
    up /= np.linalg.norm(up)
    r0 = np.asarray(cp.position[:], np.float64) - look
    p0 = r0 - up * (up @ r0)
    for k, c in enumerate(out):
        r = np.asarray(c.camera_parameters.position[:], np.float64) - look
        assert abs(up @ r - up @ r0) <= 1e-4 * d0
        p = r - up * (up @ r)
        ang = np.degrees(np.arctan2(up @ np.cross(p0, p), p0 @ p)) % 360.0
        assert abs(ang - 360.0 * k / frames) < 1e-3 or abs(ang - 360.0 * k / frames - 360.0) < 1e-3


def test_orbit_of_zero_degrees_is_copies_and_partial_turns_stop_short():
    cfg = scene("fire")
    for c in orbit(cfg, 5, degrees=0.0):
        assert bytes(c) == bytes(cfg)
    quarter = orbit(cfg, 3, 90.0)
    full = orbit(cfg, 12, 360.0)
    for k in range(3):   # 0, 30, 60 degrees
        assert _bits(quarter[k].camera_parameters.position) == _bits(full[k].camera_parameters.position)
    with pytest.raises(ValueError):
        orbit(cfg, 0)


def test_read_camera_path(tmp_path):
    good = [{"position": [1, 2, 3], "look": [0, 0, 0]},
            {"position": [1.5, 2, 3], "look": [0, 0.25, 0], "up": [0, 0, 1], "vfov_deg": 20}]
    p = tmp_path / "path.json"
    p.write_text(json.dumps(good))
    cams = read_camera_path(p)
    assert cams == [{"position": [1.0, 2.0, 3.0], "look": [0.0, 0.0, 0.0]},
                    {"position": [1.5, 2.0, 3.0], "look": [0.0, 0.25, 0.0], "up": [0.0, 0.0, 1.0], "vfov_deg": 20.0}]
    cfg = scene("wdas_cloud")
    c = with_camera(cfg, **cams[1])
    assert c.camera_parameters.position[:] == [1.5, 2.0, 3.0] and c.camera_parameters.vfov_deg == 20.0
    assert c.camera_parameters.up[:] == [0.0, 0.0, 1.0]
    c = with_camera(cfg, **cams[0])   # absent optional keys keep the scene's values
    assert _bits(c.camera_parameters.up) == _bits(cfg.camera_parameters.up)
    assert c.camera_parameters.vfov_deg == cfg.camera_parameters.vfov_deg
    bad = {
        "unknown key": [{"position": [1, 2, 3], "look": [0, 0, 0], "fov": 3}],
        "missing position": [{"look": [0, 0, 0]}],
        "not a list": {"position": [1, 2, 3], "look": [0, 0, 0]},
        "short vector": [{"position": [1, 2], "look": [0, 0, 0]}],
        "not a number": [{"position": [1, 2, "3"], "look": [0, 0, 0]}],
        "empty": [],
    }
    for what, doc in bad.items():
        p.write_text(json.dumps(doc))
        with pytest.raises(ValueError):
            read_camera_path(p)
        assert what


@pytest.mark.parametrize("extra", [
    [],                                                    # the output path itself has no field
    ["--film-out", "film.npy"],                            # one of the other paths has none
    ["--alpha-out", "a_%d_%d.npy"],                        # two fields
    ["--event-log", "log_%s.csv"],                         # a field that is no frame index
])
def test_cli_refuses_a_sequence_without_patterns_before_touching_hip(tmp_path, capsys, extra, monkeypatch):
    """Exit 1 with a message, before any Integrator exists: the constructor is replaced by one that fails the test,
    and torch's device state stays what it was (uninitialised, unless an earlier test of this process used a device)."""
    torch = pytest.importorskip("torch")
    from volume_path_tracer_amd import render
    from volume_path_tracer_amd.__main__ import main

    def no_integrator(*a, **k):
        raise AssertionError("an Integrator was created")

    monkeypatch.setattr(render, "Integrator", no_integrator)
    was_initialized = torch.cuda.is_initialized()
    out = str(tmp_path / ("o.png" if not extra else "o_%03d.png"))
    extra = [a if a.startswith("--") else str(tmp_path / a) for a in extra]
    rc = main([str(SCENE_DIR / "wdas_cloud.json"), out, "--synthetic", "cloud:64", "--frames", "3"] + extra)
    assert rc == 1
    assert "exactly one %d-style field" in capsys.readouterr().err
    assert torch.cuda.is_initialized() == was_initialized
    if not was_initialized:
        assert not torch.cuda.is_initialized(), "the refusal initialised a device"
    assert not list(tmp_path.iterdir()), "nothing was written"


def test_cli_sequence_argument_conflicts(tmp_path, capsys):
    from volume_path_tracer_amd.__main__ import main

    scene_path, out = str(SCENE_DIR / "wdas_cloud.json"), str(tmp_path / "o_%d.png")
    assert main([scene_path, out, "--volume-sequence", str(tmp_path / "v_%d.npz")]) == 1
    assert "--frames" in capsys.readouterr().err
    assert main([scene_path, out, "--frames", "2", "--orbit", "90", "--camera-path", "p.json"]) == 1
    assert "give one" in capsys.readouterr().err
    assert main([scene_path, out, "--frames", "0"]) == 1
    assert main([scene_path, out, "--frames", "2", "--volume-sequence", str(tmp_path / "v.npz")]) == 1
    assert "--volume-sequence" in capsys.readouterr().err
