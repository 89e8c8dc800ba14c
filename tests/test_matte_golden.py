"""Frozen bits of the matte march (tools/make_golden_matte.py): the tau plane, the depth and reach planes and the march
cut at a depth, of four frames, and the stand-alone program's fixed rays over four volumes.

The host build (tests/alpha_lib.py, tests/depth_lib.py) must reproduce every array byte for byte.  The GPU tests hold
vpt_alpha_kernel and vpt_depth_kernel to that host build byte for byte, so an edit of the march that moved a bit in
both would pass them; it is caught here."""
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parents[1]
GOLD = ROOT / "tests" / "golden" / "matte_planes.npz"


def _gen():
    import importlib.util

    spec = importlib.util.spec_from_file_location("make_golden_matte", ROOT / "tools" / "make_golden_matte.py")
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _same(got, want):
    assert sorted(got) == sorted(k for k in want.files if k.split("_")[0] in {g.split("_")[0] for g in got})
    for k, v in got.items():
        assert v.dtype == want[k].dtype and v.shape == want[k].shape, k
        assert v.tobytes() == want[k].tobytes(), (k, int((v.view(np.uint32) != want[k].view(np.uint32)).sum()))


@pytest.mark.parametrize("name", ["cube", "anchor", "cloud", "fire"])
def test_host_march_reproduces_golden_planes(name):
    want = np.load(GOLD)
    got = _gen().golden_planes(name)
    _same(got, want)
    assert got[f"{name}_upto"].size > 10  # the finite cut is exercised (the skewed camera's cloud covers 18 pixels)


def test_host_program_reproduces_golden_rays():
    want = np.load(GOLD)
    got = _gen().golden_program()
    _same(got, want)
    assert got["prog_tau"].shape == (4, 11) and (got["prog_reached"] == 4).sum() >= 8
