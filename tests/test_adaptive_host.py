"""Host-side checks of the adaptive-sampling calls (no GPU needed): exports, the ABI version, the documented codes
of null-context and bad-parameter calls, and a self-check of the numpy restatement of vpt_gpu_tile_errors (tests/
adaptive_ref.py) on a hand-made film."""
import ctypes as C
import re
import subprocess

import numpy as np

import adaptive_ref as A
from volume_path_tracer_amd import capi
from volume_path_tracer_amd.scenes import workload

VPT_E_INVALID = 1
NEW = ("vpt_gpu_set_film_moments", "vpt_gpu_render_tile_list", "vpt_gpu_tile_errors", "vpt_gpu_render_adaptive")
F = np.float32


def test_new_symbols_are_exported():
    lib = capi.lib()
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (vpt_\w+)", out))
    for n in NEW:
        assert n in exported, n
        getattr(lib, n)
    assert lib.vpt_abi_version() == 1


def test_struct_layouts():
    assert C.sizeof(capi.AdaptiveParams) == 20
    assert C.sizeof(capi.AdaptiveResult) == 32
    assert capi.AdaptiveResult.jobs_rendered.offset == 8 and capi.AdaptiveResult.max_error.offset == 24


def test_null_context_and_bad_parameters():
    L = capi.lib()
    one = (C.c_uint32 * 1)(0)
    err = (C.c_float * 1)()
    dummy = C.c_void_p(16)  # never dereferenced: the calls fail on their arguments first
    assert L.vpt_gpu_set_film_moments(None, None) == VPT_E_INVALID
    assert b"null context" in L.vpt_last_error()
    assert L.vpt_gpu_render_tile_list(None, one, 1, 0, 1, None, None) == VPT_E_INVALID
    assert L.vpt_gpu_tile_errors(None, None, dummy, 1e-3, err, None) == VPT_E_INVALID
    p = capi.AdaptiveParams(0.1, 1e-3, 8, 8, 32)
    waves = (C.c_uint32 * 1)()
    assert L.vpt_gpu_render_adaptive(None, C.byref(p), None, dummy, waves, err, None, None) == VPT_E_INVALID
    assert b"null" in L.vpt_last_error()


def test_tile_error_restatement_on_a_hand_made_film():
    wl = workload("c3", width=37, height=29, spp=4, grid_n=64)
    cfg = wl.cfg
    film, m2 = A.hand_made_film(cfg)
    floor = F(1e-3)
    err = A.tile_errors(cfg, film, m2, floor)
    assert err.dtype == np.float32 and err.shape == (cfg.jobs_per_wave(),)
    assert err[1] < 1e-3  # the all-equal tile: v clamps to 0 or is a rounding residue
    assert err[2] == 0 and err[3] == 0  # black: 0 / (0 + floor * cnt); no counted pixel: defined 0
    assert np.isfinite(err).all() and (err[4:] > 0).all()
    # one tile by hand, in Python floats rounded after every operation, with an explicit tree
    t = 0
    x0, y0, rw, rh = A.tile_rect(cfg, t)
    se, mean, cnt = [F(0)] * 64, [F(0)] * 64, 0
    for yl in range(rh):
        for xl in range(rw):
            f, m = film[y0 + yl, x0 + xl], m2[y0 + yl, x0 + xl]
            n = f[3]
            if n >= 2:
                mu = F(f[1] / n)
                v = F(F(m / n) - F(mu * mu))
                v = v if v > 0 else F(0)
                se[yl * rw + xl] = F(np.sqrt(F(v / F(n - F(1)))))
                mean[yl * rw + xl] = mu
                cnt += 1
    assert cnt == 62  # (0, 0) has no sample, (2, 1) one

    def tree(a):
        a = list(a)
        h = len(a) // 2
        while h >= 1:
            for i in range(h):
                a[i] = F(a[i] + a[i + h])
            h //= 2
        return a[0]

    want = F(tree(se) / F(tree(mean) + F(floor * F(cnt))))
    assert err[t].view(np.uint32) == want.view(np.uint32)
    # the tree's association is not the left-to-right sum's
    a = (np.arange(1, 65, dtype=np.float32) * F(0.1)).astype(np.float32)
    assert A.tree_sum(a) == tree(a)
