"""Host-side checks of vpt_gpu_render_adaptive_fused (no GPU needed): the export, its argument checks, which come
before any use of a device, and the Python binding's declaration."""
import ctypes as C
import re
import subprocess

import numpy as np

from volume_path_tracer_amd import capi

VPT_E_INVALID = 1


def test_the_library_exports_the_call():
    out = subprocess.run(["nm", "-D", "--defined-only", str(capi.LIB_PATH)], capture_output=True, text=True).stdout
    assert "vpt_gpu_render_adaptive_fused" in set(re.findall(r"\bT (vpt_\w+)", out))
    assert capi.lib().vpt_gpu_render_adaptive_fused is not None


def test_capi_declares_its_argument_types():
    L = capi.lib()
    assert L.vpt_gpu_render_adaptive_fused.argtypes == L.vpt_gpu_render_adaptive.argtypes
    a = L.vpt_gpu_render_adaptive_fused.argtypes
    assert len(a) == 8 and a[1] == C.POINTER(capi.AdaptiveParams) and a[6] == C.POINTER(capi.AdaptiveResult)
    assert a[4] == C.POINTER(C.c_uint32) and a[5] == C.POINTER(C.c_float)


def test_null_arguments_are_invalid_without_a_device():
    L = capi.lib()
    p = capi.AdaptiveParams(0.1, 1e-3, 8, 8, 32)
    res = capi.AdaptiveResult()
    wv, er = np.zeros(4, np.uint32), np.zeros(4, np.float32)
    wp, ep = wv.ctypes.data_as(C.POINTER(C.c_uint32)), er.ctypes.data_as(C.POINTER(C.c_float))
    plane = C.c_void_p(0x1000)  # (never dereferenced: the context is checked first)
    assert L.vpt_gpu_render_adaptive_fused(None, C.byref(p), None, plane, wp, ep, C.byref(res), None) == VPT_E_INVALID
    assert b"vpt_gpu_render_adaptive_fused" in L.vpt_last_error() and b"null" in L.vpt_last_error()
    assert L.vpt_gpu_render_adaptive_fused(None, None, None, None, None, None, None, None) == VPT_E_INVALID
    assert not wv.any() and not er.any()


def test_render_adaptive_takes_the_fused_argument():
    import inspect

    from volume_path_tracer_amd.render import render_adaptive

    assert inspect.signature(render_adaptive).parameters["fused"].default is False
