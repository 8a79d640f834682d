"""The alpha output's native entry points (include/gsr.h) through ctypes; no GPU needed.

gsr_alpha_views rejects a bad call before the library touches HIP, so every row here runs with dummy
device pointers (DEV) that are never dereferenced.  NO ROW MAY LAUNCH: every row is a rejected call
(rc != 0), as tests/test_capi_backward_args.py holds its rejected rows; whoever removes or reorders a
check of gsr_alpha_views in capi.hip runs this module on a machine without a GPU first.

The three backward entry points with dL_dalphas share the code, and with it the argument checks, of
the ones without (gsr_backward_dc_acc, gsr_backward_views, gsr_backward_render_views), which
tests/test_capi_backward_args.py pins; here their symbols and signatures are checked: dL_dalphas
directly after dL_invdepths, every other parameter as in the entry point it extends.
"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

INVALID = 1   # GSR_ERR_INVALID
DEV = 0x1000  # a "device pointer" no checked path dereferences
EXTENDS = {"gsr_backward_alpha": "gsr_backward_dc_acc", "gsr_backward_views_alpha": "gsr_backward_views",
           "gsr_backward_render_views_alpha": "gsr_backward_render_views"}


@pytest.fixture(scope="module")
def lib():
    from diff_gaussian_rasterization import _C
    return _C.lib


def _array(values):
    a = (ctypes.c_void_p * len(values))(*values)
    return a, ctypes.cast(a, ctypes.c_void_p)


# (V, width, height, image_buffers, out_alphas): None = a NULL array, a list = a host array of pointers
ROWS = [
    pytest.param(0, 32, 32, [], [], "V must be in [1, 16]", id="V-0"),
    pytest.param(17, 32, 32, [DEV] * 17, [DEV] * 17, "V must be in [1, 16]", id="V-17"),
    pytest.param(2, 32, 32, None, [DEV, DEV], "null per-view array", id="null-array-image_buffers"),
    pytest.param(2, 32, 32, [DEV, DEV], None, "null per-view array", id="null-array-out_alphas"),
    pytest.param(2, 32, 32, [DEV, None], [DEV, DEV], "null image buffer or alpha output", id="null-image_buffer"),
    pytest.param(2, 32, 32, [DEV, DEV], [None, DEV], "null image buffer or alpha output", id="null-out_alpha"),
    pytest.param(2, 0, 32, [DEV, DEV], [DEV, DEV], "width and height must be > 0", id="width-0"),
    pytest.param(2, 32, -1, [DEV, DEV], [DEV, DEV], "width and height must be > 0", id="height-negative"),
]


@pytest.mark.parametrize("V,width,height,images,outs,text", ROWS)
def test_alpha_views_argument_checks(lib, V, width, height, images, outs, text):
    keep, ptrs = [], []
    for values in (images, outs):
        if values is None:
            ptrs.append(None)
        else:
            a, p = _array(values or [None])
            keep.append(a)
            ptrs.append(p)
    rc = lib.gsr_alpha_views(V, width, height, ptrs[0], ptrs[1], None)
    err = lib.gsr_last_error().decode()
    assert rc == INVALID, f"returned {rc} ({err!r}), expected {INVALID}"
    assert err and text in err


def _parameters():
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {name: [p.split()[-1].lstrip("*") for p in params.split(",")]
            for name, params in re.findall(r"\b(gsr_\w+)\s*\(([^()]*)\)\s*;", text)}


def test_symbols_and_signatures(lib):
    names = _parameters()
    assert names["gsr_alpha_views"] == ["V", "width", "height", "image_buffers", "out_alphas", "stream"]
    fn = lib.gsr_alpha_views
    assert fn.argtypes is not None and len(fn.argtypes) == 6
    for new, old in EXTENDS.items():
        fn, base = getattr(lib, new), getattr(lib, old)
        assert fn.argtypes is not None, f"{new}: no argtypes"
        k = names[old].index("dL_invdepths") + 1
        assert names[new] == names[old][:k] + ["dL_dalphas"] + names[old][k:], new
        assert list(fn.argtypes) == list(base.argtypes[:k]) + [ctypes.c_void_p] + list(base.argtypes[k:]), new
