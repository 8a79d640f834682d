"""The argument checks of the native backward entry points (include/gsr.h), through ctypes; no GPU needed.

A rejected call, a P == 0 call and a render-only call whose views all have R == 0 return before the
library touches HIP, so every row here runs with dummy device pointers (DEV) that are never
dereferenced.  NO ROW MAY LAUNCH: a row is either rejected (rc != 0) or has P == 0 or R == 0, and
`test_no_row_can_launch` holds the table to that.  (gsr_backward_camera_views writes its zeros with a
kernel also for P == 0, so it has no P == 0 row.)

That guard covers the GSR_OK rows only.  A rejected row stays launch-free only while its check holds:
if a check regresses, the call goes on to a launch with DEV pointers, which on a machine with a GPU is
a fault of the device, not a failed assertion.  The risk is accepted because the rows exist to pin
exactly those checks and cannot be driven any other way without a GPU; whoever removes or reorders a
check in capi.hip runs this module on a machine without a GPU first.

Each row is one call with exactly one thing wrong (or nothing wrong, for the GSR_OK rows): the entry
point, the arguments that differ from a valid call, the return code and a substring of gsr_last_error().
The expected values of the rows not marked TIGHTENED are what the library answered before the
backward's host code became one path (measured on that build, not read off the new code); TIGHTENED
rows are calls that build let through -- into a kernel with a null pointer, or with a negative count
read as "nothing" -- and that every backward entry point now rejects alike.
"""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, INVALID, ALLOC = 0, 1, 3  # GSR_OK, GSR_ERR_INVALID, GSR_ERR_ALLOC
DEV = 0x1000                  # a "device pointer" no checked path dereferences
V, P, R = 2, 200, 5

ONE_OF = "Please provide exactly one of either SHs or precomputed colors!"
V_RANGE = "V must be in [1, 16]"
ARRAY = "null per-view array"
STATE = "null state buffer"
GRADIENT = "null per-view gradient"
PARAMS = "null parameter array"
CAMERA = "null camera"
RANGE = "range outside [0, P)"
CAM_OUT = "null workspace or camera gradient"

# host arrays of the batched entry points and what their elements are
POINTER_ARRAYS = ("viewmatrices", "projmatrices", "campos", "radii", "geom_buffers", "binning_buffers",
                  "image_buffers", "dL_dpix", "dL_invdepths", "dL_dmean2D")
BATCHED = ("gsr_backward_render_views", "gsr_backward_preprocess_views_range", "gsr_backward_views",
           "gsr_backward_camera_views")
RENDER_ONLY = ("gsr_backward_render", "gsr_backward_render_views")

# a valid call: every argument not named here is a non-null dummy device pointer
VALID = {"V": V, "P": P, "D": 3, "M": 16, "width": 32, "height": 32, "scale_modifier": 1.0, "tan_fovx": 0.5,
         "tan_fovy": 0.5, "antialiasing": False, "debug": False, "has_invdepth": False, "accumulate": 0,
         "g_begin": 0, "stream": None,
         # optional inputs and outputs that a plain call leaves out
         "dc": None, "colors_precomp": None, "cov3D_precomp": None, "radii": None, "dL_invdepths": None,
         "dL_dinvdepth": None, "dL_ddc": None}
DC = {"dc": DEV, "dL_ddc": DEV, "M": 15}  # the separate-dc surface, valid


def _parameter_names():
    with open(os.path.join(ROOT, "include", "gsr.h")) as f:
        text = re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S)
    return {name: [p.split()[-1].lstrip("*") for p in params.split(",")]
            for name, params in re.findall(r"\b(gsr_backward\w*)\s*\(([^()]*)\)\s*;", text)}


NAMES = _parameter_names()


def _value(entry, name, args):
    if name in args:
        return args[name]
    if name == "g_end":
        return args.get("P", P)
    if name == "R":
        return [R] * V if entry in BATCHED else R
    if entry in BATCHED and name in ("tan_fovx", "tan_fovy"):
        return [0.5] * V
    if name in VALID:
        return VALID[name]
    return [DEV] * V if name in POINTER_ARRAYS else DEV


def _call(lib, entry, args):
    unknown = set(args) - set(NAMES[entry])
    assert not unknown, f"{entry} has no parameter {unknown}"
    fn, keep, argv = getattr(lib, entry), [], []
    for name, ct in zip(NAMES[entry], fn.argtypes):
        v = _value(entry, name, args)
        if isinstance(v, list):  # a per-view host array
            kind = ctypes.c_void_p if name in POINTER_ARRAYS else ctypes.c_int if name == "R" else ctypes.c_float
            v = (kind * len(v))(*v)
            keep.append(v)
            v = ctypes.cast(v, ctypes.c_void_p)
        argv.append(v if ct is ctypes.c_void_p else ct(v))
    rc = fn(*argv)
    return rc, lib.gsr_last_error().decode()


TIGHTENED = "tightened"


def row(entry, what, args, rc, text="", mark=None):
    return pytest.param(entry, args, rc, text, mark, id=f"{entry[4:]}-{what}")


def _shared_preprocess_rows(entry, base):
    """What gsr_backward_dc_acc, gsr_backward_preprocess_views_range and gsr_backward_views check alike
    (base: arguments that keep the render half of gsr_backward_views from launching first)."""
    return [
        row(entry, "accumulate-bits", {**base, "accumulate": 256}, INVALID, "unknown accumulate bits"),
        row(entry, "dc-without-dL_ddc", {**base, **DC, "dL_ddc": None}, INVALID, "dc given without dL_ddc"),
        row(entry, "dc-with-colors_precomp", {**base, **DC, "colors_precomp": DEV}, INVALID, ONE_OF),
        row(entry, "dc-null-shs", {**base, **DC, "shs": None}, INVALID, "dc given with M > 0 but shs/dL_dsh NULL"),
        row(entry, "dc-null-dL_dsh", {**base, **DC, "dL_dsh": None}, INVALID,
            "dc given with M > 0 but shs/dL_dsh NULL"),
    ] + [row(entry, f"null-{a}", {**base, a: None}, INVALID, PARAMS, TIGHTENED)
         for a in ("means3D", "opacities", "scales", "rotations")]


def _batch_rows(entry, arrays, base):
    return [row(entry, f"V-{v}", {"V": v}, INVALID, V_RANGE) for v in (0, 17)] + \
           [row(entry, f"null-array-{a}", {**base, a: None}, INVALID, ARRAY) for a in arrays]


NO_RENDER = {"R": [0, 0]}  # gsr_backward_views: BACKWARD::render launches nothing, the preprocess half checks
CAMERAS = ("viewmatrices", "projmatrices", "campos")

ROWS = (
    # ---- gsr_backward_dc_acc (gsr_backward_dc and gsr_backward forward to it) ----
    _shared_preprocess_rows("gsr_backward_dc_acc", {}) + [
        row("gsr_backward_dc_acc", "invdepth-without-output", {"dL_invdepths": DEV}, INVALID,
            "dL_dinvdepth must be given with dL_invdepths"),
        row("gsr_backward_dc_acc", "null-binning", {"binning_buffer": None}, ALLOC, "null binning buffer"),
        row("gsr_backward_dc_acc", "P-0", {"P": 0}, OK),
        row("gsr_backward_dc_acc", "P-negative", {"P": -1}, INVALID, "P must be >= 0", TIGHTENED),
        row("gsr_backward_dc_acc", "R-negative", {"R": -1}, INVALID, "R must be >= 0", TIGHTENED),
        row("gsr_backward_dc_acc", "null-geometry", {"geom_buffer": None}, ALLOC, STATE, TIGHTENED),
        row("gsr_backward_dc_acc", "null-geometry-R-0", {"geom_buffer": None, "R": 0}, ALLOC, STATE, TIGHTENED),
        row("gsr_backward_dc_acc", "null-image", {"image_buffer": None}, ALLOC, STATE, TIGHTENED),
        row("gsr_backward_dc_acc", "null-dL_dpix", {"dL_dpix": None}, INVALID, "null dL_dpix", TIGHTENED),
    ] +
    # ---- gsr_backward_render ----
    [
        row("gsr_backward_render", "P-negative", {"P": -1}, INVALID, "P and R must be >= 0"),
        row("gsr_backward_render", "R-negative", {"R": -1}, INVALID, "P and R must be >= 0"),
        row("gsr_backward_render", "P-0", {"P": 0}, OK),
        row("gsr_backward_render", "R-0", {"R": 0}, OK),
        row("gsr_backward_render", "null-geometry", {"geom_buffer": None}, ALLOC, STATE),
        row("gsr_backward_render", "null-image", {"image_buffer": None}, ALLOC, STATE),
        row("gsr_backward_render", "null-binning", {"binning_buffer": None}, ALLOC, STATE),
        row("gsr_backward_render", "null-dL_dpix", {"dL_dpix": None}, INVALID, "null dL_dpix"),
    ] +
    # ---- gsr_backward_render_views ----
    _batch_rows("gsr_backward_render_views", ("R", "geom_buffers", "binning_buffers", "image_buffers", "dL_dpix"),
                {}) + [
        row("gsr_backward_render_views", "P-0", {"P": 0}, OK),
        row("gsr_backward_render_views", "R-0", {"R": [0, 0]}, OK),
        row("gsr_backward_render_views", "P-negative", {"P": -1}, INVALID, "P must be >= 0", TIGHTENED),
        row("gsr_backward_render_views", "R-negative", {"R": [R, -1]}, INVALID, "R must be >= 0"),
        row("gsr_backward_render_views", "null-geometry", {"geom_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_render_views", "null-binning", {"binning_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_render_views", "null-image", {"image_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_render_views", "null-image-R-0", {"image_buffers": [DEV, None], "R": [0, 0]}, ALLOC, STATE),
        row("gsr_backward_render_views", "null-geometry-R-0", {"geom_buffers": [DEV, None], "R": [0, 0]}, ALLOC,
            STATE, TIGHTENED),
        row("gsr_backward_render_views", "null-dL_dpix", {"dL_dpix": [DEV, None]}, INVALID, GRADIENT),
        row("gsr_backward_render_views", "null-dL_invdepth", {"dL_invdepths": [DEV, None]}, INVALID, GRADIENT),
    ] +
    # ---- gsr_backward_preprocess_views_range (gsr_backward_preprocess_views forwards to it with [0, P)) ----
    _batch_rows("gsr_backward_preprocess_views_range",
                ("R",) + CAMERAS + ("tan_fovx", "tan_fovy", "geom_buffers", "binning_buffers", "dL_dmean2D"), {}) +
    _shared_preprocess_rows("gsr_backward_preprocess_views_range", {}) + [
        row("gsr_backward_preprocess_views_range", "P-0", {"P": 0}, OK),
        row("gsr_backward_preprocess_views_range", "P-negative", {"P": -1}, INVALID, RANGE),
        row("gsr_backward_preprocess_views_range", "range-begin-negative", {"g_begin": -1}, INVALID, RANGE),
        row("gsr_backward_preprocess_views_range", "range-end-past-P", {"g_end": P + 1}, INVALID, RANGE),
        row("gsr_backward_preprocess_views_range", "range-reversed", {"g_begin": 10, "g_end": 5}, INVALID, RANGE),
        row("gsr_backward_preprocess_views_range", "null-geometry", {"geom_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_preprocess_views_range", "null-geometry-R-0", {"geom_buffers": [DEV, None], "R": [0, 0]},
            ALLOC, STATE),
        row("gsr_backward_preprocess_views_range", "null-binning", {"binning_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_preprocess_views_range", "null-dL_dmean2D", {"dL_dmean2D": [DEV, None]}, INVALID, GRADIENT),
        row("gsr_backward_preprocess_views_range", "R-negative", {"R": [R, -1]}, INVALID, "R must be >= 0", TIGHTENED),
    ] + [row("gsr_backward_preprocess_views_range", f"null-{a}", {a: [DEV, None]}, INVALID, CAMERA, TIGHTENED)
         for a in CAMERAS] +
    # ---- gsr_backward_views: the render half's checks, then (nothing to render) the preprocess half's ----
    _batch_rows("gsr_backward_views", ("R", "geom_buffers", "binning_buffers", "image_buffers", "dL_dpix"), {}) +
    _batch_rows("gsr_backward_views", CAMERAS + ("tan_fovx", "tan_fovy", "dL_dmean2D"), NO_RENDER)[2:] +
    _shared_preprocess_rows("gsr_backward_views", NO_RENDER) + [
        row("gsr_backward_views", "P-0", {"P": 0}, OK),
        row("gsr_backward_views", "P-negative", {"P": -1}, INVALID, "P must be >= 0", TIGHTENED),
        row("gsr_backward_views", "R-negative", {"R": [R, -1]}, INVALID, "R must be >= 0"),
        row("gsr_backward_views", "null-geometry", {"geom_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_views", "null-binning", {"binning_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_views", "null-image", {"image_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_views", "null-dL_dpix", {"dL_dpix": [DEV, None]}, INVALID, GRADIENT),
        row("gsr_backward_views", "null-dL_invdepth", {"dL_invdepths": [DEV, None]}, INVALID, GRADIENT),
        row("gsr_backward_views", "null-dL_dmean2D", {**NO_RENDER, "dL_dmean2D": [DEV, None]}, INVALID, GRADIENT),
        row("gsr_backward_views", "null-viewmatrix", {**NO_RENDER, "viewmatrices": [DEV, None]}, INVALID, CAMERA,
            TIGHTENED),
    ] +
    # ---- gsr_backward_camera_views ----
    _batch_rows("gsr_backward_camera_views",
                ("R",) + CAMERAS + ("tan_fovx", "tan_fovy", "geom_buffers", "binning_buffers"), {}) + [
        row("gsr_backward_camera_views", "P-negative", {"P": -1}, INVALID, "P must be >= 0"),
        row("gsr_backward_camera_views", "dc-with-colors_precomp", {"dc": DEV, "M": 15, "colors_precomp": DEV},
            INVALID, ONE_OF),
        row("gsr_backward_camera_views", "dc-null-shs", {"dc": DEV, "M": 15, "shs": None}, INVALID,
            "dc given with M > 0 but shs NULL"),
        row("gsr_backward_camera_views", "R-negative", {"R": [R, -1]}, INVALID, "R must be >= 0"),
        row("gsr_backward_camera_views", "null-geometry", {"geom_buffers": [DEV, None]}, ALLOC, STATE),
        row("gsr_backward_camera_views", "null-binning", {"binning_buffers": [DEV, None]}, ALLOC, STATE),
    ] + [row("gsr_backward_camera_views", f"null-{a}", {a: None}, INVALID, CAM_OUT)
         for a in ("workspace", "dL_dviewmatrix", "dL_dprojmatrix", "dL_dcampos")] +
    [row("gsr_backward_camera_views", f"null-{a}", {a: None}, INVALID, PARAMS)
     for a in ("means3D", "opacities", "scales", "rotations")] +
    [row("gsr_backward_camera_views", f"null-{a}", {a: [DEV, None]}, INVALID, CAMERA) for a in CAMERAS]
)


@pytest.fixture(scope="module")
def lib():
    from diff_gaussian_rasterization import _C
    return _C.lib


def test_no_row_can_launch():
    """A row that is not rejected has P == 0, or renders only and has nothing to render."""
    assert len(ROWS) == len({r.id for r in ROWS})
    for r in ROWS:
        entry, args, rc = r.values[:3]
        if rc == OK:
            nothing = args.get("R") in (0, [0] * V) and entry in RENDER_ONLY
            assert args.get("P") == 0 or nothing, r.id
            assert entry != "gsr_backward_camera_views", r.id


@pytest.mark.parametrize("entry,args,rc,text,mark", ROWS)
def test_backward_argument_checks(lib, entry, args, rc, text, mark):
    got, err = _call(lib, entry, args)
    assert got == rc, f"returned {got} ({err!r}), expected {rc}"
    if rc != OK:
        assert text in err
