"""Host binding of libgsr_hip.so (include/gsr.h) behind the reference's `_C` op surface.

Mirrors the three ops the reference's torch glue exposes
(diff-gaussian-rasterization-npu/rasterize_points.cu:35-244, bound in ext.cpp:15-19):
``rasterize_gaussians``, ``rasterize_gaussians_backward`` and ``mark_visible`` -- same
argument order, same returned tuples, same shape errors.  PyTorch only provides device
memory and the current HIP stream; all compute runs in the HIP library.  There is no
CPU fallback: a missing library, a non-GPU tensor or a HIP failure raises.
"""
import collections
import ctypes
import functools
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgsr_hip.so")

_vp, _i, _f, _b, _sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_bool, ctypes.c_size_t


def _load(path=LIB_PATH):
    """The C ABI of the HIP library at `path` with its ctypes signatures (tests/
    test_binding_signatures.py holds them against include/gsr.h).  The package loads only
    LIB_PATH; tests/test_ref_alpha_exact.py passes its test-only GSR_REF_ALPHA build here."""
    if not os.path.exists(path):
        raise ImportError(
            f"diff_gaussian_rasterization: native library {path} is missing; build it with "
            "`make -C gaussian-splatting-npu_amd` (or __graft_entry__.build()). There is no CPU fallback.")
    lib = ctypes.CDLL(path)
    for n in ("gsr_last_error", "gsr_version"):
        getattr(lib, n).restype = ctypes.c_char_p
        getattr(lib, n).argtypes = []
    for n in ("gsr_geometry_buffer_size", "gsr_binning_buffer_size"):
        getattr(lib, n).restype = _sz
        getattr(lib, n).argtypes = [_i]
    lib.gsr_image_buffer_size.restype = _sz
    lib.gsr_image_buffer_size.argtypes = [_i, _i]
    lib.gsr_mark_visible.argtypes = [_i, _vp, _vp, _vp, _vp, _vp]
    lib.gsr_forward_geometry.argtypes = [_vp, _vp, _i, _i, _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                         _vp, _vp, _f, _f, _b, _b, _vp, _b, _vp, ctypes.POINTER(_i)]
    lib.gsr_forward_render.argtypes = [_vp, _vp, _vp, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _b, _vp]
    lib.gsr_forward_prealloc.argtypes = [_vp, _vp, _vp, _sz, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp,
                                         _vp, _vp, _vp, _vp, _f, _f, _b, _b, _vp, _vp, _vp, _b, _vp,
                                         ctypes.POINTER(_i), ctypes.POINTER(_i)]
    lib.gsr_backward.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp,
                                 _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                 _vp, _b, _b, _vp]
    lib.gsr_forward_prealloc_dc.argtypes = [_vp, _vp, _vp, _sz, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                            _f, _vp, _vp, _vp, _vp, _vp, _f, _f, _b, _b, _vp, _vp, _vp, _b, _vp,
                                            ctypes.POINTER(_i), ctypes.POINTER(_i)]
    lib.gsr_backward_dc.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp,
                                    _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _b, _b, _vp]
    lib.gsr_backward_dc_acc.argtypes = lib.gsr_backward_dc.argtypes[:-1] + [ctypes.c_uint, _vp]
    lib.gsr_backward_views.argtypes = [_i, _i, _i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                       _vp, _vp, _vp, _vp, _vp, _b, _b, ctypes.c_uint, _vp]
    lib.gsr_backward_render.argtypes = [_i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _b, _vp]
    lib.gsr_backward_preprocess_views.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _b, _vp, _vp,
                                                  _vp, _vp, _vp, _vp, _vp, _vp, _vp, _b, _b, ctypes.c_uint, _vp]
    lib.gsr_backward_preprocess_views_range.argtypes = lib.gsr_backward_preprocess_views.argtypes[:-1] + [_i, _i, _vp]
    lib.gsr_backward_render_views.argtypes = [_i, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _b, _vp]
    # the alpha output: its forward pass, and the backward entry points with dL_dalphas after dL_invdepths
    lib.gsr_alpha_views.argtypes = [_i, _i, _i, _vp, _vp, _vp]
    lib.gsr_backward_alpha.argtypes = lib.gsr_backward_dc_acc.argtypes[:27] + [_vp] + \
        lib.gsr_backward_dc_acc.argtypes[27:]
    lib.gsr_backward_views_alpha.argtypes = lib.gsr_backward_views.argtypes[:28] + [_vp] + \
        lib.gsr_backward_views.argtypes[28:]
    lib.gsr_backward_render_views_alpha.argtypes = lib.gsr_backward_render_views.argtypes[:11] + [_vp] + \
        lib.gsr_backward_render_views.argtypes[11:]
    lib.gsr_camera_grad_workspace_size.restype = _sz
    lib.gsr_camera_grad_workspace_size.argtypes = [_i, _i]
    lib.gsr_backward_camera_views.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp,
                                              _vp, _vp, _vp, _vp, _vp, _vp, _vp, _b, _b, _vp, _vp, _vp, _vp, _b, _vp]
    lib.gsr_forward_views.argtypes = [_i, _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                      _vp, _vp, _vp, _vp, _b, _b, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _b, _vp, _vp,
                                      _vp]
    lib.gsr_adam_update.argtypes = [_vp, _vp, _vp, _vp, _vp, _f, _f, _f, _f, _i, _i, _vp]
    lib.gsr_adam_update_multi.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i, _vp]
    lib.gsr_densification_stats.argtypes = [_i, _i, _vp, _vp, _vp, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp]
    lib.gsr_activate_forward.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    lib.gsr_activate_backward.argtypes = [_i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]
    lib.gsr_densify_workspace_size.argtypes = [_i]
    lib.gsr_densify_workspace_size.restype = _sz
    lib.gsr_densify_rows_per_workgroup.argtypes = []
    lib.gsr_densify_plan.argtypes = [_i, _vp, ctypes.c_long, _vp, ctypes.c_long, _vp, _vp, _f, _f, _f, _f, _i, _vp,
                                     ctypes.POINTER(_i), _vp]
    lib.gsr_densify_apply.argtypes = [_i, _i, _i, _i, _i, ctypes.POINTER(_i), _i, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp]
    lib.gsr_union_rows_per_wave.argtypes = []
    lib.gsr_union_workspace_size.argtypes = [_i]
    lib.gsr_union_workspace_size.restype = _sz
    lib.gsr_visibility_pack.argtypes = [_i, _vp, _vp, _vp]
    lib.gsr_union_plan.argtypes = [_i, _i, _vp, _i, ctypes.POINTER(_i), _vp, _vp, _vp, ctypes.POINTER(_i),
                                   ctypes.POINTER(_i), _vp]
    lib.gsr_rows_gather.argtypes = [_i, _i, _i, _i, _i, ctypes.POINTER(_i), _vp, _vp, _vp, _vp]
    lib.gsr_rows_scatter.argtypes = lib.gsr_rows_gather.argtypes
    lib.gsr_debug_sorted_keys.argtypes = [_vp, _vp, _vp, _i, _i, _i, _i, _vp, _vp, _vp, _vp]
    lib.gsr_debug_depth_sort_workspace_size.argtypes = [_i]
    lib.gsr_debug_depth_sort_workspace_size.restype = _sz
    lib.gsr_debug_depth_sort.argtypes = [_vp, _i, _vp, _vp, _vp]
    if hasattr(lib, "gsr_debug_set_depth_wide"):  # (test hooks; absent from libraries built before them)
        lib.gsr_debug_depth_wide.argtypes = []
        lib.gsr_debug_set_depth_wide.argtypes = [_i]
    if hasattr(lib, "gsr_debug_last_depth_passes"):
        lib.gsr_debug_last_depth_passes.argtypes = [_i]
    for n in ("gsr_geometry_layout", "gsr_binning_layout"):
        getattr(lib, n).argtypes = [_i, ctypes.POINTER(_sz), _i]
    lib.gsr_image_layout.argtypes = [_i, _i, ctypes.POINTER(_sz), _i]
    return lib


lib = _load()


def _check(rc):
    if rc != 0:
        raise RuntimeError(f"diff_gaussian_rasterization (HIP): {lib.gsr_last_error().decode()} [status {rc}]")


_contig_cache = {}  # small non-contiguous inputs (the transposed view matrices) -> contiguous copy
# Per device: the last forward's num_rendered.  The next forward pre-allocates its binning buffer
# from it (_binning_capacity), so the native forward can run emission, sorts and render straight
# after the num_rendered read-back instead of returning to Python to allocate (the reference's
# binningBuffer resize lambda, rasterize_points.cu:27-33, rasterizer_impl.cu:286).
_binning_hint = {}
_binning_hint_views = {}  # per device: the last view batch's num_rendered per view
views_reruns = 0  # batched forwards that outgrew their binning buffers and ran a second time


def _binning_capacity(hint):
    """Bytes of the binning buffer a forward pre-allocates for `hint` rendered instances (+25 % and
    64K instances of headroom); 0 without a hint."""
    return lib.gsr_binning_buffer_size(min(int(hint * 1.25) + 65536, 0x7FFFFFFF)) if hint is not None else 0


def _contiguous(t):
    """t.contiguous(), memoised for small tensors: the reference's camera matrices are
    transposed views (scene/cameras.py:86-88) that every call would otherwise copy with a
    separate kernel launch.  Keyed on storage, layout and the in-place version counter."""
    if t.is_contiguous():
        return t
    if t.numel() > 64:
        return t.contiguous()
    key = (t.data_ptr(), t.shape, t.stride(), t._version, t.device)
    hit = _contig_cache.get(key)
    if hit is None:
        if len(_contig_cache) > 256:
            _contig_cache.clear()
        # the entry keeps `t` alive, so its storage cannot be recycled under the same key
        hit = _contig_cache[key] = (t, t.contiguous())
    return hit[1]


def _ptr(t, name, device):
    """Device pointer of a float32 tensor, or None for an absent (empty) input -- the
    reference passes `.data<float>()` of `torch.Tensor([])`, i.e. nullptr."""
    if t is None or t.numel() == 0:
        return None, None
    if t.device != device:
        raise RuntimeError(f"{name} must be on {device}, got {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    t = _contiguous(t)
    return t.data_ptr(), t


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def _require_gpu(t):
    if t.device.type != "cuda":
        raise RuntimeError("diff_gaussian_rasterization runs on the GPU only (HIP); got a tensor on "
                           f"{t.device}. There is no CPU path.")


def _sh_split(sh, dc, P=None):
    """(M, has_dc): M = sh.size(1) -- with dc, the number of REST coefficients (0 if sh is empty).
    With P (the forwards), dc's shape is checked."""
    M = sh.size(1) if sh is not None and sh.numel() != 0 and sh.size(0) != 0 else 0
    has_dc = dc is not None and dc.numel() != 0
    if has_dc and P is not None and (dc.dim() != 3 or dc.size(0) != P or dc.size(1) != 1 or dc.size(2) != 3):
        raise RuntimeError("dc must have dimensions (num_points, 1, 3)")
    return M, has_dc


# The per-view block of the batched entry points: R[] (host ints), `cams` = (viewmatrices[],
# projmatrices[], campos[], tan_fovx[], tan_fovy[]) and the views' radii[] / geom[] / binning[] buffers.
_Views = collections.namedtuple("_Views", "R cams radii geoms bins")


class _Call:
    """The native arguments of one Python call on `dev`: device pointers of checked tensors, host
    arrays of them, and the argument blocks the rasterizer entry points share.  `keep` holds every
    tensor pointed into (a contiguous copy made here must outlive the launch's enqueue)."""

    def __init__(self, dev):
        self.dev = dev
        self.keep = []

    def p(self, t, name):
        """_ptr(t): the device pointer of a float32 tensor on `dev`, NULL for an absent one."""
        ptr, tt = _ptr(t, name, self.dev)
        self.keep.append(tt)
        return ptr

    def array(self, ts, name=None):
        """A host array of the device pointers of `ts` (a list, or a tensor's slices along dim 0): NULL
        for None and for an empty tensor; with `name`, every tensor through `p`."""
        if name is not None:
            return (_vp * len(ts))(*[self.p(t, name) for t in ts])
        self.keep.append(ts)
        return (_vp * len(ts))(*[None if t is None or t.numel() == 0 else t.data_ptr() for t in ts])

    def gaussians(self, means3D, dc, sh, colors, opacities, scales, scale_modifier, rotations, cov3D_precomp):
        """The Gaussians as every rasterizer entry point takes them after its sizes: means3D, dc, shs,
        colors_precomp, opacities, scales, scale_modifier, rotations, cov3D_precomp."""
        return (self.p(means3D, "means3D"), self.p(dc, "dc"), self.p(sh, "sh"), self.p(colors, "colors_precomp"),
                self.p(opacities, "opacities"), self.p(scales, "scales"), float(scale_modifier),
                self.p(rotations, "rotations"), self.p(cov3D_precomp, "cov3D_precomp"))

    def cameras(self, viewmatrices, projmatrices, campos, tan_fovx, tan_fovy):
        """_Views.cams of V views (per-view lists, or stacked tensors for the matrices and campos)."""
        V = len(tan_fovx)
        return (self.array(viewmatrices, "viewmatrix"), self.array(projmatrices, "projmatrix"),
                self.array(campos, "campos"), (_f * V)(*[float(x) for x in tan_fovx]),
                (_f * V)(*[float(x) for x in tan_fovy]))

    def views(self, viewmatrices, projmatrices, campos, tan_fovx, tan_fovy, Rs, geomBuffers, binningBuffers,
              radii=None):
        """The per-view block of a batched backward, built once per Python call."""
        return _Views((_i * len(Rs))(*[int(x) for x in Rs]),
                      self.cameras(viewmatrices, projmatrices, campos, tan_fovx, tan_fovy),
                      None if radii is None else self.array(radii), self.array(geomBuffers),
                      self.array(binningBuffers))


def _check_out(out, lead, P, H, W, dev):
    """out= of the forwards: (color, radii, invdepth) of shapes lead + (3,H,W) / (P,) / (1,H,W)."""
    for t, shape, dt in zip(out, ((3, H, W), (P,), (1, H, W)), (torch.float32, torch.int32, torch.float32)):
        shape = lead + shape
        if tuple(t.shape) != shape or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise RuntimeError(f"out: expected a contiguous {dt} tensor of shape {shape} on {dev}")
    return out


def rasterize_gaussians(background, means3D, colors, opacity, scales, rotations, scale_modifier, cov3D_precomp,
                        viewmatrix, projmatrix, tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                        prefiltered, antialiasing, debug, dc=None, out=None):
    """RasterizeGaussiansNPU (rasterize_points.cu:35-124).  `dc` (P,1,3): the separate-DC form of
    the accelerated upstream op (coefficient 0 apart from the rest in `sh`), selected by train.py
    together with SparseGaussianAdam (train.py:37-41, gaussian_renderer/__init__.py:82-100).
    `out` (color (3,H,W), radii (P,), invdepth (1,H,W)): caller-provided outputs, e.g. slices of a
    multi-view batch (MultiViewRasterizer) -- written in full."""
    if means3D.ndimension() != 2 or means3D.size(1) != 3:
        raise RuntimeError("means3D must have dimensions (num_points, 3)")
    _require_gpu(means3D)
    dev = means3D.device
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    empty = lambda: torch.empty((0,), dtype=torch.uint8, device=dev)  # noqa: E731
    if P == 0:
        radii = torch.zeros((P,), dtype=torch.int32, device=dev)
        out_invdepth = torch.zeros((1, H, W), dtype=torch.float32, device=dev)
        out_color = torch.zeros((3, H, W), dtype=torch.float32, device=dev)
        return 0, out_color, radii, empty(), empty(), empty(), out_invdepth

    # every element of these is written by the HIP forward (radii by preprocess, pixels by render)
    if out is not None:
        out_color, radii, out_invdepth = _check_out(out, (), P, H, W, dev)
    else:
        radii = torch.empty((P,), dtype=torch.int32, device=dev)
        out_invdepth = torch.empty((1, H, W), dtype=torch.float32, device=dev)
        out_color = torch.empty((3, H, W), dtype=torch.float32, device=dev)
    M, _ = _sh_split(sh, dc, P)
    a = _Call(dev)
    geom = torch.empty((lib.gsr_geometry_buffer_size(P),), dtype=torch.uint8, device=dev)
    img = torch.empty((lib.gsr_image_buffer_size(W, H),), dtype=torch.uint8, device=dev)
    stream = _stream(dev)
    nr = ctypes.c_int(0)
    rendered = ctypes.c_int(0)
    cap = _binning_capacity(_binning_hint.get(dev))
    binning = torch.empty((cap,), dtype=torch.uint8, device=dev) if cap else None
    bg_p = a.p(background, "bg")
    gauss = a.gaussians(means3D, dc, sh, colors, opacity, scales, scale_modifier, rotations, cov3D_precomp)
    _check(lib.gsr_forward_prealloc_dc(
        geom.data_ptr(), img.data_ptr(), binning.data_ptr() if cap else None, cap, P, int(degree), M, bg_p, W, H,
        *gauss, a.p(viewmatrix, "viewmatrix"), a.p(projmatrix, "projmatrix"), a.p(campos, "campos"),
        float(tan_fovx), float(tan_fovy), bool(prefiltered), bool(antialiasing), out_color.data_ptr(),
        out_invdepth.data_ptr(), radii.data_ptr(), bool(debug), stream, ctypes.byref(nr), ctypes.byref(rendered)))
    L = nr.value
    _binning_hint[dev] = L
    need = lib.gsr_binning_buffer_size(L)
    if rendered.value:
        binning = binning[:need]  # a view: the backward re-derives the layout from num_rendered
    else:  # first call on this device, or the scene grew past the headroom
        binning = torch.empty((need,), dtype=torch.uint8, device=dev)
        _check(lib.gsr_forward_render(geom.data_ptr(), binning.data_ptr(), img.data_ptr(), P, L, bg_p, W, H,
                                      gauss[3], out_color.data_ptr(), out_invdepth.data_ptr(), radii.data_ptr(),
                                      bool(debug), stream))
    return L, out_color, radii, geom, binning, img, out_invdepth


def rasterize_gaussians_views(background, means3D, colors, opacity, scales, rotations, scale_modifier,
                              cov3D_precomp, viewmatrices, projmatrices, tan_fovx, tan_fovy, image_height,
                              image_width, sh, degree, campos, prefiltered, antialiasing, debug, dc=None, out=None):
    """rasterize_gaussians over a batch of V views of the same Gaussians (gsr_forward_views: every
    stage of the views' binning prefix and their render as one launch per stage, grid.y = view).  Per-view lists of camera
    arguments; `out` = (colors (V,3,H,W), radii (V,P), invdepths (V,1,H,W)) -- written in full.
    Returns per-view lists (num_rendered, geomBuffer, binningBuffer, imageBuffer); each view's
    results are bit-identical to rasterize_gaussians on that view."""
    _require_gpu(means3D)
    dev = means3D.device
    P, H, W = means3D.size(0), int(image_height), int(image_width)
    V = len(viewmatrices)
    colors_out, radii_out, inv_out = _check_out(out, (V,), P, H, W, dev)
    if P == 0:
        colors_out.zero_()
        radii_out.zero_()
        inv_out.zero_()
        e = torch.empty((0,), dtype=torch.uint8, device=dev)
        return [0] * V, [e] * V, [e] * V, [e] * V
    M, _ = _sh_split(sh, dc, P)
    a = _Call(dev)
    gsz, isz = lib.gsr_geometry_buffer_size(P), lib.gsr_image_buffer_size(W, H)
    geoms = [torch.empty((gsz,), dtype=torch.uint8, device=dev) for _ in range(V)]
    imgs = [torch.empty((isz,), dtype=torch.uint8, device=dev) for _ in range(V)]
    # every view's capacity from the LARGEST num_rendered of the previous batch on this device (+25 %
    # and 64K instances): the hint is not keyed by camera, and a training loop deals different
    # cameras to the batch's slots every step, so a per-slot hint would overflow (and rerun the
    # whole batch) whenever a slot's new view renders more than its old one did
    hints = _binning_hint_views.get(dev)
    cap = _binning_capacity(max(hints) if hints else _binning_hint.get(dev))
    bins = [torch.empty((cap,), dtype=torch.uint8, device=dev) if cap else None for _ in range(V)]
    head = (V, P, int(degree), M, a.p(background, "bg"), W, H,
            *a.gaussians(means3D, dc, sh, colors, opacity, scales, scale_modifier, rotations, cov3D_precomp),
            *a.cameras(viewmatrices, projmatrices, campos, tan_fovx, tan_fovy), bool(prefiltered), bool(antialiasing),
            a.array(geoms), a.array(imgs))
    outs = (a.array(colors_out), a.array(inv_out), a.array(radii_out), bool(debug), _stream(dev))
    nr = (_i * V)()
    rendered = (_i * V)()

    def run(bins):
        _check(lib.gsr_forward_views(*head, a.array(bins), (_sz * V)(*[0 if b is None else b.numel() for b in bins]),
                                     *outs, nr, rendered))

    run(bins)
    Ls = [int(nr[v]) for v in range(V)]
    _binning_hint[dev] = max(Ls)
    _binning_hint_views[dev] = Ls
    if all(rendered[v] for v in range(V)):
        bins = [bins[v][:lib.gsr_binning_buffer_size(Ls[v])] for v in range(V)]  # views: the backward re-derives
    else:  # first call on this device, or the scene grew past the headroom: the batch again, exact buffers
        global views_reruns
        views_reruns += 1
        bins = [torch.empty((lib.gsr_binning_buffer_size(L),), dtype=torch.uint8, device=dev) for L in Ls]
        run(bins)
        if not all(rendered[v] for v in range(V)) or [int(nr[v]) for v in range(V)] != Ls:
            raise RuntimeError("diff_gaussian_rasterization (HIP): the repeated batch did not reproduce num_rendered")
    return Ls, geoms, bins, imgs


def render_alpha(imgBuffers, H, W, out=None):
    """gsr_alpha_views: alpha = 1 - final_T of V views, (V,1,H,W) float32, from the image state of
    their forwards (a list of imageBuffers of one image size, all on one GPU).  A view whose forward
    had no Gaussians (P == 0: an empty imageBuffer) gets zeros.  `out`: a contiguous float32
    (V,1,H,W) tensor on that GPU, written in full."""
    V, H, W = len(imgBuffers), int(H), int(W)
    if not 1 <= V <= 16:
        raise RuntimeError(f"render_alpha: 1 to 16 views, got {V}")
    dev = imgBuffers[0].device
    _require_gpu(imgBuffers[0])
    need = lib.gsr_image_buffer_size(W, H)
    for t in imgBuffers:
        if t.device != dev or t.dtype != torch.uint8 or not t.is_contiguous() or t.numel() not in (0, need):
            raise RuntimeError("render_alpha: imageBuffers must be the forward's uint8 state of a "
                               f"{H}x{W} image on {dev}")
    if out is None:
        out = torch.empty((V, 1, H, W), dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (V, 1, H, W) or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous():
        raise RuntimeError(f"out: expected a contiguous {torch.float32} tensor of shape {(V, 1, H, W)} on {dev}")
    live = [v for v in range(V) if imgBuffers[v].numel()]
    for v in range(V):
        if not imgBuffers[v].numel():
            out[v].zero_()
    if live and H * W:
        a = _Call(dev)
        with torch.cuda.device(dev):
            _check(lib.gsr_alpha_views(len(live), W, H, a.array([imgBuffers[v] for v in live]),
                                       a.array([out[v] for v in live]), _stream(dev)))
    return out


def _alpha_grad(t, H, W, dev):
    """One view's dL_dout_alpha, checked as dL_dout_color is (device, dtype; a contiguous copy if it
    is strided) and for its shape, (1,H,W) or (H,W): the float32 tensor whose pointer the backward
    takes, or None for an absent one."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in ((1, H, W), (H, W)):
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"dL_dout_alpha must have shape {(1, H, W)}, got {got}")
    if t.device != dev:
        raise RuntimeError(f"dL_dout_alpha must be on {dev}, got {t.device}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"dL_dout_alpha must be float32, got {t.dtype}")
    return t.contiguous()


def _alpha_grads(ts, V, H, W, dev):
    """dL_dout_alpha of a batch -- a list of V per-view gradients with None for a view without one, or
    one stacked (V,1,H,W) tensor -- as a list of checked tensors / None; None if no view has one."""
    if ts is None:
        return None
    if isinstance(ts, torch.Tensor):
        if tuple(ts.shape) != (V, 1, H, W):
            raise RuntimeError(f"dL_dout_alpha must have shape {(V, 1, H, W)}, got {tuple(ts.shape)}")
    elif len(ts) != V:
        raise RuntimeError(f"dL_dout_alpha must have one entry per view ({V}), got {len(ts)}")
    out = [_alpha_grad(ts[v], H, W, dev) for v in range(V)]
    return out if any(t is not None for t in out) else None


# The eight parameter gradients of the backward ops: accumulate= key, gsr.h GSR_ACC_* bit, and one
# Gaussian's gradient as a function of M (its floats per Gaussian are the product; the gradient is
# viewed as (P,) + that).  Fresh gradients are consecutive slices of ONE buffer in this order, which
# starts with multiview.PARAM_ORDER / PARAM_ORDER_DC (means3D | [dc] | sh | opacity | scales |
# rotations): autograd keeps these views as the leaves' .grad, so a multi-GPU step all-reduces the
# buffer in place instead of gathering and scattering 236 B per Gaussian around the collective.
# cov3D and colors_precomp follow, for the single view and the batch alike.
_GRADS = (("means3D", 1, lambda M: (3,)), ("dc", 2, lambda M: (1, 3)), ("sh", 4, lambda M: (M, 3)),
          ("opacities", 8, lambda M: (1,)), ("scales", 16, lambda M: (3,)), ("rotations", 32, lambda M: (4,)),
          ("cov3D_precomp", 64, lambda M: (6,)), ("colors_precomp", 128, lambda M: (3,)))
ACC_BITS = {name: bit for name, bit, _ in _GRADS}  # accumulate= keys -> GSR_ACC_* bits
# The order after dL_dmeans2D of the tuple the backward ops return (dL_ddc only with dc), and of the
# gradient pointers the batched entry points take.
_RESULT_ORDER = ("colors_precomp", "opacities", "means3D", "cov3D_precomp", "dc", "sh", "scales", "rotations")


@functools.lru_cache(maxsize=16)
def _grad_shapes(P, M):
    """{key: (shape, its contiguous strides, floats)} of the _GRADS gradients of P Gaussians (the
    host path of every backward: worked out once per size)."""
    out = {}
    for name, _, row in _GRADS:
        shape = (P,) + row(M)
        strides = tuple(math.prod(shape[d + 1:]) for d in range(len(shape)))
        out[name] = (shape, strides, math.prod(shape))
    return out


def _check_accumulate(accumulate, shapes, has_dc, dev):
    """accumulate= of a backward op as a dict, every target checked against its gradient's size."""
    acc = dict(accumulate or {})
    for k, t in acc.items():
        if k not in shapes:
            raise RuntimeError(f"accumulate: unknown gradient {k!r}")
        n = shapes[k][2]
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != n:
            raise RuntimeError(f"accumulate[{k!r}] must be a contiguous float32 tensor of {n} elements on {dev}")
    if "dc" in acc and not has_dc:
        raise RuntimeError("accumulate['dc'] given without dc")
    return acc


def _param_grads(P, M, has_dc, accumulate, dev):
    """The parameter gradients a backward writes: ({key: tensor, None for dc without dc}, the checked
    accumulate dict, its GSR_ACC_* mask).  A key of `accumulate` gets the caller's target, the
    others consecutive pieces of one fresh buffer, in _GRADS order (the kernel writes every element,
    zeros for culled Gaussians)."""
    shapes = _grad_shapes(P, M)
    acc = _check_accumulate(accumulate, shapes, has_dc, dev)
    fresh = [k for k in shapes if k not in acc and (has_dc or k != "dc")]
    buf = torch.empty((sum(shapes[k][2] for k in fresh),), dtype=torch.float32, device=dev)
    r, off = {}, 0
    for k, (shape, strides, n) in shapes.items():
        if k in fresh:
            r[k] = buf.as_strided(shape, strides, off)
            off += n
        else:
            r[k] = acc[k].view(shape) if k in acc else None
    return r, acc, sum(ACC_BITS[k] for k in acc)


def _grad_ptrs(r, M):
    """The gradients' device pointers in _RESULT_ORDER (NULL: dL_ddc without dc, dL_dsh for M = 0)."""
    return [None if r[k] is None or (k == "sh" and not M) else r[k].data_ptr() for k in _RESULT_ORDER]


def _grad_result(dL_dmeans2D, r, acc, has_dc):
    """The backward ops' tuple: None in place of a gradient the kernel added into its target."""
    return (dL_dmeans2D,) + tuple(None if k in acc else r[k] for k in _RESULT_ORDER if has_dc or k != "dc")


def rasterize_gaussians_backward(background, means3D, radii, colors, opacities, scales, rotations, scale_modifier,
                                 cov3D_precomp, viewmatrix, projmatrix, tan_fovx, tan_fovy, dL_dout_color,
                                 dL_dout_invdepth, sh, degree, campos, geomBuffer, R, binningBuffer, imageBuffer,
                                 antialiasing, debug, dc=None, accumulate=None, dL_dout_alpha=None):
    """RasterizeGaussiansBackwardNPU (rasterize_points.cu:126-223).  With `dc` (the separate-DC
    form) the result carries dL_ddc (P,1,3) before dL_dsh, as the accelerated upstream op returns
    it: (dL_dmeans2D, dL_dcolors, dL_dopacity, dL_dmeans3D, dL_dcov3D, dL_ddc, dL_dsh, dL_dscales,
    dL_drotations).

    accumulate: optional {ACC_BITS key: tensor} -- the kernel ADDS that input's gradient into the
    given contiguous float32 tensor of the input's size (gsr_backward_dc_acc) and the result holds
    None in its place.

    dL_dout_alpha (1,H,W): the gradient on render_alpha's output of this view (gsr_backward_alpha);
    None is the call without it."""
    _require_gpu(means3D)
    dev = means3D.device
    P = means3D.size(0)
    H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    dL_dout_alpha = _alpha_grad(dL_dout_alpha, H, W, dev)
    M, has_dc = _sh_split(sh, dc)
    # Render-pass gradients (one allocation): mean2D 3 | conic 4 | invdepth 1.
    # The HIP backward writes every element (no atomics, no pre-zeroing needed).
    rbuf = torch.empty((P * 8,), dtype=torch.float32, device=dev)
    dL_dmeans2D = rbuf[0:3 * P].view(P, 3)
    dL_dconic = rbuf[3 * P:7 * P].view(P, 2, 2)
    has_inv = dL_dout_invdepth is not None and dL_dout_invdepth.numel() != 0 and dL_dout_invdepth.size(0) != 0
    dL_dinvdepths = rbuf[7 * P:8 * P].view(P, 1)
    r, acc, mask = _param_grads(P, M, has_dc, accumulate, dev)
    if P == 0:
        return _grad_result(dL_dmeans2D, r, acc, has_dc)
    a = _Call(dev)
    g_color, g_opacity, *g_rest = _grad_ptrs(r, M)
    if dL_dout_alpha is None:
        entry, g_alpha = lib.gsr_backward_dc_acc, ()
    else:
        entry, g_alpha = lib.gsr_backward_alpha, (a.p(dL_dout_alpha, "dL_dout_alpha"),)
    _check(entry(
        P, int(degree), M, int(R), a.p(background, "bg"), W, H,
        *a.gaussians(means3D, dc, sh, colors, opacities, scales, scale_modifier, rotations, cov3D_precomp),
        a.p(viewmatrix, "viewmatrix"), a.p(projmatrix, "projmatrix"), a.p(campos, "campos"), float(tan_fovx),
        float(tan_fovy), radii.data_ptr(), geomBuffer.data_ptr(),
        binningBuffer.data_ptr() if binningBuffer.numel() else None, imageBuffer.data_ptr(),
        a.p(dL_dout_color, "dL_dout_color"), a.p(dL_dout_invdepth, "dL_dout_invdepth") if has_inv else None,
        *g_alpha, dL_dmeans2D.data_ptr(), dL_dconic.data_ptr(), g_opacity, g_color,
        dL_dinvdepths.data_ptr() if has_inv else None, *g_rest, bool(antialiasing), bool(debug), mask, _stream(dev)))
    return _grad_result(dL_dmeans2D, r, acc, has_dc)


def _backward_views(render, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp,
                    viewmatrices, projmatrices, tan_fovx, tan_fovy, W, H, sh, degree, campos, geomBuffers, Rs,
                    binningBuffers, has_inv, antialiasing, debug, dc, accumulate, on_chunk):
    """The batched backward behind rasterize_gaussians_backward_views (render = (background,
    imageBuffers, dL_dout_colors, dL_dout_invdepths or None, dL_dout_alphas: None or the checked
    per-view list of _alpha_grads, which selects the *_alpha entry points): the views' BACKWARD::render runs here)
    and rasterize_gaussians_preprocess_backward_views (render = None: it already ran).  Without
    on_chunk one native call (gsr_backward_views / gsr_backward_preprocess_views); with on_chunk =
    (chunks, fn) gsr_backward_render_views if `render`, then gsr_backward_preprocess_views_range over
    `chunks` Gaussian ranges (multiples of 256, the batched kernel's workgroup width), fn(g0, g1,
    grads) after each."""
    _require_gpu(means3D)
    dev = means3D.device
    P, V = means3D.size(0), len(geomBuffers)
    M, has_dc = _sh_split(sh, dc)
    dL_dmeans2D = torch.empty((V, P, 3), dtype=torch.float32, device=dev)
    r, acc, mask = _param_grads(P, M, has_dc, accumulate, dev)
    a = _Call(dev)
    vb = a.views(viewmatrices, projmatrices, campos, tan_fovx, tan_fovy, Rs, geomBuffers, binningBuffers, radii)
    sizes = (V, P, int(degree), M, vb.R)
    gauss = a.gaussians(means3D, dc, sh, colors, opacities, scales, scale_modifier, rotations, cov3D_precomp)
    state = (*vb.cams, vb.radii, vb.geoms, vb.bins)
    grads = (a.array(dL_dmeans2D), *_grad_ptrs(r, M), bool(antialiasing), bool(debug), mask)
    if render is not None:
        background, imageBuffers, dL_dout_colors, dL_dout_invdepths, dL_dout_alphas = render
        frame = (a.p(background, "bg"), W, H)
        pix = (a.array(imageBuffers), a.array(dL_dout_colors, "dL_dout_color"),
               a.array(dL_dout_invdepths, "dL_dout_invdepth") if has_inv else None)
        both, half = lib.gsr_backward_views, lib.gsr_backward_render_views
        if dL_dout_alphas is not None:
            pix += (a.array(dL_dout_alphas, "dL_dout_alpha"),)
            both, half = lib.gsr_backward_views_alpha, lib.gsr_backward_render_views_alpha
        if on_chunk is None:
            _check(both(*sizes, *frame, *gauss, *state, *pix, *grads, _stream(dev)))
            return _grad_result(dL_dmeans2D, r, acc, has_dc)
        _check(half(V, P, vb.R, *frame, vb.geoms, vb.bins, *pix, bool(debug), _stream(dev)))
    preprocess = (*sizes, int(W), int(H), *gauss, *state, bool(has_inv), *grads)
    if on_chunk is None:
        _check(lib.gsr_backward_preprocess_views(*preprocess, _stream(dev)))
        return _grad_result(dL_dmeans2D, r, acc, has_dc)
    chunks, fn = on_chunk
    step = max(256, -(-P // max(1, int(chunks)) // 256) * 256)
    given = {k: t for k, t in r.items() if t is not None}
    for g0 in range(0, P, step):
        g1 = min(P, g0 + step)
        _check(lib.gsr_backward_preprocess_views_range(*preprocess, g0, g1, _stream(dev)))
        fn(g0, g1, given)
    return _grad_result(dL_dmeans2D, r, acc, has_dc)


def rasterize_gaussians_backward_views(background, means3D, radii, colors, opacities, scales, rotations,
                                       scale_modifier, cov3D_precomp, viewmatrices, projmatrices, tan_fovx, tan_fovy,
                                       dL_dout_colors, dL_dout_invdepths, sh, degree, campos, geomBuffers, Rs,
                                       binningBuffers, imageBuffers, antialiasing, debug, dc=None, accumulate=None,
                                       on_chunk=None, dL_dout_alpha=None):
    """Backward of a batch of V views (gsr_backward_views): per-view lists of the forward's state
    (radii (P,), camera, buffers, num_rendered) and dL_dout_colors (V,3,H,W), dL_dout_invdepths
    (V,1,H,W) or None.  Returns (dL_dmeans2D (V,P,3), dL_dcolors, dL_dopacity, dL_dmeans3D,
    dL_dcov3D, [dL_ddc,] dL_dsh, dL_dscales, dL_drotations): the screen-space gradient per view,
    everything else summed over the views; `accumulate` as in rasterize_gaussians_backward.
    on_chunk = (chunks, fn): the BACKWARD::preprocess runs as `chunks` launches over Gaussian ranges
    (gsr_backward_render_views, then gsr_backward_preprocess_views_range per range) and fn(g0, g1,
    grads) is called after each launch is enqueued, grads = {input name: its gradient tensor (P,...)}
    (the caller's accumulate targets or the fresh buffers): rows [g0, g1) are final from then on in
    stream order (multiview.overlapped_allreduce).
    dL_dout_alpha: the gradients on render_alpha's output (gsr_backward_views_alpha) as a list of V
    (1,H,W) tensors with None for a view without one, or one stacked (V,1,H,W) tensor; None is the
    call without it."""
    V = len(geomBuffers)
    H, W = dL_dout_colors.size(2), dL_dout_colors.size(3)
    dL_dout_alpha = _alpha_grads(dL_dout_alpha, V, H, W, means3D.device)
    has_inv = dL_dout_invdepths is not None and dL_dout_invdepths.numel() != 0
    if dL_dout_colors.shape != (V, 3, H, W) or (has_inv and dL_dout_invdepths.shape != (V, 1, H, W)):
        raise RuntimeError("dL_dout_colors must be (V,3,H,W) and dL_dout_invdepths (V,1,H,W)")
    return _backward_views((background, imageBuffers, dL_dout_colors, dL_dout_invdepths, dL_dout_alpha), means3D,
                           radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                           tan_fovx, tan_fovy, W, H, sh, degree, campos, geomBuffers, Rs, binningBuffers, has_inv,
                           antialiasing, debug, dc, accumulate, on_chunk)


def rasterize_gaussians_render_backward(background, P, R, geomBuffer, binningBuffer, imageBuffer, dL_dout_color,
                                        dL_dout_invdepth, debug, dL_dout_alpha=None):
    """BACKWARD::render of one view (gsr_backward_render): its per-(tile, Gaussian) gradient
    records into binningBuffer, for rasterize_gaussians_preprocess_backward_views later.
    dL_dout_alpha (1,H,W): the gradient on render_alpha's output of this view
    (gsr_backward_render_views_alpha with one view); None is the call without it."""
    a = _Call(dL_dout_color.device)
    H, W = dL_dout_color.size(1), dL_dout_color.size(2)
    has_inv = dL_dout_invdepth is not None and dL_dout_invdepth.numel() != 0
    dL_dout_alpha = _alpha_grad(dL_dout_alpha, H, W, a.dev)
    if dL_dout_alpha is not None:
        one = lambda t, name=None: a.array([t], name)  # noqa: E731
        _check(lib.gsr_backward_render_views_alpha(
            1, int(P), (_i * 1)(int(R)), a.p(background, "bg"), W, H, one(geomBuffer),
            one(binningBuffer), one(imageBuffer), one(dL_dout_color, "dL_dout_color"),
            one(dL_dout_invdepth, "dL_dout_invdepth") if has_inv else None, one(dL_dout_alpha, "dL_dout_alpha"),
            bool(debug), _stream(a.dev)))
        return has_inv
    _check(lib.gsr_backward_render(int(P), int(R), a.p(background, "bg"), W, H, geomBuffer.data_ptr(),
                                   binningBuffer.data_ptr() if binningBuffer.numel() else None,
                                   imageBuffer.data_ptr(), a.p(dL_dout_color, "dL_dout_color"),
                                   a.p(dL_dout_invdepth, "dL_dout_invdepth"), bool(debug), _stream(a.dev)))
    return has_inv


def rasterize_gaussians_preprocess_backward_views(means3D, radii, colors, opacities, scales, rotations,
                                                  scale_modifier, cov3D_precomp, viewmatrices, projmatrices,
                                                  tan_fovx, tan_fovy, image_height, image_width, sh, degree, campos,
                                                  geomBuffers, Rs, binningBuffers, has_invdepth, antialiasing, debug,
                                                  dc=None, accumulate=None, on_chunk=None):
    """BACKWARD::preprocess of V views whose render backward already ran
    (gsr_backward_preprocess_views); returns what rasterize_gaussians_backward_views returns;
    on_chunk as there."""
    return _backward_views(None, means3D, radii, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp,
                           viewmatrices, projmatrices, tan_fovx, tan_fovy, image_width, image_height, sh, degree,
                           campos, geomBuffers, Rs, binningBuffers, has_invdepth, antialiasing, debug, dc, accumulate,
                           on_chunk)


def _camera_check(name, t, shape):
    """One camera array (or camera gradient) of backward_camera_views: float32, contiguous, `shape`."""
    if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} must have shape {shape}, got {got}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous, got strides {tuple(t.stride())}")


def camera_grad_workspace_size(V, P):
    """Bytes of gsr_backward_camera_views' workspace for V views of P Gaussians."""
    return int(lib.gsr_camera_grad_workspace_size(int(V), int(P)))


def backward_camera_views(means3D, colors, opacities, scales, rotations, scale_modifier, cov3D_precomp, viewmatrices,
                          projmatrices, campos, tan_fovx, tan_fovy, image_height, image_width, sh, degree,
                          geomBuffers, Rs, binningBuffers, has_invdepth, antialiasing, debug, dc=None,
                          dL_dviewmatrices=None, dL_dprojmatrices=None, dL_dcampos=None):
    """gsr_backward_camera_views: the camera gradient of V views whose render backward already ran
    (before or after their preprocess backward; the state is only read).  viewmatrices and
    projmatrices (V,4,4) and campos (V,3): contiguous float32, stacked as the forward took them
    (row-major as torch stores them); the per-view lists (tan_fovx, tan_fovy, geomBuffers, Rs,
    binningBuffers) and the Gaussians as rasterize_gaussians_preprocess_backward_views takes them.
    Returns (dL_dviewmatrices (V,4,4), dL_dprojmatrices (V,4,4), dL_dcampos (V,3)): fresh tensors, or
    the given ones (contiguous float32 of those shapes), fully written; column 3 of dL/dview and
    column 2 of dL/dproj are zero.  Bitwise reproducible; a view's gradient is the same bits alone or
    in a batch."""
    if not isinstance(viewmatrices, torch.Tensor) or viewmatrices.dim() != 3:
        got = tuple(viewmatrices.shape) if isinstance(viewmatrices, torch.Tensor) else type(viewmatrices).__name__
        raise RuntimeError(f"viewmatrices must have shape (views, 4, 4), got {got}")
    V = viewmatrices.size(0)
    cams = (("viewmatrices", viewmatrices, (V, 4, 4)), ("projmatrices", projmatrices, (V, 4, 4)),
            ("campos", campos, (V, 3)))
    outs = (("dL_dviewmatrices", dL_dviewmatrices, (V, 4, 4)), ("dL_dprojmatrices", dL_dprojmatrices, (V, 4, 4)),
            ("dL_dcampos", dL_dcampos, (V, 3)))
    for name, t, shape in cams:
        _camera_check(name, t, shape)
    for name, t, shape in outs:
        if t is not None:
            _camera_check(name, t, shape)
    if not 1 <= V <= 16:
        raise RuntimeError(f"viewmatrices: 1 to 16 views, got {V}")
    for name, seq in (("tan_fovx", tan_fovx), ("tan_fovy", tan_fovy), ("geomBuffers", geomBuffers), ("Rs", Rs),
                      ("binningBuffers", binningBuffers)):
        if len(seq) != V:
            raise RuntimeError(f"{name} must have one entry per view ({V}), got {len(seq)}")
    dev = _act_device([(name, t) for name, t, _ in cams + outs if t is not None])
    _require_gpu(means3D)
    P = means3D.size(0)
    M, _ = _sh_split(sh, dc)
    grads = [t if t is not None else torch.empty(shape, dtype=torch.float32, device=dev) for _, t, shape in outs]
    a = _Call(dev)
    vb = a.views(viewmatrices, projmatrices, campos, tan_fovx, tan_fovy, Rs, geomBuffers, binningBuffers)
    workspace = torch.empty((camera_grad_workspace_size(V, P),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.gsr_backward_camera_views(
            V, P, int(degree), M, vb.R, int(image_width), int(image_height),
            *a.gaussians(means3D, dc, sh, colors, opacities, scales, scale_modifier, rotations, cov3D_precomp),
            *vb.cams, vb.geoms, vb.bins, bool(has_invdepth), bool(antialiasing), workspace.data_ptr(),
            grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), bool(debug), _stream(dev)))
    return tuple(grads)


def _adam_check(param, param_grad, exp_avg, exp_avg_sq, N, M, dev):
    for name, t in (("param", param), ("param_grad", param_grad), ("exp_avg", exp_avg), ("exp_avg_sq", exp_avg_sq)):
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
            raise RuntimeError(f"adamUpdate: {name} must be a contiguous float32 tensor on {dev}")
        if t.numel() != int(N) * int(M):
            raise RuntimeError(f"adamUpdate: {name} has {t.numel()} elements, expected N*M = {int(N) * int(M)}")


def _adam_visible(visible, N, dev):
    """The visibility mask of the Adam calls, contiguous: N bool flags on `dev`."""
    if visible.device != dev or visible.dtype != torch.bool or visible.numel() != int(N):
        raise RuntimeError(f"adamUpdate: visible must be a bool tensor of N = {int(N)} flags on {dev}")
    return visible.contiguous()


def adam_update_groups(groups, visible, b1, b2, N):
    """One launch for several (param, grad, exp_avg, exp_avg_sq, lr, eps) groups sharing the
    visibility mask of N Gaussians (SparseGaussianAdam.step); M = param.numel() // N per group."""
    if not groups:
        return
    dev = groups[0][0].device
    _require_gpu(groups[0][0])
    visible = _adam_visible(visible, N, dev)
    n = len(groups)
    Ms = [g[0].numel() // int(N) if int(N) else 0 for g in groups]
    for (p, gr, m, v, _, _), M in zip(groups, Ms):
        _adam_check(p, gr, m, v, N, M, dev)
    ptrs = [(_vp * n)(*[g[k].data_ptr() for g in groups]) for k in range(4)]
    _check(lib.gsr_adam_update_multi(n, *ptrs, (_i * n)(*Ms), (_f * n)(*[float(g[4]) for g in groups]),
                                     (_f * n)(*[float(g[5]) for g in groups]), visible.data_ptr(), float(b1),
                                     float(b2), int(N), _stream(dev)))


def adamUpdate(param, param_grad, exp_avg, exp_avg_sq, visible, lr, b1, b2, eps, N, M):
    """The accelerated upstream's `_C.adamUpdate` (called by SparseGaussianAdam.step): Adam on the
    rows of the N Gaussians with visible[i] set (M elements each), in place; no bias correction."""
    _require_gpu(param)
    dev = param.device
    _adam_check(param, param_grad, exp_avg, exp_avg_sq, N, M, dev)
    visible = _adam_visible(visible, N, dev)
    _check(lib.gsr_adam_update(param.data_ptr(), param_grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(),
                               visible.data_ptr(), float(lr), float(b1), float(b2), float(eps), int(N), int(M),
                               _stream(dev)))


def _column_stride(name, t, P, dev):
    """The row stride in floats (>= 1) of a float32 column of P rows -- (P,) or (P,1), any row stride:
    a column of one (P,2) buffer, or a tensor of its own (xyz_gradient_accum, denom)."""
    if t.device != dev or t.dtype != torch.float32 or t.numel() != P or t.dim() not in (1, 2) or t.size(0) != P:
        raise RuntimeError(f"{name} must be a float32 tensor of shape ({P},) or ({P}, 1) on {dev}")
    return max(1, t.stride(0))


def densification_stats(viewspace_grads, radii, max_radii2D, accum, denom, visible_count=None):
    """gsr_densification_stats: train.py's densification statistics of V views in one launch, in
    place and without a host synchronisation.  viewspace_grads (V,P,3) float32 and radii (V,P) int32,
    contiguous; max_radii2D (P,) contiguous; accum / denom (P,) or (P,1) float32 with any row stride
    (columns of one (P,2) buffer, or tensors of their own); visible_count (P,) contiguous or None."""
    _require_gpu(viewspace_grads)
    dev = viewspace_grads.device
    if viewspace_grads.dim() != 3 or viewspace_grads.size(2) != 3:
        raise RuntimeError("viewspace_grads must have dimensions (views, num_points, 3)")
    V, P = viewspace_grads.size(0), viewspace_grads.size(1)
    if tuple(radii.shape) != (V, P) or radii.dtype != torch.int32 or radii.device != dev:
        raise RuntimeError(f"radii must be an int32 tensor of shape {(V, P)} on {dev}")
    if viewspace_grads.dtype != torch.float32:
        raise RuntimeError("viewspace_grads must be float32")
    rows = [_column_stride(name, t, P, dev) for name, t in (("xyz_gradient_accum", accum), ("denom", denom))]
    flat = [("max_radii2D", max_radii2D)] + ([("visible_count", visible_count)] if visible_count is not None else [])
    for name, t in flat:
        if t.device != dev or t.dtype != torch.float32 or tuple(t.shape) != (P,) or not t.is_contiguous():
            raise RuntimeError(f"{name} must be a contiguous float32 tensor of shape ({P},) on {dev}")
    if V == 0 or P == 0:
        return
    grads, radii = viewspace_grads.contiguous(), radii.contiguous()
    with torch.cuda.device(dev):
        _check(lib.gsr_densification_stats(
            V, P, grads.data_ptr(), radii.data_ptr(), max_radii2D.data_ptr(), accum.data_ptr(), rows[0],
            denom.data_ptr(), rows[1], visible_count.data_ptr() if visible_count is not None else None, _stream(dev)))


def _act_check(name, t, P, cols):
    """One array of the activation calls: float32, contiguous, (P, cols) -- (P, 1) or (P,) for
    cols == 1."""
    shapes = ((P, 1), (P,)) if cols == 1 else ((P, cols),)
    if not isinstance(t, torch.Tensor) or tuple(t.shape) not in shapes:
        want = " or ".join(str(s) for s in shapes)
        got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
        raise RuntimeError(f"{name} must have shape {want}, got {got}")
    if t.dtype != torch.float32:
        raise RuntimeError(f"{name} must be float32, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")


def _act_device(named):
    """The one GPU every (name, tensor) of `named` is on (checked after the arrays themselves, so a
    wrong shape or dtype is reported as such wherever the tensor lives)."""
    dev = None
    for name, t in named:
        if t.device.type != "cuda":
            raise RuntimeError(f"{name} must be on the GPU (HIP), got a tensor on {t.device}. There is no CPU path.")
        if dev is not None and t.device != dev:
            raise RuntimeError(f"{name} must be on {dev}, got {t.device}")
        dev = t.device
    return dev


def activate_forward(scaling, rotation, opacity):
    """gsr_activate_forward: (exp(scaling), normalize(rotation), sigmoid(opacity)) -- GaussianModel's
    get_scaling / get_rotation / get_opacity (gaussian_model.py:102-135) -- in one launch.  scaling
    (P,3), rotation (P,4), opacity (P,1) or (P,): contiguous float32 on one GPU.  Returns fresh
    contiguous tensors shaped as the inputs."""
    if not isinstance(scaling, torch.Tensor) or scaling.dim() != 2 or scaling.size(1) != 3:
        raise RuntimeError("scaling must have shape (num_points, 3)")
    P = scaling.size(0)
    named = (("scaling", scaling, 3), ("rotation", rotation, 4), ("opacity", opacity, 1))
    for name, t, cols in named:
        _act_check(name, t, P, cols)
    dev = _act_device([(name, t) for name, t, _ in named])
    scales, rotations, opacities = torch.empty_like(scaling), torch.empty_like(rotation), torch.empty_like(opacity)
    if P != 0:
        with torch.cuda.device(dev):
            _check(lib.gsr_activate_forward(P, scaling.data_ptr(), rotation.data_ptr(), opacity.data_ptr(),
                                            scales.data_ptr(), rotations.data_ptr(), opacities.data_ptr(),
                                            _stream(dev)))
    return scales, rotations, opacities


# accumulate_mask of activate_backward: bit of each group
ACT_ACC_BITS = {"scaling": 1, "rotation": 2, "opacity": 4}


def activate_backward(scales, rotation, opacities, dL_dscales, dL_drotations, dL_dopacities, dL_dscaling,
                      dL_drotation, dL_dopacity, accumulate_mask=0):
    """gsr_activate_backward: the backward of activate_forward from its outputs `scales` and
    `opacities` and the raw `rotation`.  A group (scaling, rotation, opacity) whose incoming gradient
    or destination is None is skipped; the destinations are written in place -- overwritten, or added
    to where the group's ACT_ACC_BITS bit of accumulate_mask is set.  Every tensor given: contiguous
    float32 on one GPU, (P,3) / (P,4) / (P,1) or (P,); destinations may be views at any float offset."""
    groups = (("scales", scales, "dL_dscales", dL_dscales, "dL_dscaling", dL_dscaling, 3),
              ("rotation", rotation, "dL_drotations", dL_drotations, "dL_drotation", dL_drotation, 4),
              ("opacities", opacities, "dL_dopacities", dL_dopacities, "dL_dopacity", dL_dopacity, 1))
    accumulate_mask = int(accumulate_mask)
    if accumulate_mask & ~7:
        raise RuntimeError(f"accumulate_mask has unknown bits: {accumulate_mask}")
    given = [t for g in groups for t in (g[1], g[3], g[5]) if isinstance(t, torch.Tensor)]
    if not given:
        return
    P = given[0].size(0) if given[0].dim() else -1
    named, ptrs = [], [None] * 9
    for j, (n_in, t_in, n_g, t_g, n_d, t_d, cols) in enumerate(groups):
        if t_g is None or t_d is None:
            continue
        for k, (name, t) in enumerate(((n_in, t_in), (n_g, t_g), (n_d, t_d))):
            _act_check(name, t, P, cols)
            named.append((name, t))
            ptrs[3 * k + j] = t.data_ptr()
    if not named:
        return
    dev = _act_device(named)
    if P == 0:
        return
    with torch.cuda.device(dev):
        _check(lib.gsr_activate_backward(P, *ptrs, accumulate_mask, _stream(dev)))


def densify_rows_per_workgroup():
    """Source rows one workgroup of densify_plan's scan covers (tests size their inputs from it)."""
    return int(lib.gsr_densify_rows_per_workgroup())


def densify_plan(accum, denom, scaling, opacity, max_grad, dense_extent, min_opacity, big_extent, N):
    """gsr_densify_plan: decides what GaussianModel.densify_and_prune does with each of the P Gaussians.
    accum / denom (P,) or (P,1) float32 with any row stride (as densification_stats takes them);
    scaling (P,3) and opacity (P,1) or (P,), contiguous float32; big_extent None: no world-size test.
    Returns (workspace, counts): the device workspace densify_apply reads, and the dict
    {"cloned", "split", "pruned", "P_after"}.  One stream synchronisation."""
    _require_gpu(scaling)
    dev = scaling.device
    if scaling.dim() != 2 or scaling.size(1) != 3 or scaling.dtype != torch.float32 or not scaling.is_contiguous():
        raise RuntimeError("scaling must be a contiguous float32 tensor of shape (num_points, 3)")
    P = scaling.size(0)
    if (opacity.device != dev or opacity.dtype != torch.float32 or opacity.numel() != P or opacity.dim() not in (1, 2)
            or opacity.size(0) != P or not opacity.is_contiguous()):
        raise RuntimeError(f"opacity must be a contiguous float32 tensor of shape ({P},) or ({P}, 1) on {dev}")
    rows = [_column_stride(name, t, P, dev) for name, t in (("xyz_gradient_accum", accum), ("denom", denom))]
    if int(N) < 1:
        raise RuntimeError("N must be >= 1")
    counts = (_i * 4)()
    workspace = torch.empty((int(lib.gsr_densify_workspace_size(P)),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        _check(lib.gsr_densify_plan(
            P, accum.data_ptr(), rows[0], denom.data_ptr(), rows[1], scaling.data_ptr(), opacity.data_ptr(),
            float(max_grad), float(dense_extent), float(min_opacity), -1.0 if big_extent is None else float(big_extent),
            int(N), workspace.data_ptr(), counts, _stream(dev)))
    return workspace, {"cloned": counts[0], "split": counts[1], "pruned": counts[2], "P_after": counts[3]}


def densify_apply(workspace, counts, N, names, src, src_state, dst, dst_state, samples, roles=("xyz", "scaling",
                                                                                                "rotation")):
    """gsr_densify_apply: writes the tensors densify_plan planned, every group in one launch.
    workspace, counts: densify_plan's; names: the groups; src / dst: name -> the (P, ...) input and the
    (P_after, ...) output, contiguous float32; src_state / dst_state: name -> (exp_avg, exp_avg_sq) or
    None for a group without optimizer state; samples: (N * split, 3) standard normal draws; roles: the
    names of the position, log-scale and quaternion groups."""
    P = src[names[0]].size(0) if names else 0
    _require_gpu(src[names[0]])
    dev = src[names[0]].device
    P_after, n_split = int(counts["P_after"]), int(counts["split"])
    if (samples.device != dev or samples.dtype != torch.float32 or tuple(samples.shape) != (int(N) * n_split, 3)
            or not samples.is_contiguous()):
        raise RuntimeError(f"samples must be a contiguous float32 tensor of shape ({int(N) * n_split}, 3) on {dev}")
    if workspace.device != dev or workspace.dtype != torch.uint8 or \
            workspace.numel() < int(lib.gsr_densify_workspace_size(P)):
        raise RuntimeError(f"workspace must be densify_plan's uint8 workspace for {P} points on {dev}")
    Ms, cols = [], [[] for _ in range(6)]
    for k in names:
        s, d = src[k], dst[k]
        M = s.numel() // P if P else 0
        ss, ds = src_state.get(k), dst_state.get(k)
        if (ss is None) != (ds is None):
            raise RuntimeError(f"{k}: moments must be given for both the input and the output, or for neither")
        for name, t, rows in [(k, s, P), (f"new {k}", d, P_after)] + ([] if ss is None else [
                (f"{k} exp_avg", ss[0], P), (f"{k} exp_avg_sq", ss[1], P), (f"new {k} exp_avg", ds[0], P_after),
                (f"new {k} exp_avg_sq", ds[1], P_after)]):
            if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous():
                raise RuntimeError(f"densify_apply: {name} must be a contiguous float32 tensor on {dev}")
            if t.size(0) != rows or t.numel() != rows * M:
                raise RuntimeError(f"densify_apply: {name} has shape {tuple(t.shape)}, expected {rows} rows of {M}")
        Ms.append(M)
        for col, t in zip(cols, (s, None if ss is None else ss[0], None if ss is None else ss[1], d,
                                 None if ds is None else ds[0], None if ds is None else ds[1])):
            col.append(t.data_ptr() if t is not None and t.numel() else None)
    n = len(names)
    if P == 0 or P_after == 0:
        return
    role_idx = [names.index(r) for r in roles]
    with torch.cuda.device(dev):
        _check(lib.gsr_densify_apply(
            P, P_after, n_split, int(N), n, (_i * n)(*Ms), *role_idx, *[(_vp * n)(*c) for c in cols],
            samples.data_ptr() if n_split else None, workspace.data_ptr(), _stream(dev)))


def union_rows_per_wave():
    """Gaussians one wave of union_plan covers: its boundaries are multiples of this (or P)."""
    return int(lib.gsr_union_rows_per_wave())


def visibility_words(P):
    """int32 words of one rank's visibility bits for P Gaussians."""
    return (int(P) + 31) // 32


def visibility_pack(count, out=None):
    """gsr_visibility_pack: bit (g & 31) of word (g >> 5) = count[g] > 0 for the contiguous float32 (P,)
    `count`; bits at or beyond P are zero.  Returns the int32 tensor of (P + 31) // 32 words (`out`, if
    given).  Asynchronous."""
    _require_gpu(count)
    dev = count.device
    if count.dtype != torch.float32 or count.dim() != 1 or not count.is_contiguous():
        raise RuntimeError("count must be a contiguous float32 tensor of shape (num_points,)")
    P = count.numel()
    n = visibility_words(P)
    if out is None:
        out = torch.empty((n,), dtype=torch.int32, device=dev)
    elif out.device != dev or out.dtype != torch.int32 or out.numel() != n or not out.is_contiguous():
        raise RuntimeError(f"out must be a contiguous int32 tensor of {n} words on {dev}")
    if P:
        with torch.cuda.device(dev):
            _check(lib.gsr_visibility_pack(P, count.data_ptr(), out.data_ptr(), _stream(dev)))
    return out


def union_plan(words, P, bounds=None, rows=None, mask=None, workspace=None):
    """gsr_union_plan: the union of the ranks' visibility bits as an ascending row list.  words: int32
    (ranks, (P + 31) // 32), contiguous, one visibility_pack row per rank.  bounds: up to 16 Gaussian
    indices, each P or a multiple of union_rows_per_wave().  rows: an int32 (P,) tensor to write the
    list into (allocated if None; only [0, U) is written).  mask: True for a fresh bool (P,) union
    mask, a bool (P,) tensor to write it into, or None.  workspace: a uint8 tensor of
    gsr_union_workspace_size(P) bytes to reuse, or None.  Returns (U, rows, mask, bound_ranks) with
    bound_ranks[k] the number of union rows below bounds[k].  One stream synchronisation."""
    _require_gpu(words)
    dev = words.device
    P = int(P)
    n = visibility_words(P)
    if words.dtype != torch.int32 or words.dim() != 2 or words.size(1) != n or not words.is_contiguous():
        raise RuntimeError(f"words must be a contiguous int32 tensor of shape (ranks, {n})")
    ranks = words.size(0)
    if ranks < 1:
        raise RuntimeError("ranks must be >= 1")
    bounds = [int(b) for b in (bounds or [])]
    if len(bounds) > 16:
        raise RuntimeError("at most 16 boundaries")
    if rows is None:
        rows = torch.empty((P,), dtype=torch.int32, device=dev)
    elif rows.device != dev or rows.dtype != torch.int32 or rows.numel() < P or not rows.is_contiguous():
        raise RuntimeError(f"rows must be a contiguous int32 tensor of {P} elements on {dev}")
    if mask is True:
        mask = torch.empty((P,), dtype=torch.bool, device=dev)
    elif mask is not None and (mask.device != dev or mask.dtype != torch.bool or mask.numel() != P
                               or not mask.is_contiguous()):
        raise RuntimeError(f"mask must be a contiguous bool tensor of {P} elements on {dev}")
    need = int(lib.gsr_union_workspace_size(P))
    if workspace is None:
        workspace = torch.empty((need,), dtype=torch.uint8, device=dev)
    elif workspace.device != dev or workspace.dtype != torch.uint8 or workspace.numel() < need:
        raise RuntimeError(f"workspace must be a uint8 tensor of {need} bytes on {dev}")
    nb = len(bounds)
    U, ranks_out = _i(0), (_i * max(nb, 1))()
    with torch.cuda.device(dev):
        _check(lib.gsr_union_plan(P, ranks, words.data_ptr() if P else None, nb, (_i * max(nb, 1))(*bounds),
                                  workspace.data_ptr() if P else None, rows.data_ptr() if P else None,
                                  mask.data_ptr() if mask is not None and P else None, ctypes.byref(U), ranks_out,
                                  _stream(dev)))
    return int(U.value), rows, mask, [int(ranks_out[k]) for k in range(nb)]


def _rows_move(fn, name, tensors, rows, U, compact, window):
    if not tensors:
        raise RuntimeError(f"{name}: no tensors")
    _require_gpu(tensors[0])
    dev = tensors[0].device
    P = tensors[0].size(0)
    U = int(U)
    Ms = []
    for k, t in enumerate(tensors):
        if t.device != dev or t.dtype != torch.float32 or not t.is_contiguous() or t.dim() < 1 or t.size(0) != P:
            raise RuntimeError(f"{name}: tensor {k} must be a contiguous float32 tensor of {P} rows on {dev}")
        Ms.append(t.numel() // P if P else 0)
    if len(tensors) > 8:
        raise RuntimeError(f"{name}: at most 8 groups")
    if rows.device != dev or rows.dtype != torch.int32 or rows.numel() < U or not rows.is_contiguous():
        raise RuntimeError(f"{name}: rows must be union_plan's int32 list of at least U = {U} rows on {dev}")
    total = U * sum(Ms)  # [group][union row][column]: multiview.compact_layout
    if compact.device != dev or compact.dtype != torch.float32 or compact.numel() < total or not compact.is_contiguous():
        raise RuntimeError(f"{name}: compact must be a contiguous float32 tensor of at least {total} elements on {dev}")
    u0, u1 = (0, U) if window is None else (int(window[0]), int(window[1]))
    n = len(tensors)
    with torch.cuda.device(dev):
        _check(fn(P, U, u0, u1, n, (_i * n)(*Ms), (_vp * n)(*[t.data_ptr() if t.numel() else None for t in tensors]),
                  rows.data_ptr(), compact.data_ptr(), _stream(dev)))


def rows_gather(tensors, rows, U, compact, window=None):
    """gsr_rows_gather: the union rows rows[u0:u1] (window, default all U) of every (P, ...) float32
    tensor into `compact` (layout: multiview.compact_layout), all tensors in one launch.  Asynchronous."""
    _rows_move(lib.gsr_rows_gather, "rows_gather", tensors, rows, U, compact, window)


def rows_scatter(tensors, rows, U, compact, window=None):
    """gsr_rows_scatter: the inverse of rows_gather -- writes the window's union rows of every tensor
    from `compact` and touches no other row.  Asynchronous."""
    _rows_move(lib.gsr_rows_scatter, "rows_scatter", tensors, rows, U, compact, window)


def mark_visible(means3D, viewmatrix, projmatrix):
    """markVisible (rasterize_points.cu:225-244)."""
    _require_gpu(means3D)
    a = _Call(means3D.device)
    P = means3D.size(0)
    present = torch.zeros((P,), dtype=torch.bool, device=a.dev)
    if P != 0:
        _check(lib.gsr_mark_visible(P, a.p(means3D, "means3D"), a.p(viewmatrix, "viewmatrix"),
                                    a.p(projmatrix, "projmatrix"), present.data_ptr(), _stream(a.dev)))
    return present


# ---- parity/debug introspection (tests only) -------------------------------------------------
def _layout(fn, *args, n=64):
    offs = (_sz * n)()
    cnt = fn(*args, offs, n)
    return [offs[i] for i in range(cnt + 1)]


def geometry_layout(P):
    return _layout(lib.gsr_geometry_layout, P)


def image_layout(W, H):
    return _layout(lib.gsr_image_layout, W, H)


def binning_layout(L):
    return _layout(lib.gsr_binning_layout, L)


def sorted_keys(geomBuffer, binningBuffer, imgBuffer, P, L, W, H):
    """Sorted tile|depth keys, sorted Gaussian ids and per-tile ranges of the last forward."""
    dev = geomBuffer.device
    T = ((W + 15) // 16) * ((H + 15) // 16)
    keys = torch.empty((max(L, 0),), dtype=torch.int64, device=dev)
    vals = torch.empty((max(L, 0),), dtype=torch.int32, device=dev)
    ranges = torch.empty((T, 2), dtype=torch.int32, device=dev)
    _check(lib.gsr_debug_sorted_keys(geomBuffer.data_ptr(), binningBuffer.data_ptr() if L else None,
                                     imgBuffer.data_ptr(), P, L, W, H, keys.data_ptr() if L else None,
                                     vals.data_ptr() if L else None, ranges.data_ptr(), _stream(dev)))
    return keys, vals, ranges


def depth_sort(keys):
    """The forward's depth sort on its own (parity helper): the stable order of the u32 keys
    (int32 tensor of bit patterns; -1 = culled, sorted last)."""
    n = keys.numel()
    ids = torch.empty((n,), dtype=torch.int32, device=keys.device)
    if n == 0:
        return ids
    ws = torch.empty((lib.gsr_debug_depth_sort_workspace_size(n),), dtype=torch.uint8, device=keys.device)
    keys = keys.contiguous()
    _check(lib.gsr_debug_depth_sort(keys.data_ptr(), n, ids.data_ptr(), ws.data_ptr(),
                                    _stream(keys.device)))
    return ids


def depth_wide():
    """Test hook: True while this host thread's depth sorts are forced to four 8-bit passes
    (set_depth_wide).  Forwards never set it: a too-wide depth range re-runs that call's sort only."""
    return bool(lib.gsr_debug_depth_wide())


def set_depth_wide(on):
    """Test hook: force (True) or release (False) the four-pass depth sort for this host thread."""
    _check(lib.gsr_debug_set_depth_wide(1 if on else 0))


def grad_record_floats():
    """Floats per per-instance gradient record (10 = 40 B; diagnostics)."""
    return int(lib.gsr_debug_grad_record_floats())


def last_depth_passes(view=0):
    """Test hook: the passes of the final depth sort of view `view` in this thread's last forward (3,
    or 4 when its visible depth range was too wide for three and the sort was re-run)."""
    return int(lib.gsr_debug_last_depth_passes(int(view)))


def fusedssim(C1, C2, img1, img2):
    """The dr_aa extension's SSIM-map op that utils/loss_utils.py:17-30 imports: ssim_map."""
    import fused_ssim
    return fused_ssim.fusedssim(C1, C2, img1, img2, train=False)[0]


def fusedssim_backward(C1, C2, img1, img2, opt_grad):
    """dL/dimg1 of the SSIM map for upstream opt_grad (utils/loss_utils.py:32-37)."""
    import fused_ssim
    _, a, b, c = fused_ssim.fusedssim(C1, C2, img1, img2, train=True)
    return fused_ssim.fusedssim_backward(C1, C2, img1, img2, opt_grad, a, b, c)
