"""Drop-in for the reference's optional `fused_ssim` module (submodule fused-ssim, un-vendored;
train.py:31-35 imports `from fused_ssim import fused_ssim` and uses it at train.py:121-124).

fused_ssim(img1, img2, padding="same", train=True) -> mean SSIM, differentiable w.r.t. img1,
with the semantics of the reference's PyTorch ssim (utils/loss_utils.py:56-86).  The map and its
gradient are computed by the HIP kernels behind include/fused_ssim.h; there is no CPU path.

fused_l1_ssim_loss(img, gt, lambda_dssim=0.2, clamp=False) -> the whole photometric loss of
train.py:119-124, (1 - lambda) L1 + lambda (1 - SSIM), for one image or a batch of views in one
forward and one backward kernel (not part of the reference's module: an opt-in extra).

fused_view_loss(img, gt, lambda_dssim=0.2, clamp=True, exposure=None, alpha_mask=None, invdepth=None,
invdepth_target=None, depth_mask=None, depth_weight=0.0) -> all of train.py:112-141 from the raw
rasterizer outputs: per-camera exposure, clamp, alpha mask, that loss and the inverse-depth L1 term,
differentiable in img, exposure and invdepth (an opt-in extra as well).
"""
import ctypes

import torch

from diff_gaussian_rasterization import _C as _gsr

_lib = _gsr.lib
_vp, _i, _f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
_lib.gsr_ssim_forward.restype = _i
_lib.gsr_ssim_forward.argtypes = [_i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.gsr_ssim_backward.restype = _i
_lib.gsr_ssim_backward.argtypes = [_i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]

allowed_padding = ["same", "valid"]


def _planes(img):
    if img.device.type != "cuda":
        raise RuntimeError(f"fused_ssim runs on the GPU only (HIP); got a tensor on {img.device}")
    if img.dim() < 2:
        raise RuntimeError("images must be (..., H, W)")
    H, W = img.shape[-2], img.shape[-1]
    return (img.numel() // (H * W) if H * W else 0), H, W


def _f32(t):
    return t.detach().float().contiguous()


def fusedssim(C1, C2, img1, img2, train=True):
    """(ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12); the last three are empty if not train."""
    if img1.shape != img2.shape:
        raise RuntimeError("img1 and img2 must have the same shape")
    n, H, W = _planes(img1)
    a, b = _f32(img1), _f32(img2)
    out = torch.empty_like(a)
    parts = [torch.empty_like(a) for _ in range(3)] if train else [torch.empty(0, device=a.device)] * 3
    ptr = [p.data_ptr() if train else None for p in parts]
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        _gsr._check(_lib.gsr_ssim_forward(n, H, W, C1, C2, a.data_ptr(), b.data_ptr(), out.data_ptr(), ptr[0],
                                          ptr[1], ptr[2], stream))
    return (out, *parts)


def fusedssim_backward(C1, C2, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12):
    n, H, W = _planes(img1)
    a, b, g = _f32(img1), _f32(img2), _f32(dL_dmap)
    grad = torch.empty_like(a)
    with torch.cuda.device(a.device):
        stream = torch.cuda.current_stream(a.device).cuda_stream
        _gsr._check(_lib.gsr_ssim_backward(n, H, W, C1, C2, a.data_ptr(), b.data_ptr(), g.data_ptr(),
                                           dm_dmu1.data_ptr(), dm_dsigma1_sq.data_ptr(), dm_dsigma12.data_ptr(),
                                           grad.data_ptr(), stream))
    return grad


class FusedSSIMMap(torch.autograd.Function):
    @staticmethod
    def forward(ctx, C1, C2, img1, img2, padding="same", train=True):
        ssim_map, dm_dmu1, dm_dsigma1_sq, dm_dsigma12 = fusedssim(C1, C2, img1, img2, train)
        if padding == "valid":
            ssim_map = ssim_map[..., 5:-5, 5:-5]
        ctx.save_for_backward(img1.detach(), img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)
        ctx.C1, ctx.C2, ctx.padding, ctx.train = C1, C2, padding, train
        return ssim_map

    @staticmethod
    def backward(ctx, opt_grad):
        img1, img2, dm_dmu1, dm_dsigma1_sq, dm_dsigma12 = ctx.saved_tensors
        if not ctx.train:
            raise RuntimeError("fused_ssim(train=False) keeps no state for a backward pass")
        dL_dmap = opt_grad
        if ctx.padding == "valid":
            dL_dmap = torch.zeros_like(img1)
            dL_dmap[..., 5:-5, 5:-5] = opt_grad
        grad = fusedssim_backward(ctx.C1, ctx.C2, img1, img2, dL_dmap, dm_dmu1, dm_dsigma1_sq, dm_dsigma12)
        return None, None, grad.to(img1.dtype), None, None, None


def fused_ssim(img1, img2, padding="same", train=True):
    C1 = 0.01 ** 2
    C2 = 0.03 ** 2
    assert padding in allowed_padding
    img1 = img1.contiguous()
    ssim_map = FusedSSIMMap.apply(C1, C2, img1, img2, padding, train)
    return ssim_map.mean()


# ---- the whole photometric loss of a batch of views in two kernels -------------------------------
MAX_VIEWS = 16
_sz = ctypes.c_size_t
_lib.gsr_photo_loss_workspace_size.restype = _sz
_lib.gsr_photo_loss_workspace_size.argtypes = [_i, _i, _i, _i]
_lib.gsr_photo_loss_forward.restype = _i
_lib.gsr_photo_loss_forward.argtypes = [_i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]
_lib.gsr_photo_loss_backward.restype = _i
_lib.gsr_photo_loss_backward.argtypes = [_i, _i, _i, _i, _f, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]


def _gt_pointers(gts):
    return (_vp * len(gts))(*[g.data_ptr() for g in gts])


def _ground_truths(gt, x, single):
    """`gt` -- one tensor of img's shape (checked by the caller) or a sequence of V (C,H,W) tensors --
    as the validated list of V detached contiguous float32 tensors on the device of x, the (V,C,H,W) img."""
    if torch.is_tensor(gt):
        gts = [gt] if single else list(gt.unbind(0))
    else:
        gts = list(gt)
    V = x.shape[0]
    if len(gts) != V:
        raise RuntimeError(f"{V} views but {len(gts)} ground-truth images")
    for g in gts:
        if not torch.is_tensor(g) or g.shape != x.shape[1:]:
            raise RuntimeError("every ground-truth image must have the shape of one view of img")
        if g.device != x.device or g.dtype != torch.float32:
            raise RuntimeError(f"ground-truth images must be float32 on {x.device}")
    if x.numel() == 0:
        raise RuntimeError("img is empty")
    return [g.detach().contiguous() for g in gts]


class FusedL1SSIMLoss(torch.autograd.Function):
    """(V,) losses of a contiguous float32 (V,C,H,W) batch against V separate (C,H,W) ground truths.
    `train`: keep the partial planes for a backward."""

    @staticmethod
    def forward(ctx, img, lambda_dssim, clamp, train, *gts):
        V, C, H, W = img.shape
        dev = img.device
        x = img.detach()
        loss = torch.empty((V,), dtype=torch.float32, device=dev)
        parts = [torch.empty_like(x) for _ in range(3)] if train else [None] * 3
        with torch.cuda.device(dev):
            ws = torch.empty((_lib.gsr_photo_loss_workspace_size(V, C, H, W),), dtype=torch.uint8, device=dev)
            _gsr._check(_lib.gsr_photo_loss_forward(
                V, C, H, W, lambda_dssim, int(clamp), x.data_ptr(), _gt_pointers(gts), loss.data_ptr(),
                *[p.data_ptr() if train else None for p in parts], ws.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream))
        if train:
            ctx.save_for_backward(x, *parts, *gts)
        ctx.lambda_dssim, ctx.clamp, ctx.train = lambda_dssim, clamp, train
        return loss

    @staticmethod
    def backward(ctx, dloss):
        if not ctx.train:
            raise RuntimeError("fused_l1_ssim_loss kept no state for a backward pass")
        x, dA, dB, dC, *gts = ctx.saved_tensors
        V, C, H, W = x.shape
        dev = x.device
        g = dloss.detach().to(torch.float32).contiguous()  # stays on the device: the kernel reads it
        grad = torch.empty_like(x)
        with torch.cuda.device(dev):
            _gsr._check(_lib.gsr_photo_loss_backward(
                V, C, H, W, ctx.lambda_dssim, int(ctx.clamp), x.data_ptr(), _gt_pointers(gts), g.data_ptr(),
                dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), grad.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream))
        return (grad, None, None, None) + (None,) * len(gts)


def fused_l1_ssim_loss(img, gt, lambda_dssim=0.2, clamp=False):
    """train.py:119-124 for a batch of views in two HIP kernels (one forward, one backward):

        loss_v = (1 - lambda_dssim) mean|x_v - gt_v| + lambda_dssim (1 - mean SSIM(x_v, gt_v)),

    x = img, or clamp(img, 0, 1) with `clamp`; the means run over the view's C*H*W elements and
    SSIM is fused_ssim's (padding "same").  img: float32 (V,C,H,W) with 1 <= V <= 16, or (C,H,W);
    gt: a tensor of the same shape, or a sequence of V (C,H,W) tensors (they are not stacked).
    Returns the (V,) per-view losses (0-dim for a 3-D img), differentiable with respect to img
    (sign(0) = 0; the clamp passes the gradient for 0 <= img <= 1).  Under torch.no_grad(), or when
    img needs no gradient, nothing is kept for a backward.  GPU only; there is no CPU path."""
    if img.device.type != "cuda":
        raise RuntimeError(f"fused_l1_ssim_loss runs on the GPU only (HIP); got a tensor on {img.device}")
    if img.dim() not in (3, 4):
        raise RuntimeError("img must be (V, C, H, W) or (C, H, W)")
    if img.dtype != torch.float32:
        raise RuntimeError(f"img must be float32, got {img.dtype}")
    single = img.dim() == 3
    if torch.is_tensor(gt) and gt.shape != img.shape:
        raise RuntimeError("img and gt must have the same shape")
    x = img[None] if single else img
    V = x.shape[0]
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"fused_l1_ssim_loss takes 1 to {MAX_VIEWS} views, got {V}")
    gts = _ground_truths(gt, x, single)
    train = torch.is_grad_enabled() and x.requires_grad
    loss = FusedL1SSIMLoss.apply(x.contiguous(), float(lambda_dssim), bool(clamp), train, *gts)
    return loss[0] if single else loss


# ---- the whole per-view loss, from the raw rasterizer outputs, in one forward and one backward ------
_lib.gsr_view_loss_workspace_size.restype = _sz
_lib.gsr_view_loss_workspace_size.argtypes = [_i, _i, _i, _i]
_lib.gsr_view_loss_forward.restype = _i
_lib.gsr_view_loss_forward.argtypes = [_i, _i, _i, _i, _f, _i] + [_vp] * 7 + [_f] + [_vp] * 6
_lib.gsr_view_loss_backward.restype = _i
_lib.gsr_view_loss_backward.argtypes = [_i, _i, _i, _i, _f, _i] + [_vp] * 7 + [_f] + [_vp] * 9


def _optional_pointers(ts):
    """A host array of device pointers with NULL for None; None (no array) if every entry is None."""
    if all(t is None for t in ts):
        return None
    return (_vp * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def _ptr(t):
    return None if t is None else t.data_ptr()


class FusedViewLoss(torch.autograd.Function):
    """(V,) losses of a contiguous float32 (V,C,H,W) batch of raw renders.  exposure: (V,3,4) or None;
    invdepth: (V,H,W)-sized or None (None unless the depth term runs); `views`: the per-view lists
    (gts, alpha masks, depth targets, depth masks) with None entries; `train`: keep the partial
    planes for a backward."""

    @staticmethod
    def forward(ctx, img, exposure, invdepth, lambda_dssim, clamp, depth_weight, train, views):
        V, C, H, W = img.shape
        dev = img.device
        x = img.detach()
        E = None if exposure is None else exposure.detach()
        inv = None if invdepth is None else invdepth.detach()
        loss = torch.empty((V,), dtype=torch.float32, device=dev)
        parts = [torch.empty_like(x) for _ in range(3)] if train else [None] * 3
        gts, masks, targets, dmasks = views
        with torch.cuda.device(dev):
            ws = torch.empty((_lib.gsr_view_loss_workspace_size(V, C, H, W),), dtype=torch.uint8, device=dev)
            _gsr._check(_lib.gsr_view_loss_forward(
                V, C, H, W, lambda_dssim, int(clamp), x.data_ptr(), _gt_pointers(gts), _ptr(E),
                _optional_pointers(masks), _ptr(inv), _optional_pointers(targets), _optional_pointers(dmasks),
                depth_weight, loss.data_ptr(), *[_ptr(p) for p in parts], ws.data_ptr(),
                torch.cuda.current_stream(dev).cuda_stream))
        if train:
            ctx.save_for_backward(x, E, inv, *parts)
            ctx.views = views  # constants: they carry no graph
        ctx.cfg = (lambda_dssim, clamp, depth_weight, train)
        return loss

    @staticmethod
    def backward(ctx, dloss):
        lambda_dssim, clamp, depth_weight, train = ctx.cfg
        if not train:
            raise RuntimeError("fused_view_loss kept no state for a backward pass")
        x, E, inv, dA, dB, dC = ctx.saved_tensors
        gts, masks, targets, dmasks = ctx.views
        V, C, H, W = x.shape
        dev = x.device
        g = dloss.detach().to(torch.float32).contiguous()  # stays on the device: the kernel reads it
        grad = torch.empty_like(x)
        dE = None if E is None else torch.empty_like(E)
        dinv = None if inv is None else torch.empty_like(inv)
        with torch.cuda.device(dev):
            ws = torch.empty((_lib.gsr_view_loss_workspace_size(V, C, H, W),), dtype=torch.uint8, device=dev)
            _gsr._check(_lib.gsr_view_loss_backward(
                V, C, H, W, lambda_dssim, int(clamp), x.data_ptr(), _gt_pointers(gts), _ptr(E),
                _optional_pointers(masks), _ptr(inv), _optional_pointers(targets), _optional_pointers(dmasks),
                depth_weight, g.data_ptr(), dA.data_ptr(), dB.data_ptr(), dC.data_ptr(), grad.data_ptr(), _ptr(dE),
                _ptr(dinv), ws.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        return grad, dE, dinv, None, None, None, None, None


def _per_view(name, t, V, H, W, single, dev):
    """`t` -- None, one tensor for all views, or a sequence with None entries -- as a list of V
    contiguous float32 (H W)-sized tensors or None."""
    if t is None:
        return [None] * V
    if torch.is_tensor(t):
        if single:
            ts = [t]
        elif t.dim() >= 3 and t.shape[0] == V:
            ts = list(t.unbind(0))
        else:
            raise RuntimeError(f"{name} must have one (H, W) plane per view")
    else:
        ts = list(t)
    if len(ts) != V:
        raise RuntimeError(f"{V} views but {len(ts)} entries in {name}")
    out = []
    for e in ts:
        if e is not None:
            if not torch.is_tensor(e) or e.dim() < 2 or tuple(e.shape[-2:]) != (H, W) or e.numel() != H * W:
                raise RuntimeError(f"every {name} entry must be None or one (H, W) plane of the image size")
            if e.device != dev or e.dtype != torch.float32:
                raise RuntimeError(f"{name} must be float32 on {dev}")
            e = e.detach().contiguous()
        out.append(e)
    return out


def fused_view_loss(img, gt, lambda_dssim=0.2, clamp=True, exposure=None, alpha_mask=None, invdepth=None,
                    invdepth_target=None, depth_mask=None, depth_weight=0.0):
    """train.py:112-141 for a batch of views, from the raw rasterizer outputs, in one forward and one
    backward launch sequence (view_loss_fwd_kernel / view_loss_bwd_kernel):

        e_c    = sum_k img_k E_v[k, c] + E_v[c, 3]          (exposure (V,3,4), 3 channels; None: e = img)
        x_c    = clamp(e_c, 0, 1) * m_v                      (`clamp`; alpha_mask (1,H,W) per view; None: 1)
        loss_v = (1 - lambda_dssim) mean|x - gt_v| + lambda_dssim (1 - mean SSIM(x, gt_v))
                 + depth_weight mean|(invdepth_v - t_v) * dm_v|    (views with a target t_v only)

    img: float32 (V,C,H,W) with 1 <= V <= 16, or (C,H,W) (then exposure is (3,4) and the per-view
    inputs single tensors).  gt, alpha_mask, invdepth_target, depth_mask: one tensor for all views or
    a sequence of V tensors, with None for a view that has none (gt: every view).  invdepth:
    (V,1,H,W).  Returns the (V,) losses (0-dim for a 3-D img), differentiable in img, exposure and
    invdepth (sign(0) = 0; the clamp passes the gradient for 0 <= e <= 1).  If no view has a depth
    target, or depth_weight == 0, invdepth receives no gradient at all (None, not zeros), so the
    rasterizer's backward skips its inverse-depth term.  With every optional input absent this is
    fused_l1_ssim_loss, bit for bit.  GPU only; there is no CPU path."""
    if img.device.type != "cuda":
        raise RuntimeError(f"fused_view_loss runs on the GPU only (HIP); got a tensor on {img.device}")
    if img.dim() not in (3, 4):
        raise RuntimeError("img must be (V, C, H, W) or (C, H, W)")
    if img.dtype != torch.float32:
        raise RuntimeError(f"img must be float32, got {img.dtype}")
    depth_weight = float(depth_weight)
    if not 0.0 <= depth_weight < float("inf"):
        raise RuntimeError(f"depth_weight must be finite and >= 0, got {depth_weight}")
    single = img.dim() == 3
    x = img[None] if single else img
    V, C, H, W = x.shape
    dev = x.device
    if not 1 <= V <= MAX_VIEWS:
        raise RuntimeError(f"fused_view_loss takes 1 to {MAX_VIEWS} views, got {V}")
    if torch.is_tensor(gt) and gt.shape != img.shape:
        raise RuntimeError("img and gt must have the same shape")
    masks = _per_view("alpha_mask", alpha_mask, V, H, W, single, dev)
    targets = _per_view("invdepth_target", invdepth_target, V, H, W, single, dev)
    dmasks = _per_view("depth_mask", depth_mask, V, H, W, single, dev)
    if invdepth is None:
        if any(t is not None for t in targets):
            raise RuntimeError("invdepth_target needs invdepth, the rendered inverse depth")
    else:
        if not torch.is_tensor(invdepth) or invdepth.dim() < 2 or tuple(invdepth.shape[-2:]) != (H, W) \
                or invdepth.numel() != V * H * W:
            raise RuntimeError("invdepth must be (V, 1, H, W), one plane of the image size per view")
        if invdepth.device != dev or invdepth.dtype != torch.float32:
            raise RuntimeError(f"invdepth must be float32 on {dev}")
    if exposure is not None:
        if not torch.is_tensor(exposure) or tuple(exposure.shape) != ((3, 4) if single else (V, 3, 4)):
            raise RuntimeError("exposure must be (V, 3, 4), or (3, 4) for a 3-D img")
        if C != 3:
            raise RuntimeError(f"exposure needs a 3-channel img, got {C} channels")
        if exposure.device != dev or exposure.dtype != torch.float32:
            raise RuntimeError(f"exposure must be float32 on {dev}")
    depth = invdepth is not None and depth_weight > 0 and any(t is not None for t in targets)
    if exposure is None and not depth and all(m is None for m in masks):
        return fused_l1_ssim_loss(img, gt, lambda_dssim, clamp)
    gts = _ground_truths(gt, x, single)
    if H * W >= 2 ** 30:
        raise RuntimeError("fused_view_loss takes images of fewer than 2^30 pixels")
    E = None if exposure is None else (exposure[None] if single else exposure).contiguous()
    inv = invdepth.reshape(V, 1, H, W).contiguous() if depth else None
    if not depth:
        targets, dmasks = [None] * V, [None] * V
    train = torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (x, E, inv))
    loss = FusedViewLoss.apply(x.contiguous(), E, inv, float(lambda_dssim), bool(clamp), depth_weight, train,
                               (gts, masks, targets, dmasks))
    return loss[0] if single else loss
