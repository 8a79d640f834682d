"""fused_ssim.fused_l1_ssim_loss (photo_loss_fwd_kernel / photo_loss_bwd_kernel) against the float64
restatement: loss_v = (1 - l) mean|x - gt| + l (1 - mean SSIM(x, gt)) with SSIM from
oracle/ssim_oracle.py and both terms differentiated by autograd in float64.

Tolerances are those of tests/test_ssim.py for these float32 kernels: every loss within 2e-6,
every view's gradient within 1e-4 of its largest reference element.  The shapes are the smallest
at which the kernels take another path: below one 64x32 tile, one past a tile edge on both axes,
an exact tile height, and 600 tiles (more than the 512 persistent workgroups, so the grid-stride
loop with its prefetch runs).  Views differ and carry different upstream gradients, so a tile
credited to the wrong view shows.  The CPU tests pin the C ABI's argument checks, which run
before any HIP call.
"""
import ctypes
import functools
import os
import re

import numpy as np
import pytest
import torch

import ssim_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussian-splatting-npu_amd", "diff_gaussian_rasterization", "libgsr_hip.so")
SYMBOLS = ("gsr_photo_loss_workspace_size", "gsr_photo_loss_forward", "gsr_photo_loss_backward")
GSR_OK, GSR_ERR_INVALID = 0, 1

SHAPES = [(3, 37, 29), (2, 3, 33, 65), (3, 3, 64, 80), (2, 3, 300, 600)]
IDS = [str(s) for s in SHAPES]
LAMBDAS = [0.0, 0.2, 1.0]


@functools.lru_cache(maxsize=None)
def _case(shape, clamp):
    """(img, gt, upstream (V,), reference pieces in float64) -- computed once per shape, read-only.
    Pieces per view: mean L1, mean SSIM and their gradients with respect to img."""
    g = torch.Generator().manual_seed(100 + len(shape) * 1000 + shape[-1] + (7 if clamp else 0))
    shape4 = shape if len(shape) == 4 else (1,) + shape
    V = shape4[0]
    if clamp:
        img = 1.4 * torch.rand(shape4, generator=g) - 0.2
        gt = torch.rand(shape4, generator=g)
    else:
        img = torch.rand(shape4, generator=g)
        gt = (img + 0.1 * torch.randn(shape4, generator=g)).clamp(0, 1)
    img[..., ::7, ::5] = gt[..., ::7, ::5]  # x == gt exactly: sign(0) = 0
    up = torch.linspace(0.5, 2.0, V) if V > 1 else torch.tensor([1.7])
    a = img.double().requires_grad_(True)
    x = a.clamp(0, 1) if clamp else a
    l1 = (x - gt.double()).abs().mean(dim=(1, 2, 3))
    ssim = so.ssim_map(x, gt).mean(dim=(1, 2, 3))
    g_l1, = torch.autograd.grad(l1.sum(), a, retain_graph=True)
    g_ssim, = torch.autograd.grad(ssim.sum(), a)
    return img, gt, up, (l1.detach(), ssim.detach(), g_l1, g_ssim)


def _reference(shape, clamp, lam):
    img, gt, up, (l1, ssim, g_l1, g_ssim) = _case(shape, clamp)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    grad = up.double()[:, None, None, None] * ((1.0 - lam) * g_l1 - lam * g_ssim)
    return loss.numpy(), grad.numpy()


def _run(shape, clamp, lam, gt_as_list):
    from fused_ssim import fused_l1_ssim_loss
    img, gt, up, _ = _case(shape, clamp)
    if len(shape) == 3:
        img, gt = img[0], gt[0]
    x = img.cuda().requires_grad_(True)
    gtc = gt.cuda()
    target = ([gtc] if len(shape) == 3 else [t.clone() for t in gtc]) if gt_as_list else gtc
    loss = fused_l1_ssim_loss(x, target, lam, clamp=clamp)
    assert loss.shape == (() if len(shape) == 3 else (shape[0],))
    (loss.reshape(-1) * up.cuda()).sum().backward()
    return loss.detach().cpu().numpy().reshape(-1), x.grad.cpu().numpy().reshape(_case(shape, clamp)[0].shape), img


def _check(shape, clamp, lam, gt_as_list):
    loss, grad, _ = _run(shape, clamp, lam, gt_as_list)
    ref_loss, ref_grad = _reference(shape, clamp, lam)
    print(f"{shape} clamp={clamp} lambda={lam}: max |loss - ref| = {np.abs(loss - ref_loss).max():.3e}")
    for v in range(len(ref_loss)):
        err, big = np.abs(grad[v] - ref_grad[v]).max(), np.abs(ref_grad[v]).max()
        print(f"  view {v}: max |grad - ref| = {err:.3e} of {big:.3e}")
    assert np.abs(loss - ref_loss).max() < 2e-6
    for v in range(len(ref_loss)):
        assert np.abs(grad[v] - ref_grad[v]).max() <= 1e-4 * np.abs(ref_grad[v]).max() + 1e-12
    return grad


@pytest.mark.gpu
@pytest.mark.parametrize("lam", LAMBDAS)
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_matches_oracle_gt_list(shape, lam):
    _check(shape, False, lam, gt_as_list=True)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_matches_oracle_gt_tensor(shape):
    _check(shape, False, 0.2, gt_as_list=False)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_clamp(shape):
    """clamp=True on img = 1.4 rand - 0.2: the loss of the clamped image, and no gradient at all
    where the clamp is active."""
    grad = _check(shape, True, 0.2, gt_as_list=True)
    img = _case(shape, True)[0].numpy()
    outside = (img < 0) | (img > 1)
    assert outside.any() and (~outside).any()
    assert np.all(grad[outside] == 0.0)
    assert np.count_nonzero(grad[~outside]) > 0.9 * (~outside).sum()


@pytest.mark.gpu
def test_sign_of_zero_is_zero():
    """lambda = 0 leaves the L1 term alone: where x == gt exactly the gradient is exactly zero."""
    shape = (2, 3, 33, 65)
    _, grad, _ = _run(shape, False, 0.0, True)
    img, gt, up, _ = _case(shape, False)
    same = (img == gt).numpy()
    assert same.any() and np.all(grad[same] == 0.0)
    n = img[0].numel()
    expect = (up[:, None, None, None] * torch.sign(img - gt) / n).numpy()
    assert np.allclose(grad, expect, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_bitwise_reproducible():
    a = _run((2, 3, 300, 600), True, 0.2, True)
    b = _run((2, 3, 300, 600), True, 0.2, True)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 29), (2, 3, 300, 600)], ids=["(3, 37, 29)", "(2, 3, 300, 600)"])
def test_no_grad_loss_is_the_training_loss(shape):
    from fused_ssim import fused_l1_ssim_loss
    img, gt, _, _ = _case(shape, True)
    if len(shape) == 3:
        img, gt = img[0], gt[0]
    x, g = img.cuda(), gt.cuda()
    train = fused_l1_ssim_loss(x.clone().requires_grad_(True), g, 0.2, clamp=True)
    assert train.requires_grad
    with torch.no_grad():
        quiet = fused_l1_ssim_loss(x.clone().requires_grad_(True), g, 0.2, clamp=True)
    plain = fused_l1_ssim_loss(x, g, 0.2, clamp=True)
    assert not quiet.requires_grad and not plain.requires_grad
    assert torch.equal(train.detach(), quiet) and torch.equal(train.detach(), plain)


@pytest.mark.gpu
def test_rejects_bad_input():
    from fused_ssim import fused_l1_ssim_loss
    with pytest.raises(RuntimeError, match="GPU only"):
        fused_l1_ssim_loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    z = torch.zeros(17, 1, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="1 to 16 views"):
        fused_l1_ssim_loss(z, z)
    with pytest.raises(RuntimeError, match="same shape"):
        fused_l1_ssim_loss(z[:2], torch.zeros(2, 1, 8, 9, device="cuda"))
    with pytest.raises(RuntimeError, match="ground-truth"):
        fused_l1_ssim_loss(z[:2], [z[0]])


# ---- the C ABI's argument checks: no device needed ------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.gsr_last_error.restype = ctypes.c_char_p
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.gsr_photo_loss_workspace_size.restype = ctypes.c_size_t
    lib.gsr_photo_loss_workspace_size.argtypes = [i, i, i, i]
    lib.gsr_photo_loss_forward.argtypes = [i, i, i, i, f, i] + [vp] * 8
    lib.gsr_photo_loss_backward.argtypes = [i, i, i, i, f, i] + [vp] * 8
    return lib


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "fused_ssim.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s


def test_workspace_size(lib):
    assert lib.gsr_photo_loss_workspace_size(0, 3, 8, 8) == 0
    assert lib.gsr_photo_loss_workspace_size(1, 3, 1, 1) >= 3 * 16
    # one pair of doubles per 64x32 tile of every plane
    assert lib.gsr_photo_loss_workspace_size(8, 3, 1080, 1920) == 8 * 3 * 30 * 34 * 16


def test_zero_size_is_ok_and_bad_arguments_are_refused(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    gts = (ctypes.c_void_p * 16)(*[p.value] * 16)
    for V, C, H, W in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0)):
        assert lib.gsr_photo_loss_forward(V, C, H, W, 0.2, 0, None, None, None, None, None, None, None, None) == GSR_OK
        assert lib.gsr_photo_loss_backward(V, C, H, W, 0.2, 0, None, None, None, None, None, None, None, None) == GSR_OK
    for V, C, H, W in ((-1, 3, 8, 8), (1, -3, 8, 8), (1, 3, -8, 8), (1, 3, 8, -8), (17, 3, 8, 8)):
        assert lib.gsr_photo_loss_forward(V, C, H, W, 0.2, 0, p, gts, p, None, None, None, p, None) == GSR_ERR_INVALID
        assert lib.gsr_last_error()
        assert lib.gsr_photo_loss_backward(V, C, H, W, 0.2, 0, p, gts, p, p, p, p, p, None) == GSR_ERR_INVALID
    # a null image, ground-truth array, ground-truth entry, loss or workspace
    ok = [p, gts, p, None, None, None, p]
    for k in (0, 1, 2, 6):
        a = list(ok)
        a[k] = None
        assert lib.gsr_photo_loss_forward(1, 1, 4, 4, 0.2, 0, *a, None) == GSR_ERR_INVALID, k
        assert b"null" in lib.gsr_last_error()
    holes = (ctypes.c_void_p * 16)(p.value, None)
    assert lib.gsr_photo_loss_forward(2, 1, 4, 4, 0.2, 0, p, holes, p, None, None, None, p, None) == GSR_ERR_INVALID
    okb = [p, gts, p, p, p, p, p]
    for k in range(7):
        a = list(okb)
        a[k] = None
        assert lib.gsr_photo_loss_backward(1, 1, 4, 4, 0.2, 0, *a, None) == GSR_ERR_INVALID, k
    assert lib.gsr_photo_loss_forward(1, 1, 4, 4, 1.5, 0, p, gts, p, None, None, None, p, None) == GSR_ERR_INVALID
