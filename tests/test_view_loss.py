"""fused_ssim.fused_view_loss (view_loss_fwd_kernel / view_loss_bwd_kernel) against float64 torch
autograd of train.py:112-141 restated per view:

    e_c   = sum_k raw_k E[k, c] + E[c, 3]                  (no exposure: e = raw)
    x_c   = clamp(e_c, 0, 1) * m                            (clamp optional; no mask: m = 1)
    photo = (1 - l) mean|x - gt| + l (1 - mean SSIM(x, gt))  (SSIM: oracle/ssim_oracle.py)
    depth = w mean|(inv - t) * dm|                           (views with a target t only)
    loss  = photo + depth

Tolerances are those of tests/test_photo_loss.py: every loss within 2e-6; every view's dL/draw,
dL/dinv and dL/dE within 1e-4 of that array's largest reference element.  The shapes are that
file's, for the same reasons (below one tile, one past a tile edge, an exact tile height, more tiles
than persistent workgroups).  A view tile spans a view's three channels, so at the largest of them no
workgroup gets a second view tile; MANY_TILES (below) is there for that.

The float32 kernel and the float64 reference must take the same branch of the clamp and of
sign(x - gt), so threshold pixels are removed by construction: raw is nudged until neither raw nor
the exposed value has a channel within 1e-5 of 0 or 1, and gt is nudged wherever |x - gt| < 1e-5
without x == gt, for every combination of exposure / mask / clamp the tests use; each test asserts
that both sets are empty for its combination before it calls the kernel.  gt is zero on half of the
masked-out pixels: there x == gt == 0 exactly.

The CPU tests pin the C ABI's argument checks, which run before any HIP call.
"""
import ctypes
import functools
import itertools
import os
import re

import numpy as np
import pytest
import torch

import ssim_oracle as so

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "gaussian-splatting-npu_amd", "diff_gaussian_rasterization", "libgsr_hip.so")
SYMBOLS = ("gsr_view_loss_workspace_size", "gsr_view_loss_forward", "gsr_view_loss_backward")
GSR_OK, GSR_ERR_INVALID = 0, 1

SHAPES = [(3, 37, 29), (2, 3, 33, 65), (3, 3, 64, 80), (2, 3, 300, 600)]
SMALL = SHAPES[:3]
IDS = [str(s) for s in SHAPES]
LAMBDAS = [0.0, 0.2, 1.0]
# More view tiles (and as many depth tiles) than persistent workgroups, so that a workgroup prefetches
# its next tile's halo across the tile loop: all extras at one lambda only.
MANY_TILES = (2, 3, 481, 1025)
ALL_EXTRAS = [(s, l) for l in LAMBDAS for s in SHAPES] + [(MANY_TILES, 0.2)]
DEPTH_WEIGHT = 0.7
EPS, NUDGE = 1e-5, 1e-3


def _exposed(raw, E):
    return torch.einsum("vkhw,vkc->vchw", raw, E[:, :, :3]) + E[:, :, 3][:, :, None, None]


def _x(raw, E, mask, use_e, use_m, clamp):
    e = _exposed(raw, E) if use_e else raw
    x = e.clamp(0, 1) if clamp else e
    return e, (x * mask if use_m else x)


def _near_threshold(e):
    return ((e.abs() < EPS) | ((e - 1).abs() < EPS)).any(dim=1, keepdim=True)


def _near_gt(x, gt):
    d = (x - gt).abs()
    return (d < EPS) & (d != 0)


@functools.lru_cache(maxsize=None)
def _inputs(shape):
    """float32 inputs of one shape (read-only): raw, E, gt, mask, inv, targets / depth masks (lists
    with None), upstream (V,)."""
    g = torch.Generator().manual_seed(4100 + len(shape) * 1000 + shape[-1])
    V, C, H, W = shape if len(shape) == 4 else (1,) + shape
    raw = 1.4 * torch.rand((V, C, H, W), generator=g) - 0.2
    E = torch.eye(3, 4)[None].repeat(V, 1, 1) + 0.05 * torch.randn((V, 3, 4), generator=g)
    gt = torch.rand((V, C, H, W), generator=g)
    keep = torch.rand((V, 1, H, W), generator=g) >= 0.3
    mask = torch.where(keep, 0.25 + 0.75 * torch.rand((V, 1, H, W), generator=g), torch.zeros(()))
    rows = (torch.arange(H) % 2 == 0)[None, None, :, None]
    gt = torch.where(~keep & rows, torch.zeros(()), gt)
    rounds = 0
    exposable = (False, True) if C == 3 else (False,)
    while True:  # the clamp's thresholds, with and without exposure
        near = _near_threshold(raw.double())
        if C == 3:
            near |= _near_threshold(_exposed(raw.double(), E.double()))
        if not near.any():
            break
        raw = raw + NUDGE * near.float()
        rounds += 1
    assert rounds <= 2
    nudged = 0
    while True:  # sign(x - gt), for every combination the tests use
        near = torch.zeros_like(gt, dtype=torch.bool)
        for use_e, use_m, clamp in itertools.product(exposable, (False, True), (False, True)):
            near |= _near_gt(_x(raw.double(), E.double(), mask.double(), use_e, use_m, clamp)[1], gt.double())
        if not near.any():
            break
        gt = gt + NUDGE * near.float()
        nudged += int(near.sum())
    inv = 0.1 + torch.rand((V, 1, H, W), generator=g)
    targets, dmasks = [], []
    for v in range(V):
        t = inv[v] + 0.3 * torch.randn((1, H, W), generator=g)
        t = torch.where((inv[v] - t).abs() < 1e-4, t + NUDGE, t)
        dm = (torch.rand((1, H, W), generator=g) > 0.2).float() * (0.5 + torch.rand((1, H, W), generator=g))
        targets.append(t if v % 2 == 0 else None)       # views 0, 2 carry a target ...
        dmasks.append(dm if v % 4 == 0 else None)       # ... and view 0 a depth mask
    up = torch.linspace(0.5, 2.0, V) if V > 1 else torch.tensor([1.7])
    e = _exposed(raw.double(), E.double()) if C == 3 else raw.double()
    print(f"{shape}: {rounds} raw nudge rounds, {nudged} gt nudges, "
          f"{float(((e < 0) | (e > 1)).double().mean()):.3f} clamped, {float((mask == 0).double().mean()):.3f} masked out")
    return raw, E, gt, mask, inv, targets, dmasks, up


@functools.lru_cache(maxsize=None)
def _photo_pieces(shape, use_e, use_m, clamp):
    """float64: per-view mean L1 and mean SSIM, and the gradients of sum_v up_v * each with respect
    to raw and E."""
    raw, E, gt, mask, _, _, _, up = _inputs(shape)
    a, Ed = raw.double().requires_grad_(True), E.double().requires_grad_(True)
    _, x = _x(a, Ed, mask.double(), use_e, use_m, clamp)
    l1 = (x - gt.double()).abs().mean(dim=(1, 2, 3))
    ssim = so.ssim_map(x, gt).mean(dim=(1, 2, 3))
    wrt = (a, Ed) if use_e else (a,)
    g_l1 = torch.autograd.grad((l1 * up.double()).sum(), wrt, retain_graph=True)
    g_ssim = torch.autograd.grad((ssim * up.double()).sum(), wrt)
    return l1.detach(), ssim.detach(), g_l1, g_ssim


@functools.lru_cache(maxsize=None)
def _depth_pieces(shape):
    """float64: per-view mean|(inv - t) dm| (0 without a target) and d sum_v up_v * it / d inv."""
    _, _, _, _, inv, targets, dmasks, up = _inputs(shape)
    a = inv.double().requires_grad_(True)
    terms = []
    for v, t in enumerate(targets):
        if t is None:
            terms.append(a[v].sum() * 0)
            continue
        d = a[v] - t.double()
        terms.append((d if dmasks[v] is None else d * dmasks[v].double()).abs().mean())
    depth = torch.stack(terms)
    g, = torch.autograd.grad((depth * up.double()).sum(), a)
    return depth.detach(), g


def _reference(shape, use_e, use_m, use_d, clamp, lam):
    l1, ssim, g_l1, g_ssim = _photo_pieces(shape, use_e, use_m, clamp)
    loss = (1.0 - lam) * l1 + lam * (1.0 - ssim)
    ref = {"raw": ((1.0 - lam) * g_l1[0] - lam * g_ssim[0]).numpy()}
    if use_e:
        ref["E"] = ((1.0 - lam) * g_l1[1] - lam * g_ssim[1]).numpy()
    if use_d:
        depth, g = _depth_pieces(shape)
        loss = loss + DEPTH_WEIGHT * depth
        ref["inv"] = (DEPTH_WEIGHT * g).numpy()
    return loss.numpy(), ref


def _run(shape, use_e, use_m, use_d, clamp, lam, lists=True):
    """fused_view_loss on the GPU: (loss (V,), {"raw", "E", "inv"} gradients as numpy, the loss tensor)."""
    from fused_ssim import fused_view_loss
    raw, E, gt, mask, inv, targets, dmasks, up = _inputs(shape)
    # no threshold pixels for this combination
    e, x = _x(raw.double(), E.double(), mask.double(), use_e, use_m, clamp)
    assert not _near_threshold(e).any() and not _near_gt(x, gt.double()).any()
    single = len(shape) == 3
    dev = torch.device("cuda", 0)
    a = (raw[0] if single else raw).to(dev).requires_grad_(True)
    kw = {}
    leaves = {"raw": a}
    if use_e:
        leaves["E"] = kw["exposure"] = (E[0] if single else E).to(dev).requires_grad_(True)
    if use_m:
        kw["alpha_mask"] = mask[0].to(dev) if single else ([m.to(dev) for m in mask] if lists else mask.to(dev))
    if use_d:
        leaves["inv"] = kw["invdepth"] = (inv[0] if single else inv).to(dev).requires_grad_(True)
        tg = [None if t is None else t.to(dev) for t in targets]
        dm = [None if m is None else m.to(dev) for m in dmasks]
        kw["invdepth_target"], kw["depth_mask"] = (tg[0], dm[0]) if single else (tg, dm)
        kw["depth_weight"] = DEPTH_WEIGHT
    g = (gt[0] if single else gt).to(dev)
    loss = fused_view_loss(a, g if single or not lists else [t.clone() for t in g], lam, clamp=clamp, **kw)
    assert loss.shape == (() if single else (shape[0],))
    (loss.reshape(-1) * up.to(dev)).sum().backward()
    grads = {k: (None if t.grad is None else t.grad.cpu().numpy().reshape((len(up),) + tuple(t.shape[-3 if k != "E" else -2:])))
             for k, t in leaves.items()}
    return loss.detach().cpu().numpy().reshape(-1), grads, loss


def _check(shape, use_e, use_m, use_d, clamp, lam, lists=True):
    loss, grads, _ = _run(shape, use_e, use_m, use_d, clamp, lam, lists)
    ref_loss, ref = _reference(shape, use_e, use_m, use_d, clamp, lam)
    print(f"{shape} E={use_e} mask={use_m} depth={use_d} clamp={clamp} lambda={lam}: "
          f"max |loss - ref| = {np.abs(loss - ref_loss).max():.3e}")
    worst = {}
    for k, r in ref.items():
        for v in range(len(ref_loss)):
            err, big = np.abs(grads[k][v] - r[v]).max(), np.abs(r[v]).max()
            print(f"  d{k} view {v}: max |grad - ref| = {err:.3e} of {big:.3e}")
            worst[(k, v)] = (err, big)
    assert np.abs(loss - ref_loss).max() < 2e-6
    for (k, v), (err, big) in worst.items():
        assert err <= 1e-4 * big + 1e-12, (k, v, err, big)
    return grads


def _check_exact_zeros(shape, use_e, use_m, clamp, grads):
    """Nothing flows where the mask is 0 or the clamp is active."""
    raw, E, _, mask, _, _, _, _ = _inputs(shape)
    e = (_exposed(raw.double(), E.double()) if use_e else raw.double()).numpy()
    blocked = np.zeros(e.shape, dtype=bool)
    if clamp:
        blocked |= (e < 0) | (e > 1)
    if use_m:
        blocked |= np.broadcast_to(mask.numpy() == 0, e.shape)
    if use_e:  # a raw channel feeds every exposed channel: zero only where all three are blocked
        blocked = np.broadcast_to(blocked.all(axis=1, keepdims=True), e.shape)
    if clamp or use_m:
        assert blocked.any() and (~blocked).any()
    assert np.all(grads["raw"][blocked] == 0.0)
    assert np.count_nonzero(grads["raw"][~blocked]) > 0.9 * (~blocked).sum()


ALONE = [(True, False, False), (False, True, False), (False, False, True)]


@pytest.mark.gpu
@pytest.mark.parametrize("extras", ALONE, ids=["exposure", "mask", "depth"])
@pytest.mark.parametrize("shape", SMALL, ids=IDS[:3])
def test_each_extra_alone(shape, extras):
    use_e, use_m, use_d = extras
    grads = _check(shape, use_e, use_m, use_d, True, 0.2)
    _check_exact_zeros(shape, use_e, use_m, True, grads)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,lam", ALL_EXTRAS, ids=[f"{s}-{l}" for s, l in ALL_EXTRAS])
def test_all_extras(shape, lam):
    if shape == MANY_TILES:
        # 16 x 17 tile positions, two views: 544 depth tiles, then 544 view tiles, for a persistent grid
        # of 2 workgroups per CU, so some workgroups walk a second view tile (prefetched across the tile
        # loop) and some reach the view tiles on a later round of the depth-tile loop
        assert 2 * 16 * 17 > 2 * torch.cuda.get_device_properties(0).multi_processor_count
    grads = _check(shape, True, True, True, True, lam)
    _check_exact_zeros(shape, True, True, True, grads)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_without_clamp(shape):
    grads = _check(shape, True, True, True, False, 0.2)
    _check_exact_zeros(shape, True, True, False, grads)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(2, 4, 33, 65), (1, 33, 65)], ids=["(2, 4, 33, 65)", "(1, 33, 65)"])
def test_other_channel_counts(shape):
    """Without an exposure any C: the kernels walk channel groups of up to three, so C = 4 is a full
    group and a group of one, C = 1 a group of one."""
    grads = _check(shape, False, True, True, True, 0.2)
    _check_exact_zeros(shape, False, True, True, grads)


@pytest.mark.gpu
def test_mask_tensor_and_gt_tensor():
    """alpha_mask as one (V,1,H,W) tensor and gt as one (V,3,H,W) tensor."""
    _check((2, 3, 33, 65), False, True, False, True, 0.2, lists=False)


@pytest.mark.gpu
def test_sign_of_zero_is_zero():
    """lambda = 0 leaves the L1 term alone: where x == gt exactly (gt = 0 under a zero mask) the
    gradient is exactly zero, and elsewhere it is the closed form."""
    shape = (2, 3, 33, 65)
    _, grads, _ = _run(shape, False, True, False, True, 0.0)
    raw, _, gt, mask, _, _, _, up = _inputs(shape)
    x = raw.clamp(0, 1) * mask
    same = (x == gt).numpy()
    assert same.any() and np.all(grads["raw"][same] == 0.0)
    inside = ((raw >= 0) & (raw <= 1)).float()
    expect = (up[:, None, None, None] * torch.sign(x - gt) * mask * inside / raw[0].numel()).numpy()
    assert np.allclose(grads["raw"], expect, rtol=1e-6, atol=0)


@pytest.mark.gpu
def test_view_without_target_gets_zero_depth_gradient():
    shape = (3, 3, 64, 80)
    _, grads, _ = _run(shape, True, True, True, True, 0.2)
    targets = _inputs(shape)[5]
    assert [t is None for t in targets] == [False, True, False]
    assert np.all(grads["inv"][1] == 0.0)
    assert np.count_nonzero(grads["inv"][0]) > 0 and np.count_nonzero(grads["inv"][2]) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 29), (2, 3, 300, 600)], ids=[IDS[0], IDS[3]])
def test_no_extras_is_fused_l1_ssim_loss(shape):
    from fused_ssim import fused_l1_ssim_loss, fused_view_loss
    raw, _, gt, _, _, _, _, up = _inputs(shape)
    out = []
    for fn in (fused_view_loss, fused_l1_ssim_loss):
        a = (raw[0] if len(shape) == 3 else raw).cuda().requires_grad_(True)
        loss = fn(a, (gt[0] if len(shape) == 3 else gt).cuda(), 0.2, clamp=True)
        (loss.reshape(-1) * up.cuda()).sum().backward()
        out.append((loss.detach(), a.grad))
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_identity_exposure_and_ones_mask():
    """[I|0] and a mask of ones change nothing: within the loss kernels' tolerances of fused_l1_ssim_loss."""
    from fused_ssim import fused_l1_ssim_loss, fused_view_loss
    shape = (2, 3, 33, 65)
    raw, _, gt, _, _, _, _, up = _inputs(shape)
    a = raw.cuda().requires_grad_(True)
    b = raw.cuda().requires_grad_(True)
    E = torch.eye(3, 4)[None].repeat(2, 1, 1).cuda().requires_grad_(True)
    one = fused_view_loss(a, gt.cuda(), 0.2, clamp=True, exposure=E, alpha_mask=torch.ones(2, 1, 33, 65).cuda())
    two = fused_l1_ssim_loss(b, gt.cuda(), 0.2, clamp=True)
    (one * up.cuda()).sum().backward()
    (two * up.cuda()).sum().backward()
    assert (one - two).abs().max().item() < 2e-6
    for v in range(2):
        assert (a.grad[v] - b.grad[v]).abs().max().item() <= 1e-4 * b.grad[v].abs().max().item()
    assert E.grad is not None and E.grad.abs().max().item() > 0


@pytest.mark.gpu
def test_bitwise_reproducible():
    a = _run((2, 3, 300, 600), True, True, True, True, 0.2)
    b = _run((2, 3, 300, 600), True, True, True, True, 0.2)
    assert np.array_equal(a[0], b[0])
    for k in ("raw", "E", "inv"):
        assert np.array_equal(a[1][k], b[1][k]), k


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(3, 37, 29), (2, 3, 300, 600)], ids=[IDS[0], IDS[3]])
def test_no_grad_loss_is_the_training_loss(shape):
    from fused_ssim import fused_view_loss
    raw, E, gt, mask, inv, targets, dmasks, _ = _inputs(shape)
    single = len(shape) == 3
    pick = (lambda t: t[0].cuda()) if single else (lambda t: t.cuda())
    tg = [None if t is None else t.cuda() for t in targets]
    dm = [None if t is None else t.cuda() for t in dmasks]
    kw = dict(exposure=pick(E), alpha_mask=pick(mask), invdepth=pick(inv), depth_weight=DEPTH_WEIGHT,
              invdepth_target=tg[0] if single else tg, depth_mask=dm[0] if single else dm)
    x, g = pick(raw), pick(gt)
    train = fused_view_loss(x.clone().requires_grad_(True), g, 0.2, **kw)
    assert train.requires_grad
    with torch.no_grad():
        quiet = fused_view_loss(x.clone().requires_grad_(True), g, 0.2, **kw)
    plain = fused_view_loss(x, g, 0.2, **kw)
    assert not quiet.requires_grad and not plain.requires_grad
    assert torch.equal(train.detach(), quiet) and torch.equal(train.detach(), plain)


@pytest.mark.gpu
def test_invdepth_grad_is_none_when_nothing_asks_for_it():
    from fused_ssim import fused_view_loss
    shape = (2, 3, 33, 65)
    raw, _, gt, mask, inv, targets, _, _ = _inputs(shape)
    tg = [None if t is None else t.cuda() for t in targets]
    for kw in (dict(invdepth_target=tg, depth_weight=0.0), dict(invdepth_target=[None, None], depth_weight=0.5),
               dict(depth_weight=0.5)):
        a = raw.cuda().requires_grad_(True)
        d = inv.cuda().requires_grad_(True)
        fused_view_loss(a, gt.cuda(), 0.2, alpha_mask=mask.cuda(), invdepth=d, **kw).sum().backward()
        assert d.grad is None and a.grad is not None
    d = inv.cuda().requires_grad_(True)
    fused_view_loss(raw.cuda().requires_grad_(True), gt.cuda(), 0.2, invdepth=d, invdepth_target=tg,
                    depth_weight=0.5).sum().backward()
    assert d.grad is not None


@pytest.mark.gpu
def test_rejects_bad_input():
    from fused_ssim import fused_view_loss
    with pytest.raises(RuntimeError, match="GPU only"):
        fused_view_loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))
    z = torch.zeros(17, 3, 8, 8, device="cuda")
    with pytest.raises(RuntimeError, match="1 to 16 views"):
        fused_view_loss(z, z)
    z = z[:2]
    with pytest.raises(RuntimeError, match="float32"):
        fused_view_loss(z.double(), z.double())
    with pytest.raises(RuntimeError, match="same shape"):
        fused_view_loss(z, torch.zeros(2, 3, 8, 9, device="cuda"))
    with pytest.raises(RuntimeError, match="ground-truth"):
        fused_view_loss(z, [z[0]])
    with pytest.raises(RuntimeError, match="exposure"):
        fused_view_loss(z, z, exposure=torch.zeros(2, 3, 3, device="cuda"))
    with pytest.raises(RuntimeError, match="exposure"):
        fused_view_loss(z[:, :1], z[:, :1], exposure=torch.zeros(2, 3, 4, device="cuda"))
    with pytest.raises(RuntimeError, match="alpha_mask"):
        fused_view_loss(z, z, alpha_mask=[torch.zeros(1, 8, 9, device="cuda"), None])
    with pytest.raises(RuntimeError, match="invdepth"):
        fused_view_loss(z, z, invdepth_target=[torch.zeros(1, 8, 8, device="cuda"), None], depth_weight=1.0)
    with pytest.raises(RuntimeError, match="invdepth"):
        fused_view_loss(z, z, invdepth=torch.zeros(2, 1, 8, 9, device="cuda"))
    with pytest.raises(RuntimeError, match="depth_weight"):
        fused_view_loss(z, z, invdepth=torch.zeros(2, 1, 8, 8, device="cuda"), depth_weight=-1.0)
    with pytest.raises(RuntimeError, match="depth_weight"):
        fused_view_loss(z, z, invdepth=torch.zeros(2, 1, 8, 8, device="cuda"), depth_weight=float("nan"))


# ---- the C ABI's argument checks: no device needed ------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        pytest.fail(f"{LIB} missing: run __graft_entry__.build()")
    lib = ctypes.CDLL(LIB)
    lib.gsr_last_error.restype = ctypes.c_char_p
    vp, i, f = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
    lib.gsr_view_loss_workspace_size.restype = ctypes.c_size_t
    lib.gsr_view_loss_workspace_size.argtypes = [i, i, i, i]
    # V C H W lambda clamp | img gt exposure alpha_mask invdepth invdepth_target depth_mask | depth_weight | ...
    lib.gsr_view_loss_forward.argtypes = [i, i, i, i, f, i] + [vp] * 7 + [f] + [vp] * 6
    lib.gsr_view_loss_backward.argtypes = [i, i, i, i, f, i] + [vp] * 7 + [f] + [vp] * 9
    return lib


def test_symbols_declared_and_exported(lib):
    text = open(os.path.join(ROOT, "include", "fused_ssim.h")).read()
    for s in SYMBOLS:
        assert re.search(r"\b%s\s*\(" % s, text), s
        assert hasattr(lib, s), s


def test_workspace_size(lib):
    assert lib.gsr_view_loss_workspace_size(0, 3, 8, 8) == 0
    assert lib.gsr_view_loss_workspace_size(17, 3, 8, 8) == 0
    # per view and 64x32 tile position: the 12 exposure-gradient sums of the backward (doubles), which
    # is more than the forward's (SSIM, L1) pair per group of three channels plus one depth sum
    assert lib.gsr_view_loss_workspace_size(1, 3, 1, 1) == 12 * 8
    assert lib.gsr_view_loss_workspace_size(8, 3, 1080, 1920) == 8 * 30 * 34 * 12 * 8
    # 20 channels: 7 groups of up to three, 2 * 7 + 1 = 15 doubles
    assert lib.gsr_view_loss_workspace_size(2, 20, 33, 65) == 2 * 2 * 2 * 15 * 8


def test_zero_size_is_ok_and_bad_arguments_are_refused(lib):
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    arr = (ctypes.c_void_p * 16)(*[p.value] * 16)
    none = (ctypes.c_void_p * 16)()

    def fwd(V, C, H, W, lam=0.2, img=p, gt=arr, exposure=None, alpha=None, inv=None, target=None, dmask=None,
            weight=0.0, loss=p, ws=p):
        return lib.gsr_view_loss_forward(V, C, H, W, lam, 1, img, gt, exposure, alpha, inv, target, dmask, weight,
                                         loss, None, None, None, ws, None)

    def bwd(V, C, H, W, lam=0.2, img=p, gt=arr, exposure=None, alpha=None, inv=None, target=None, dmask=None,
            weight=0.0, dloss=p, planes=(p, p, p), draw=p, dE=None, dinv=None, ws=p):
        return lib.gsr_view_loss_backward(V, C, H, W, lam, 1, img, gt, exposure, alpha, inv, target, dmask, weight,
                                          dloss, *planes, draw, dE, dinv, ws, None)

    for V, C, H, W in ((0, 3, 8, 8), (1, 0, 8, 8), (1, 3, 0, 8), (1, 3, 8, 0)):
        assert fwd(V, C, H, W, img=None, gt=None, loss=None, ws=None) == GSR_OK
        assert bwd(V, C, H, W, img=None, gt=None, dloss=None, planes=(None,) * 3, draw=None, ws=None) == GSR_OK
    for V, C, H, W in ((-1, 3, 8, 8), (1, -3, 8, 8), (1, 3, -8, 8), (1, 3, 8, -8), (17, 3, 8, 8)):
        assert fwd(V, C, H, W) == GSR_ERR_INVALID
        assert lib.gsr_last_error()
        assert bwd(V, C, H, W) == GSR_ERR_INVALID
    # lambda outside [0, 1]
    assert fwd(1, 3, 4, 4, lam=1.5) == GSR_ERR_INVALID and bwd(1, 3, 4, 4, lam=-0.1) == GSR_ERR_INVALID
    # null required pointers
    for kw in ({"img": None}, {"gt": None}, {"loss": None}, {"ws": None}):
        assert fwd(1, 3, 4, 4, **kw) == GSR_ERR_INVALID, kw
        assert b"null" in lib.gsr_last_error()
    for kw in ({"img": None}, {"gt": None}, {"dloss": None}, {"draw": None}, {"planes": (p, None, p)},
               {"exposure": p}, {"exposure": p, "dE": p, "ws": None}):  # exposure without dL_dexposure / workspace
        assert bwd(1, 3, 4, 4, **kw) == GSR_ERR_INVALID, kw
        assert b"null" in lib.gsr_last_error()
    # holes in gt
    holes = (ctypes.c_void_p * 16)(p.value, None)
    assert fwd(2, 3, 4, 4, gt=holes) == GSR_ERR_INVALID and bwd(2, 3, 4, 4, gt=holes) == GSR_ERR_INVALID
    # exposure with C != 3
    assert fwd(1, 1, 4, 4, exposure=p) == GSR_ERR_INVALID
    assert b"exposure" in lib.gsr_last_error()
    assert bwd(1, 4, 4, 4, exposure=p, dE=p) == GSR_ERR_INVALID
    # depth targets without invdepth
    assert fwd(1, 3, 4, 4, target=arr, weight=1.0) == GSR_ERR_INVALID
    assert b"invdepth" in lib.gsr_last_error()
    assert bwd(1, 3, 4, 4, target=arr, weight=1.0) == GSR_ERR_INVALID
    # a depth mask without targets
    assert fwd(1, 3, 4, 4, inv=p, dmask=arr, weight=1.0) == GSR_ERR_INVALID
    # negative or non-finite depth_weight
    for w in (-1.0, float("nan"), float("inf")):
        assert fwd(1, 3, 4, 4, inv=p, target=none, weight=w) == GSR_ERR_INVALID, w
        assert b"depth_weight" in lib.gsr_last_error()
        assert bwd(1, 3, 4, 4, inv=p, target=none, weight=w) == GSR_ERR_INVALID, w
