"""The alpha output, alpha = 1 - final_T, and its gradient (needs an MI355X: -m gpu).

* forward: GaussianRasterizer / MultiViewRasterizer(return_alpha=True) return the accumulated opacity
  of each pixel, bit-equal to 1 - final_T of the call's own image state and within IMG_ATOL of the
  oracle's; the other three outputs are the bits of the call without it.
* backward, zero tolerance: a gradient gA on alpha enters render_bwd's walk as its start value
  bg . dL/dpixel - gA and nowhere else.  With bg = 0 and gA = -(k gC[0]) the walk therefore starts from
  fl(k gC[0]) -- the value it starts from with bg = (k, 0, 0) and no alpha gradient, where
  fma(0, ., fma(0, ., k gC[0])) is that product too -- and nothing else in the backward reads bg:
  every input gradient of the two runs must be the same bits.
* backward against the oracle: the reference has no alpha output, but its render with colour 1 and
  background 0 has channel 0 = 1 - final_T, so two oracle passes over the same geometry (the usual
  one, and that one with dL_dcolor = (gA, 0, 0)) sum to the gradients of the loss with an alpha term.

The "stack" scenes put 12 large, opaque Gaussians on the camera's axis in front of a 300-Gaussian
cloud: their pixels saturate (final_T < 1e-3, the walk stops before the tile's list ends) and the
tiles' lists are longer than one 64-entry batch of render_bwd, at image sizes with partial edge
tiles.  _stack_case asserts both from the oracle alone before a test looks at the GPU.
"""
import functools

import numpy as np
import pytest
import torch

import common
import synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
K_BG = 0.75
MODES = ("sh_scales", "colors_scales", "sh_cov", "colors_cov")


def _dgr():
    import diff_gaussian_rasterization as dgr
    return dgr


def _with_precomp(case):
    g = torch.Generator().manual_seed(7)
    P = case["scene"]["means3D"].shape[0]
    case["colors_precomp"] = torch.rand(P, 3, generator=g)
    o, _ = common.run_oracle(case, "sh_scales", backward=False)
    case["cov3D_precomp"] = torch.from_numpy(o.get("cov3D").copy())
    return case


@functools.lru_cache(maxsize=None)
def _default_case():
    return _with_precomp(common.make_case())


@functools.lru_cache(maxsize=None)
def _stack_case(H, W):
    case = common.make_case(P=300, H=H, W=W)
    sc, cam = case["scene"], case["cam"]
    sc["means3D"][:12] = cam.camera_center * torch.linspace(-0.05, 0.05, 12)[:, None]
    sc["scales"][:12] = 0.3
    sc["rotations"][:12] = torch.tensor([1.0, 0.0, 0.0, 0.0])
    sc["opacities"][:12] = 0.8
    case = _with_precomp(case)
    # the scene must stay a hard one: early-stopped pixels and walks of more than one batch
    o, _ = common.run_oracle(case, backward=False)
    fT, nc = o.get("final_T").reshape(H, W), o.get("n_contrib").reshape(H, W)
    ranges = o.get("ranges").astype(np.int64)
    tiles_x = (W + 15) // 16
    ys, xs = np.mgrid[0:H, 0:W]
    length = (ranges[:, 1] - ranges[:, 0])[(ys // 16) * tiles_x + xs // 16]
    early = int(((fT < 1e-3) & (nc < length)).sum())
    assert early >= 20, f"stack {H}x{W}: only {early} early-stopped pixels"
    assert int(nc.max()) > 64, f"stack {H}x{W}: largest n_contrib {int(nc.max())}"
    assert H % 16 and W % 16
    return case


SCENES = {"default": _default_case, "stack50x70": lambda: _stack_case(50, 70),
          "stack37x50": lambda: _stack_case(37, 50)}


def _settings(case, antialiasing=False, bg=(0.0, 0.0, 0.0), cam=None):
    cam = cam or case["cam"]
    return _dgr().GaussianRasterizationSettings(
        image_height=case["H"], image_width=case["W"], tanfovx=cam.tanfovx, tanfovy=cam.tanfovy,
        bg=torch.tensor(bg, dtype=torch.float32, device=DEV), scale_modifier=1.0,
        viewmatrix=cam.world_view_transform.to(DEV), projmatrix=cam.full_proj_transform.to(DEV),
        sh_degree=case["sh_degree"], campos=cam.camera_center.to(DEV), prefiltered=False, debug=False,
        antialiasing=antialiasing)


def _leaves(case, mode):
    """The rasterizer's keyword inputs for `mode` (MODES, or "dc": SH + scales with dc apart) as leaves."""
    sc = case["scene"]
    t = {"means3D": sc["means3D"], "opacities": sc["opacities"]}
    if mode == "dc":
        t["dc"], t["shs"] = sc["shs"][:, :1].contiguous(), sc["shs"][:, 1:].contiguous()
    elif mode.startswith("sh"):
        t["shs"] = sc["shs"]
    else:
        t["colors_precomp"] = case["colors_precomp"]
    if mode.endswith("cov"):
        t["cov3D_precomp"] = case["cov3D_precomp"]
    else:
        t["scales"], t["rotations"] = sc["scales"], sc["rotations"]
    return {k: v.to(DEV).clone().requires_grad_(True) for k, v in t.items()}


def _c_forward(s, kw):
    """_C.rasterize_gaussians on the settings and GaussianRasterizer-style inputs `kw`."""
    e = torch.Tensor([])
    g = lambda k: kw[k].detach() if k in kw else e  # noqa: E731
    return _dgr()._C.rasterize_gaussians(
        s.bg, g("means3D"), g("colors_precomp"), g("opacities"), g("scales"), g("rotations"), s.scale_modifier,
        g("cov3D_precomp"), s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, s.image_height, s.image_width,
        g("shs"), s.sh_degree, s.campos, s.prefiltered, s.antialiasing, False, dc=kw.get("dc"))


def _img_state(img, W, H):
    """final_T and n_contrib of a forward, read from its image state buffer."""
    lay = _dgr()._C.image_layout(W, H)
    N = W * H
    fT = img[lay[1]:lay[1] + 4 * N].cpu().numpy().view(np.float32)
    nc = img[lay[2]:lay[2] + 4 * N].cpu().numpy().view(np.uint32)
    return fT, nc


# ---- 1. forward --------------------------------------------------------------------------------
@pytest.mark.parametrize("antialiasing", [False, True])
def test_alpha_matches_oracle(antialiasing):
    case = _default_case()
    o, _ = common.run_oracle(case, antialiasing=antialiasing, backward=False)
    t = _leaves(case, "sh_scales")
    with torch.no_grad():
        color, radii, inv, alpha = _dgr().GaussianRasterizer(_settings(case, antialiasing))(
            means2D=torch.zeros_like(t["means3D"]), return_alpha=True, **t)
    assert alpha.shape == (1, case["H"], case["W"]) and alpha.dtype == torch.float32
    ref = 1.0 - o.get("final_T").astype(np.float64)
    err = np.abs(alpha.cpu().numpy().astype(np.float64).reshape(-1) - ref)
    print(f"alpha vs oracle aa={antialiasing}: max err {err.max():.3e}")
    assert err.max() <= common.IMG_ATOL
    assert float(alpha.min()) >= 0.0 and 0.5 < float(alpha.max()) <= 1.0


@pytest.mark.parametrize("scene", list(SCENES))
def test_alpha_is_one_minus_final_T_and_leaves_the_outputs(scene):
    dgr = _dgr()
    case = SCENES[scene]()
    H, W = case["H"], case["W"]
    s = _settings(case)
    t = _leaves(case, "sh_scales")
    with torch.no_grad():
        m2 = torch.zeros_like(t["means3D"])
        plain = dgr.GaussianRasterizer(s)(means2D=m2, **t)
        color, radii, inv, alpha = dgr.GaussianRasterizer(s)(means2D=m2, return_alpha=True, **t)
        img = _c_forward(s, t)[5]
        direct = dgr._C.render_alpha([img], H, W)
    assert len(plain) == 3
    for a, b in zip(plain, (color, radii, inv)):
        assert torch.equal(a, b)
    fT, _ = _img_state(img, W, H)
    want = torch.from_numpy(np.float32(1.0) - fT).reshape(1, H, W)
    assert torch.equal(direct[0].cpu(), want), "render_alpha vs 1 - final_T of its image state"
    assert torch.equal(alpha.cpu(), want), "the node's alpha vs 1 - final_T"


def test_alpha_of_a_view_batch():
    dgr = _dgr()
    case = _stack_case(50, 70)
    cams = [synthetic.Camera(case["W"], case["H"], view=v) for v in range(3)]
    ss = [_settings(case, cam=c) for c in cams]
    t = _leaves(case, "sh_scales")
    P = t["means3D"].shape[0]
    with torch.no_grad():
        m2 = torch.zeros((3, P, 3), device=DEV)
        plain = dgr.MultiViewRasterizer(ss)(means2D=m2, **t)
        colors, radii, invs, alphas = dgr.MultiViewRasterizer(ss)(means2D=m2, return_alpha=True, **t)
        assert len(plain) == 3 and alphas.shape == (3, 1, case["H"], case["W"])
        for a, b in zip(plain, (colors, radii, invs)):
            assert torch.equal(a, b)
        for v, s in enumerate(ss):
            c, r, i, a = dgr.GaussianRasterizer(s)(means2D=m2[v], return_alpha=True, **t)
            fT, _ = _img_state(_c_forward(s, t)[5], case["W"], case["H"])
            assert torch.equal(alphas[v], a) and torch.equal(colors[v], c), f"view {v}"
            assert torch.equal(a.cpu().reshape(-1), torch.from_numpy(np.float32(1.0) - fT)), f"view {v}"


# ---- 2. the background identity, zero tolerance ------------------------------------------------
def _identity_grads(case, mode, with_alpha, gC, gI, camera=False, antialiasing=False):
    """Input gradients of run A (with_alpha: bg 0, the alpha gradient -(K_BG gC[0])) or run B (bg
    (K_BG, 0, 0), no alpha output) of the identity."""
    dgr = _dgr()
    s = _settings(case, antialiasing, bg=(0.0, 0.0, 0.0) if with_alpha else (K_BG, 0.0, 0.0))
    t = _leaves(case, mode)
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    kw = dict(t)
    if camera:
        t["cam_view"], t["cam_proj"], t["cam_pos"] = (
            x.clone().contiguous().requires_grad_(True) for x in (s.viewmatrix, s.projmatrix, s.campos))
        kw["camera"] = (t["cam_view"], t["cam_proj"], t["cam_pos"])
    out = dgr.GaussianRasterizer(s)(means2D=means2D, return_alpha=with_alpha, **kw)
    loss = (gC * out[0]).sum()
    if gI is not None:
        loss = loss + (gI * out[2]).sum()
    if with_alpha:
        gA = -(K_BG * gC[0])
        loss = loss + (gA * out[3][0]).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = {k: v.grad for k, v in t.items()}
    g["means2D"] = means2D.grad
    return g


def _assert_same_bits(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert a[k] is not None and b[k] is not None, f"{what}: no gradient for {k}"
        assert torch.equal(a[k], b[k]), \
            f"{what}: d{k} differs (max |diff| {float((a[k] - b[k]).abs().max()):.3e})"
        assert bool(torch.isfinite(a[k]).all())
    assert float(a["means3D"].abs().max()) > 0


IDENTITY = [pytest.param(scene, mode, inv, False, id=f"{scene}-{mode}-{'inv' if inv else 'noinv'}")
            for scene in SCENES for mode in ("sh_scales", "colors_cov") for inv in (False, True)] + \
           [pytest.param("stack50x70", "dc", False, False, id="stack50x70-dc"),
            pytest.param("stack37x50", "sh_scales", True, True, id="stack37x50-camera")]


@pytest.mark.parametrize("scene,mode,inv,camera", IDENTITY)
def test_alpha_gradient_is_the_background_term(scene, mode, inv, camera):
    case = SCENES[scene]()
    g = torch.Generator().manual_seed(5)
    gC = torch.randn(3, case["H"], case["W"], generator=g).to(DEV)
    gI = (torch.randn(1, case["H"], case["W"], generator=g) * 0.01).to(DEV) if inv else None
    a = _identity_grads(case, mode, True, gC, gI, camera)
    b = _identity_grads(case, mode, False, gC, gI, camera)
    _assert_same_bits(a, b, f"{scene} {mode}")
    if camera:
        assert float(a["cam_view"].abs().max()) > 0 and float(a["cam_proj"].abs().max()) > 0


def _views_state(case, ss, t, bg):
    """_C.rasterize_gaussians_views of the views `ss` with background bg: (Ls, geoms, bins, imgs, radii)."""
    dgr = _dgr()
    V, P, H, W = len(ss), t["means3D"].shape[0], case["H"], case["W"]
    out = (torch.empty((V, 3, H, W), device=DEV), torch.empty((V, P), dtype=torch.int32, device=DEV),
           torch.empty((V, 1, H, W), device=DEV))
    e = torch.Tensor([])
    s0 = ss[0]
    Ls, geoms, bins, imgs = dgr._C.rasterize_gaussians_views(
        bg, t["means3D"].detach(), e, t["opacities"].detach(), t["scales"].detach(), t["rotations"].detach(), 1.0, e,
        [s.viewmatrix for s in ss], [s.projmatrix for s in ss], [s.tanfovx for s in ss], [s.tanfovy for s in ss],
        H, W, t["shs"].detach(), s0.sh_degree, [s.campos for s in ss], False, False, False, out=out)
    return Ls, geoms, bins, imgs, out[1]


def test_alpha_gradient_in_one_view_of_a_batch():
    """Views of one launch with and without an alpha gradient (null and non-null pointers mixed): only
    view 1 has gC and gA, views 0 and 2 have gC = 0 and no alpha gradient; run B is the same batch
    with bg (K_BG, 0, 0) and no alpha gradient anywhere."""
    dgr = _dgr()
    case = _stack_case(50, 70)
    H, W = case["H"], case["W"]
    cams = [synthetic.Camera(W, H, view=v) for v in range(3)]
    ss = [_settings(case, cam=c) for c in cams]
    t = _leaves(case, "sh_scales")
    e = torch.Tensor([])
    g = torch.Generator().manual_seed(6)
    gC = torch.zeros(3, 3, H, W)
    gC[1] = torch.randn(3, H, W, generator=g)
    gC = gC.to(DEV)
    gA = -(K_BG * gC[1, 0])

    def backward(bg, alphas):
        bg = torch.tensor(bg, dtype=torch.float32, device=DEV)
        Ls, geoms, bins, imgs, radii = _views_state(case, ss, t, bg)
        return dgr._C.rasterize_gaussians_backward_views(
            bg, t["means3D"].detach(), [radii[v] for v in range(3)], e, t["opacities"].detach(), t["scales"].detach(),
            t["rotations"].detach(), 1.0, e, [s.viewmatrix for s in ss], [s.projmatrix for s in ss],
            [s.tanfovx for s in ss], [s.tanfovy for s in ss], gC, None, t["shs"].detach(), 3,
            [s.campos for s in ss], geoms, Ls, bins, imgs, False, False, dL_dout_alpha=alphas)

    a = backward((0.0, 0.0, 0.0), [None, gA.unsqueeze(0), None])
    b = backward((K_BG, 0.0, 0.0), None)
    torch.cuda.synchronize()
    assert len(a) == len(b) == 8
    for k, (x, y) in enumerate(zip(a, b)):
        assert torch.equal(x, y), f"gradient {k} of the batch differs"
    assert float(a[3].abs().max()) > 0

    # the same through the module: autograd hands the alpha gradient over as one stacked tensor
    def module(with_alpha):
        tt = _leaves(case, "sh_scales")
        m2 = torch.zeros((3, tt["means3D"].shape[0], 3), device=DEV, requires_grad=True)
        sv = ss if with_alpha else [_settings(case, bg=(K_BG, 0.0, 0.0), cam=c) for c in cams]
        out = dgr.MultiViewRasterizer(sv)(means2D=m2, return_alpha=with_alpha, **tt)
        loss = (gC * out[0]).sum()
        if with_alpha:
            loss = loss + (gA * out[3][1, 0]).sum()
        loss.backward()
        torch.cuda.synchronize()
        return dict({k: v.grad for k, v in tt.items()}, means2D=m2.grad)

    _assert_same_bits(module(True), module(False), "MultiViewRasterizer")


# ---- 3. oracle parity --------------------------------------------------------------------------
def _oracle_alpha_pass(case, mode, antialiasing, gA):
    """The reference's gradients of sum(gA * alpha): its render of the same geometry with colour 1
    and background 0 (channel 0 = 1 - final_T) under dL_dcolor = (gA, 0, 0)."""
    P = case["scene"]["means3D"].shape[0]
    c2 = dict(case, bg=torch.zeros(3), colors_precomp=torch.ones(P, 3),
              grad_color=torch.stack([gA, torch.zeros_like(gA), torch.zeros_like(gA)]), grad_invdepth=None)
    o, og = common.run_oracle(c2, "colors_scales" if mode.endswith("scales") else "colors_cov",
                              antialiasing=antialiasing)
    return o, og


def _geometry_checks(mode):
    checks = {"means3D": "dL_dmeans3D", "opacities": "dL_dopacity", "means2D": "dL_dmean2D"}
    if mode.endswith("scales"):
        checks.update(scales="dL_dscales", rotations="dL_drotations")
    else:
        checks["cov3D_precomp"] = "dL_dcov3D"
    return checks


def _hip_with_alpha(case, mode, antialiasing, gC, gI, gA):
    dgr = _dgr()
    s = _settings(case, antialiasing, bg=tuple(case["bg"].tolist()))
    t = _leaves(case, mode)
    means2D = torch.zeros_like(t["means3D"], requires_grad=True)
    color, radii, inv, alpha = dgr.GaussianRasterizer(s)(means2D=means2D, return_alpha=True, **t)
    loss = (alpha[0] * gA.to(DEV)).sum()
    if gC is not None:
        loss = loss + (color * gC.to(DEV)).sum() + (inv * gI.to(DEV)).sum()
    loss.backward()
    torch.cuda.synchronize()
    g = {k: (v.grad.cpu().numpy() if v.grad is not None else None) for k, v in t.items()}
    g["means2D"] = means2D.grad.cpu().numpy()
    fT, nc = _img_state(_c_forward(s, t)[5], case["W"], case["H"])
    render = {"color": color.detach().cpu().numpy(), "invdepth": inv.detach().cpu().numpy(), "final_T": fT,
              "n_contrib": nc}
    return g, render, alpha.detach().cpu().numpy()


def _check_against(name, case, o, g, ref, render):
    """allclose_rel at GRAD_RTOL / GRAD_ATOL per tensor; a tensor that misses it must owe that to
    flipped pixels (check_render's flips, check_grad_attributed)."""
    flips = []
    common.check_render(name, render, {"color": o.color, "invdepth": o.invdepth, "final_T": o.get("final_T"),
                                       "n_contrib": o.get("n_contrib")}, flips=flips)
    affected = None
    for hk, b in ref.items():
        a = g[hk]
        ok, rel = common.allclose_rel(a, b.reshape(a.shape))
        print(f"{name}: d{hk} rel {rel:.3e}")
        if not ok:
            if affected is None:
                affected = common.flip_gaussians(flips[0], render["n_contrib"], o.get("n_contrib"), o.get("vals"),
                                                 o.get("ranges"), case["W"], case["H"], a.shape[0])
            print(f"{name}: d{hk} beyond GRAD_RTOL, attributing to {int(flips[0].sum())} flipped pixels")
            common.check_grad_attributed(f"{name} d{hk}", a, b, affected)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("antialiasing", [False, True])
def test_alpha_gradient_matches_oracle(mode, antialiasing):
    case = _default_case()
    gA = synthetic.make_grads(case["H"], case["W"], seed=11)[0][0]
    o, og = common.run_oracle(case, mode, antialiasing=antialiasing)
    o2, og2 = _oracle_alpha_pass(case, mode, antialiasing, gA)
    np.testing.assert_array_equal(o2.get("n_contrib"), o.get("n_contrib"))
    assert np.abs(o2.color[0].reshape(-1).astype(np.float64) - (1.0 - o.get("final_T").astype(np.float64))).max() < 1e-6
    g, render, alpha = _hip_with_alpha(case, mode, antialiasing, case["grad_color"], case["grad_invdepth"], gA)
    ref = {hk: og[ok] + og2[ok] for hk, ok in _geometry_checks(mode).items()}
    if mode.startswith("sh"):
        ref["shs"] = og["dL_dsh"]
    else:
        ref["colors_precomp"] = og["dL_dcolors"]
    _check_against(f"alpha {mode} aa={antialiasing}", case, o, g, ref, render)


def test_alpha_only_loss_matches_oracle():
    """No colour and no invdepth gradient (autograd hands the node None for both): the second pass alone."""
    case = _default_case()
    gA = synthetic.make_grads(case["H"], case["W"], seed=11)[0][0]
    o, _ = common.run_oracle(case, "sh_scales", backward=False)
    o2, og2 = _oracle_alpha_pass(case, "sh_scales", False, gA)
    g, render, alpha = _hip_with_alpha(case, "sh_scales", False, None, None, gA)
    assert g["shs"] is None or not np.any(g["shs"]), "alpha does not depend on the colours"
    ref = {hk: og2[ok] for hk, ok in _geometry_checks("sh_scales").items()}
    _check_against("alpha only", case, o, g, ref, render)


# ---- 4. deferred -------------------------------------------------------------------------------
def test_alpha_gradient_through_deferred_backward():
    dgr = _dgr()
    case = _stack_case(50, 70)
    H, W = case["H"], case["W"]
    cams = [synthetic.Camera(W, H, view=v) for v in range(2)]
    ss = [_settings(case, bg=(0.1, 0.2, 0.3), cam=c) for c in cams]
    grads = [synthetic.make_grads(H, W, seed=40 + v) for v in range(2)]
    gC = torch.stack([g[0] for g in grads]).to(DEV)
    gI = torch.stack([g[1] for g in grads]).to(DEV)
    gA = torch.stack([synthetic.make_grads(H, W, seed=50 + v)[0][:1] for v in range(2)]).to(DEV)

    batch = _leaves(case, "sh_scales")
    P = batch["means3D"].shape[0]
    m2b = torch.zeros((2, P, 3), device=DEV, requires_grad=True)
    c, r, i, a = dgr.MultiViewRasterizer(ss)(means2D=m2b, return_alpha=True, **batch)
    torch.autograd.backward([c, i, a], [gC, gI, gA])

    late = _leaves(case, "sh_scales")
    m2 = [torch.zeros((P, 3), device=DEV, requires_grad=True) for _ in range(2)]
    with dgr.deferred_backward():
        for v, s in enumerate(ss):
            c, r, i, a = dgr.GaussianRasterizer(s)(means2D=m2[v], return_alpha=True, **late)
            torch.autograd.backward([c, i, a], [gC[v], gI[v], gA[v]])
    torch.cuda.synchronize()
    for k in batch:
        assert torch.equal(late[k].grad, batch[k].grad), f"d{k}: deferred vs MultiViewRasterizer"
    for v in range(2):
        assert torch.equal(m2[v].grad, m2b.grad[v]), f"means2D of view {v}"

    # and the alpha term is in there: the same views without it give other gradients
    plain = _leaves(case, "sh_scales")
    m2p = torch.zeros((2, P, 3), device=DEV, requires_grad=True)
    c, r, i = dgr.MultiViewRasterizer(ss)(means2D=m2p, **plain)
    torch.autograd.backward([c, i], [gC, gI])
    assert not torch.equal(plain["opacities"].grad, batch["opacities"].grad)


# ---- 5. surface --------------------------------------------------------------------------------
def test_alpha_surface():
    dgr = _dgr()
    case = _stack_case(37, 50)
    H, W = case["H"], case["W"]
    s = _settings(case)
    t = _leaves(case, "sh_scales")
    m2 = torch.zeros_like(t["means3D"])
    assert len(dgr.GaussianRasterizer(s)(means2D=m2, **t)) == 3
    assert len(dgr.MultiViewRasterizer([s, s])(means2D=torch.zeros((2,) + m2.shape, device=DEV), **t)) == 3
    with torch.no_grad():
        out = dgr.GaussianRasterizer(s)(means2D=m2, return_alpha=True, **t)
    assert len(out) == 4 and not out[3].requires_grad and out[3].shape == (1, H, W)
    # no Gaussians: nothing accumulated
    empty = {k: v.detach()[:0] for k, v in t.items()}
    out0 = dgr.GaussianRasterizer(s)(means2D=m2[:0], return_alpha=True, **empty)
    assert len(out0) == 4 and out0[3].shape == (1, H, W) and not bool(out0[3].any())

    L, color, radii, geom, binning, img, inv = _c_forward(s, t)
    e = torch.Tensor([])
    gC = torch.zeros(3, H, W, device=DEV)

    def backward(ga):
        return dgr._C.rasterize_gaussians_backward(
            s.bg, t["means3D"].detach(), radii, e, t["opacities"].detach(), t["scales"].detach(),
            t["rotations"].detach(), 1.0, e, s.viewmatrix, s.projmatrix, s.tanfovx, s.tanfovy, gC, e,
            t["shs"].detach(), 3, s.campos, geom, L, binning, img, False, False, dL_dout_alpha=ga)

    for bad in (torch.zeros(1, H, W), torch.zeros(1, H, W + 1, device=DEV), torch.zeros(3, H, W, device=DEV),
                torch.zeros(1, H, W, device=DEV, dtype=torch.float64)):
        with pytest.raises(RuntimeError):
            backward(bad)
        with pytest.raises(RuntimeError):
            dgr._C.rasterize_gaussians_render_backward(s.bg, t["means3D"].shape[0], L, geom, binning, img, gC, e,
                                                       False, dL_dout_alpha=bad)
    with pytest.raises(RuntimeError):
        dgr._C.render_alpha([img], H, W + 16)
    ok = backward(torch.ones(1, H, W, device=DEV))
    torch.cuda.synchronize()
    assert float(ok[2].abs().max()) > 0  # dL_dopacity: more opacity, more alpha
