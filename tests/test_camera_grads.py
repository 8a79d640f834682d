"""Camera pose gradients on the GPU (needs an MI355X: -m gpu): dL/dviewmatrix, dL/dprojmatrix and
dL/dcampos of GaussianRasterizer(camera=) / MultiViewRasterizer(cameras=) and of the C entry point
gsr_backward_camera_views.

1. against float64 autograd of tests/dense_ref.py (view, proj and campos three independent leaves);
2. the translation identity (no reference: covers clamped and culled Gaussians and a larger P);
3. with camera= set, everything that is not new is bit-identical to the call without it;
4. reproducible bit for bit, a view's gradient the same alone or inside a batch;
5. the C ABI driven through ctypes, with a poisoned workspace;
6. a pose refinement loop end to end.
"""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import camera_cases as cc
import common
import synthetic

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0") if torch.cuda.is_available() else None
MODES = ("sh_scales", "dc", "colors_cov")


def _settings(cam, case, antialiasing):
    import diff_gaussian_rasterization as dgr
    return dgr.GaussianRasterizationSettings(
        case["H"], case["W"], cam.tanfovx, cam.tanfovy, case["bg"].to(DEV), 1.0, cam.world_view_transform.to(DEV),
        cam.full_proj_transform.to(DEV), case["sh_degree"], cam.camera_center.to(DEV), False, False, antialiasing)


def _leaves(case, mode):
    sc = case["scene"]
    t = {"means3D": sc["means3D"], "opacities": sc["opacities"]}
    if mode == "dc":
        t["dc"], t["shs"] = sc["shs"][:, :1].contiguous(), sc["shs"][:, 1:].contiguous()
    elif mode == "sh_scales":
        t["shs"] = sc["shs"]
    else:
        t["colors_precomp"] = case["colors_precomp"]
    if mode == "colors_cov":
        t["cov3D_precomp"] = case["cov3D_precomp"]
    else:
        t["scales"], t["rotations"] = sc["scales"], sc["rotations"]
    return {k: v.to(DEV).clone().requires_grad_(True) for k, v in t.items()}


def _camera_leaves(cam, grad=(True, True, True)):
    return tuple(t.to(DEV).contiguous().clone().requires_grad_(g)
                 for t, g in zip((cam.world_view_transform, cam.full_proj_transform, cam.camera_center), grad))


def _single(case, cam, mode, antialiasing, gc, gi, camera=True, leaves=None, triple=None):
    """One view forward + backward; gi None: no inverse-depth gradient.  Returns the outputs, the
    leaves and the camera leaves (None without camera=)."""
    import diff_gaussian_rasterization as dgr
    leaves = _leaves(case, mode) if leaves is None else leaves
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    if camera and triple is None:
        triple = _camera_leaves(cam)
    kw = {"camera": triple} if camera else {}
    color, radii, inv = dgr.GaussianRasterizer(_settings(cam, case, antialiasing))(means2D=means2D, **leaves, **kw)
    if gi is None:
        color.backward(gc.to(DEV))
    else:
        torch.autograd.backward([color, inv], [gc.to(DEV), gi.to(DEV)])
    torch.cuda.synchronize()
    return dict(color=color.detach(), radii=radii, inv=inv.detach(), means2D=means2D, leaves=leaves, triple=triple)


# ---- 1. against float64 autograd ------------------------------------------------------------------------------

@pytest.mark.parametrize("with_invdepth", [True, False])
@pytest.mark.parametrize("antialiasing", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_camera_grads_match_float64_autograd(mode, antialiasing, with_invdepth):
    """The recipe scene, ring views 0 and 3, against dense_ref with aa_quirk=True (the HIP chain keeps
    the reference's AA rule), the upstream gradients zeroed at the reference's tie pixels on both
    sides.  Bound: common.allclose_rel at rtol 2e-4, atol 1e-7 of each tensor's max-abs, the project's
    bound for an fp32 backward against this reference (test_oracle.py:85)."""
    case = cc.recipe()
    kind = "colors_cov" if mode == "colors_cov" else "sh"
    for view in cc.RECIPE_VIEWS:
        ref = cc.dense_camera_grads_cached(1.0, view, kind, antialiasing, with_invdepth)
        # conditions on the reference alone
        assert float(ref["tie"].double().mean()) < 1e-2
        assert ref["clamped"] == 0, "a visible Gaussian is frustum-clamped: covered by the identity test"
        assert ref["alpha_max"] < 0.99
        keep = (~ref["tie"]).reshape(1, case["H"], case["W"]).float()
        r = _single(case, cc.camera(view), mode, antialiasing, case["grad_color"] * keep,
                    case["grad_invdepth"] * keep if with_invdepth else None)
        g_view, g_proj, g_campos = (t.grad.cpu() for t in r["triple"])
        # structural zeros, exactly
        assert torch.count_nonzero(g_view[:, 3]) == 0 and torch.count_nonzero(g_proj[:, 2]) == 0
        if mode == "colors_cov":
            assert torch.count_nonzero(g_campos) == 0
        ok_m, rel_m = common.allclose_rel(r["leaves"]["means3D"].grad.cpu().numpy(), ref["means3D"].numpy(),
                                          rtol=2e-4, atol=1e-7)
        rels, oks = {}, {}
        for name, g in (("view", g_view), ("proj", g_proj), ("campos", g_campos)):
            oks[name], rels[name] = common.allclose_rel(g.numpy(), ref[name].numpy(), rtol=2e-4, atol=1e-7)
        common.PARITY_LOG.append({"name": f"camera grads vs float64 {mode} aa={antialiasing} inv={with_invdepth} "
                                          f"view={view}", "rel_dview": rels["view"], "rel_dproj": rels["proj"],
                                  "rel_dcampos": rels["campos"], "rel_dmeans3D": rel_m})
        print(f"camera grads {mode} aa={antialiasing} inv={with_invdepth} view={view}: dview {rels['view']:.3e} "
              f"dproj {rels['proj']:.3e} dcampos {rels['campos']:.3e} (dmeans3D {rel_m:.3e})")
        for name in rels:
            assert oks[name], (f"{mode} aa={antialiasing} inv={with_invdepth} view {view}: dL/d{name} vs float64 "
                               f"autograd rel {rels[name]:.3e} (dL/dmeans3D on the same case: {rel_m:.3e})")


# ---- 2. translation identity ----------------------------------------------------------------------------------

# |lhs - rhs| / S per component, S = sum_i |dL/dmeans3D[i]| (the scale of the fp32 rounding of both
# sums).  Measured on an MI355X over the cases below (largest per scene; the results are bitwise
# reproducible): recipe 1.41e-8, the 5000-Gaussian cloud 4.72e-9, the spread variant with its clamped
# Gaussians 3.46e-8 (DESIGN.md carries the same numbers).  The bound is 4x the largest.  A ratio
# above 1e-4 (common.GRAD_RTOL) would mean a wrong term, not rounding.
IDENTITY_MEASURED = {"recipe": 1.412e-8, "p5000": 4.722e-9, "spread": 3.460e-8}
IDENTITY_RATIO = 4 * max(IDENTITY_MEASURED.values())
assert IDENTITY_RATIO < common.GRAD_RTOL


# camera_bwd_finish_kernel sums a view's nwg = ceil(P / 256) workgroup rows in 32 strands, each
# reading rows s + 32 u (u < 8) per trip of a loop that advances by 256 rows.  Up to 32 rows only
# u = 0 holds data; 33 rows (32 * 256 + 37 Gaussians) give strand 0 a u = 1 row; 293 rows
# (292 * 256 + 37) give every strand a second trip, and strands 0..4 a u = 1 row in it.
P_NWG33, P_NWG293 = 32 * 256 + 37, 292 * 256 + 37
H_CLOUD, W_CLOUD = 144, 176


@functools.lru_cache(maxsize=None)
def _cloud_case(P):
    """common.make_case's cloud of P small Gaussians at 144x176, with precomputed colours and
    covariances for the colors_cov mode."""
    case = common.make_case(P=P, H=H_CLOUD, W=W_CLOUD)
    g = torch.Generator().manual_seed(5)
    case["colors_precomp"] = torch.rand(P, 3, generator=g)
    case["cov3D_precomp"] = cc.cov3d_of(case["scene"]["scales"], case["scene"]["rotations"])
    return case


def _identity_case(scene):
    if scene == "recipe":
        return cc.recipe(), [cc.camera(v) for v in cc.RECIPE_VIEWS]
    if scene == "spread":
        return cc.recipe(4.0), [cc.camera(v) for v in cc.RECIPE_VIEWS]
    case = _cloud_case({"p5000": 5000, "p74789": P_NWG293}[scene])
    return case, [case["cam"]]


@pytest.mark.parametrize("mode,antialiasing", [("sh_scales", False), ("sh_scales", True), ("dc", True),
                                               ("colors_cov", False)])
@pytest.mark.parametrize("scene", ["recipe", "p5000", "spread", "p74789"])
def test_translation_identity(scene, mode, antialiasing):
    """Moving the camera centre by d equals moving every mean by -d:
    dL/dcampos - R dL/dview[3,:3] - (R Pm[:3,:]) dL/dproj[3,:] == -sum_i dL/dmeans3D[i]
    (cc.translation_identity; float64 on dense_ref: test_camera_grads_cpu.py).  The recipe, a larger
    cloud of small Gaussians (many culled, 20 workgroups) and the spread variant, whose clamped
    visible Gaussians are asserted.  The cloud of 74,789 (293 workgroups: two trips of the finish
    kernel's row loop) is held to common.GRAD_RTOL, the bound of a wrong term, not to a measurement:
    its tight bound is test_finish_kernel_sums_every_workgroup_row."""
    case, cams = _identity_case(scene)
    for cam in cams:
        r = _single(case, cam, mode, antialiasing, case["grad_color"], case["grad_invdepth"])
        vis = r["radii"].cpu() > 0
        assert 0 < int(vis.sum()) < len(vis), "some Gaussians visible, some culled"
        if scene == "spread":
            assert int(cc.clamped_visible(case["scene"]["means3D"], cam, r["radii"].cpu()).sum()) >= 1
        g_view, g_proj, g_campos = (t.grad.cpu() for t in r["triple"])
        lhs, rhs, S = cc.translation_identity(g_view, g_proj, g_campos, r["leaves"]["means3D"].grad.cpu(), cam)
        ratio = float(((lhs - rhs).abs() / S).max())
        common.PARITY_LOG.append({"name": f"camera translation identity {scene} {mode} aa={antialiasing}",
                                  "ratio": ratio, "visible": int(vis.sum())})
        print(f"translation identity {scene} {mode} aa={antialiasing}: ratio {ratio:.3e} visible {int(vis.sum())}")
        assert float(S.min()) > 0
        bound = common.GRAD_RTOL if scene == "p74789" else IDENTITY_RATIO
        assert ratio <= bound, f"{scene} {mode} aa={antialiasing}: identity off by {ratio:.3e} of S"


# ---- 3. exactness of what is not new --------------------------------------------------------------------------

def _equal_runs(a, b):
    assert torch.equal(a["color"], b["color"]) and torch.equal(a["inv"], b["inv"])
    assert torch.equal(a["radii"], b["radii"])
    assert torch.equal(a["means2D"].grad, b["means2D"].grad)
    for k in a["leaves"]:
        assert torch.equal(a["leaves"][k].grad, b["leaves"][k].grad), f"d{k} changed with camera="


@pytest.mark.parametrize("mode,antialiasing", [("sh_scales", False), ("dc", True), ("colors_cov", False)])
def test_camera_keyword_changes_nothing_else_single(mode, antialiasing):
    case, cam = cc.recipe(), cc.camera(3)
    plain = _single(case, cam, mode, antialiasing, case["grad_color"], case["grad_invdepth"], camera=False)
    with_cam = _single(case, cam, mode, antialiasing, case["grad_color"], case["grad_invdepth"])
    _equal_runs(plain, with_cam)


def _few_camera(W, H):
    """Ring view 5 turned 50 degrees about its own y axis: most of the cloud leaves the image
    (dense_ref: 65 of 549 Gaussians visible, 5 of them clamped)."""
    ring = synthetic.Camera(W, H, 5)
    R, T = synthetic.ring_camera_RT(5)
    C = -R @ T
    a = math.radians(50.0)
    Ry = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    R2 = R @ Ry
    return synthetic.Camera(W, H, R=R2, T=-R2.T @ C, fovx=ring.FoVx, fovy=ring.FoVy)


def _batch(case, cams, mode, antialiasing, gcs, gis, cameras, leaves=None, as_list=False):
    import diff_gaussian_rasterization as dgr
    leaves = _leaves(case, mode) if leaves is None else leaves
    V, P = len(cams), case["scene"]["means3D"].size(0)
    means2D = torch.zeros((V, P, 3), device=DEV, requires_grad=True)
    triples = [_camera_leaves(c) for c in cams] if cameras else None
    kw = {}
    if cameras:
        kw["cameras"] = triples if as_list else tuple(torch.stack([t[k] for t in triples]) for k in range(3))
    color, radii, inv = dgr.MultiViewRasterizer([_settings(c, case, antialiasing) for c in cams])(
        means2D=means2D, **leaves, **kw)
    torch.autograd.backward([color, inv], [gcs.to(DEV), gis.to(DEV)])
    torch.cuda.synchronize()
    return dict(color=color.detach(), radii=radii, inv=inv.detach(), means2D=means2D, leaves=leaves, triples=triples)


def _batch_grads(V, H, W):
    gs = [synthetic.make_grads(H, W, seed=40 + v) for v in range(V)]
    return torch.stack([g[0] for g in gs]), torch.stack([g[1] for g in gs])


@pytest.mark.parametrize("mode,antialiasing", [("sh_scales", True), ("dc", False)])
def test_camera_keyword_changes_nothing_else_batch(mode, antialiasing):
    case = cc.recipe()
    cams = [cc.camera(0), cc.camera(3), _few_camera(case["W"], case["H"])]
    gcs, gis = _batch_grads(3, case["H"], case["W"])
    plain = _batch(case, cams, mode, antialiasing, gcs, gis, cameras=False)
    with_cam = _batch(case, cams, mode, antialiasing, gcs, gis, cameras=True)
    _equal_runs(plain, with_cam)


def test_camera_keyword_changes_nothing_else_accumulating():
    """Under accumulate_grads_in_place(): two single views and a batch of three added into the same
    .grad buffers, with and without camera= / cameras=."""
    import diff_gaussian_rasterization as dgr
    case = cc.recipe()
    cams = [cc.camera(0), cc.camera(3), _few_camera(case["W"], case["H"])]
    gcs, gis = _batch_grads(3, case["H"], case["W"])
    runs = []
    for camera in (False, True):
        leaves = _leaves(case, "sh_scales")
        outs = []
        with dgr.accumulate_grads_in_place():
            for v in (0, 1):
                outs.append(_single(case, cams[v], "sh_scales", False, gcs[v], gis[v], camera=camera, leaves=leaves))
            outs.append(_batch(case, cams, "sh_scales", False, gcs, gis, cameras=camera, leaves=leaves))
        runs.append(outs)
        if camera:
            assert all(t.grad is not None for t in outs[0]["triple"])
    for a, b in zip(*runs):
        _equal_runs(a, b)


# ---- 4. reproducibility and batching ----------------------------------------------------------------------------

def test_camera_grads_reproducible_and_batch_equals_single():
    import diff_gaussian_rasterization as dgr
    case = cc.recipe()
    H, W = case["H"], case["W"]
    cams = [cc.camera(0), cc.camera(3), _few_camera(W, H)]
    gcs, gis = _batch_grads(3, H, W)
    # two backward passes of the same graph
    leaves = _leaves(case, "sh_scales")
    triple = _camera_leaves(cams[0])
    means2D = torch.zeros_like(leaves["means3D"], requires_grad=True)
    color, _, inv = dgr.GaussianRasterizer(_settings(cams[0], case, True))(means2D=means2D, camera=triple, **leaves)
    passes = [torch.autograd.grad([color, inv], triple, [gcs[0].to(DEV), gis[0].to(DEV)], retain_graph=True)
              for _ in range(2)]
    for a, b in zip(*passes):
        assert torch.equal(a, b)
    assert all(float(g.abs().max()) > 0 for g in passes[0])
    # a batch of three (a non-power-of-two, the last view seeing few Gaussians) against the single views
    for as_list in (False, True):
        batch = _batch(case, cams, "sh_scales", True, gcs, gis, cameras=True, as_list=as_list)
        n_vis = (batch["radii"] > 0).sum(1).tolist()
        assert 0 < n_vis[2] < 100 < n_vis[0], n_vis
        for v, cam in enumerate(cams):
            single = _single(case, cam, "sh_scales", True, gcs[v], gis[v])
            for k in range(3):
                assert torch.equal(batch["triples"][v][k].grad, single["triple"][k].grad), (v, k)
    for a, b in zip(passes[0], single["triple"]):
        assert a.shape == b.grad.shape
    # a camera tensor without requires_grad gets None
    triple = _camera_leaves(cams[1], grad=(True, False, True))
    r = _single(case, cams[1], "sh_scales", False, gcs[1], gis[1], triple=triple)
    assert r["triple"][1].grad is None and r["triple"][0].grad is not None and r["triple"][2].grad is not None
    full = _single(case, cams[1], "sh_scales", False, gcs[1], gis[1])
    assert torch.equal(r["triple"][0].grad, full["triple"][0].grad)
    assert torch.equal(r["triple"][2].grad, full["triple"][2].grad)


def _cloud_cameras():
    return [cc.camera(0, W_CLOUD, H_CLOUD), cc.camera(3, W_CLOUD, H_CLOUD), _few_camera(W_CLOUD, H_CLOUD)]


def test_camera_grads_batch_equals_single_past_256_workgroups():
    """The batch-equals-single check above at 74,789 Gaussians: 293 workgroup rows per view, so the
    finish kernel's row loop makes two trips and view v's rows start at 293 v."""
    case, cams = _cloud_case(P_NWG293), _cloud_cameras()
    gcs, gis = _batch_grads(3, H_CLOUD, W_CLOUD)
    batch = _batch(case, cams, "sh_scales", True, gcs, gis, cameras=True)
    assert all(n > 0 for n in (batch["radii"] > 0).sum(1).tolist())
    for v, cam in enumerate(cams):
        single = _single(case, cam, "sh_scales", True, gcs[v], gis[v])
        for k in range(3):
            assert float(single["triple"][k].grad.abs().max()) > 0
            assert torch.equal(batch["triples"][v][k].grad, single["triple"][k].grad), (v, k)


# ---- 5. C ABI ---------------------------------------------------------------------------------------------------

def test_c_abi_camera_views():
    """gsr_backward_camera_views through ctypes after gsr_backward_dc, its workspace poisoned with
    NaNs: identical to the Python path; the workspace size is monotone in V and P."""
    from diff_gaussian_rasterization import _C
    lib = _C.lib
    case, cam = cc.recipe(), cc.camera(0)
    H, W, P = case["H"], case["W"], cc.P_RECIPE
    sc = {k: v.to(DEV).contiguous() for k, v in case["scene"].items()}
    view, proj, campos = (t.to(DEV).contiguous() for t in (cam.world_view_transform, cam.full_proj_transform,
                                                            cam.camera_center))
    bg = case["bg"].to(DEV)
    empty = torch.Tensor([])
    L, color, radii, geom, binning, img, inv = _C.rasterize_gaussians(
        bg, sc["means3D"], empty, sc["opacities"], sc["scales"], sc["rotations"], 1.0, empty, view, proj, cam.tanfovx,
        cam.tanfovy, H, W, sc["shs"], 3, campos, False, False, False)
    gc, gi = case["grad_color"].to(DEV).contiguous(), case["grad_invdepth"].to(DEV).contiguous()
    out = {k: torch.empty(n, device=DEV) for k, n in (("m2", 3 * P), ("conic", 4 * P), ("op", P), ("col", 3 * P),
                                                       ("inv", P), ("m3", 3 * P), ("cov", 6 * P), ("sh", 48 * P),
                                                       ("sc", 3 * P), ("rot", 4 * P))}
    stream = torch.cuda.current_stream(DEV).cuda_stream
    rc = lib.gsr_backward_dc(
        P, 3, 16, int(L), bg.data_ptr(), W, H, sc["means3D"].data_ptr(), None, sc["shs"].data_ptr(), None,
        sc["opacities"].data_ptr(), sc["scales"].data_ptr(), 1.0, sc["rotations"].data_ptr(), None, view.data_ptr(),
        proj.data_ptr(), campos.data_ptr(), cam.tanfovx, cam.tanfovy, radii.data_ptr(), geom.data_ptr(),
        binning.data_ptr(), img.data_ptr(), gc.data_ptr(), gi.data_ptr(), out["m2"].data_ptr(),
        out["conic"].data_ptr(), out["op"].data_ptr(), out["col"].data_ptr(), out["inv"].data_ptr(),
        out["m3"].data_ptr(), out["cov"].data_ptr(), None, out["sh"].data_ptr(), out["sc"].data_ptr(),
        out["rot"].data_ptr(), False, False, stream)
    assert rc == 0, lib.gsr_last_error()
    sizes = [[lib.gsr_camera_grad_workspace_size(V, n) for n in (0, 1, 256, 257, P, 5000, 1 << 20)] for V in (1, 3, 16)]
    for row in sizes:
        assert all(a <= b for a, b in zip(row, row[1:])) and row[-1] > row[1]
    assert all(x <= y for a, b in zip(sizes, sizes[1:]) for x, y in zip(a, b))
    ws = torch.full((lib.gsr_camera_grad_workspace_size(1, P) // 4,), float("nan"), device=DEV)
    g = [torch.full((n,), float("nan"), device=DEV) for n in (16, 16, 3)]
    vp = ctypes.c_void_p
    rc = lib.gsr_backward_camera_views(
        1, P, 3, 16, (ctypes.c_int * 1)(int(L)), W, H, sc["means3D"].data_ptr(), None, sc["shs"].data_ptr(), None,
        sc["opacities"].data_ptr(), sc["scales"].data_ptr(), 1.0, sc["rotations"].data_ptr(), None,
        (vp * 1)(view.data_ptr()), (vp * 1)(proj.data_ptr()), (vp * 1)(campos.data_ptr()),
        (ctypes.c_float * 1)(cam.tanfovx), (ctypes.c_float * 1)(cam.tanfovy), (vp * 1)(geom.data_ptr()),
        (vp * 1)(binning.data_ptr()), True, False, ws.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
        False, stream)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    py = _single(case, cam, "sh_scales", False, case["grad_color"], case["grad_invdepth"])
    assert torch.equal(out["m3"].view(P, 3), py["leaves"]["means3D"].grad)
    for a, b in zip(g, py["triple"]):
        assert torch.equal(a.view(b.shape), b.grad)
    # refusals: status and message, no exception
    assert lib.gsr_backward_camera_views(
        0, P, 3, 16, (ctypes.c_int * 1)(int(L)), W, H, sc["means3D"].data_ptr(), None, sc["shs"].data_ptr(), None,
        sc["opacities"].data_ptr(), sc["scales"].data_ptr(), 1.0, sc["rotations"].data_ptr(), None,
        (vp * 1)(view.data_ptr()), (vp * 1)(proj.data_ptr()), (vp * 1)(campos.data_ptr()),
        (ctypes.c_float * 1)(cam.tanfovx), (ctypes.c_float * 1)(cam.tanfovy), (vp * 1)(geom.data_ptr()),
        (vp * 1)(binning.data_ptr()), True, False, ws.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(),
        False, stream) == 1
    assert b"V must be in [1, 16]" in lib.gsr_last_error()
    # the new profile id follows the existing ones
    lib.gsr_profile_kernel_name.restype = ctypes.c_char_p
    assert lib.gsr_profile_kernel_name(10) == b"camera_bwd" and lib.gsr_profile_kernel_name(8) == b"preprocess_bwd"
    assert lib.gsr_profile_kernel_name(9) == b"tile_order" and lib.gsr_profile_kernel_name(11) == b""


CAM_ROW, CAM_SUMS = 32, 27  # floats per workgroup row of the workspace; the sums a row carries


def _sums_of(g_view, g_proj, g_campos):
    """The 27 sums as the finish kernel lays them out, (V, 27) float64: dL/dview[r][c] (c < 3) at
    3 r + c, columns 0, 1 and 3 of dL/dproj[r] at 12 + 3 r + (0, 1, 2), dL/dcampos at 24..26."""
    return torch.cat([g_view[:, :, :3].reshape(-1, 12), g_proj[:, :, [0, 1, 3]].reshape(-1, 12), g_campos],
                     dim=1).double()


@pytest.mark.parametrize("P", [P_NWG33, P_NWG293], ids=["nwg33", "nwg293"])
def test_finish_kernel_sums_every_workgroup_row(P):
    """camera_bwd_finish_kernel against the float64 sum of the very rows it reads: the caller's
    workspace of gsr_backward_camera_views, (V, nwg, 32) floats, read back after the call.  V = 1 and
    V = 3 (ring views 0 and 3 and the view that sees few Gaussians), SH colours with scales.

    Bound, derived: an output is a chain of at most 8 ceil(nwg / 256) + 31 fp32 additions (a strand's
    trips of eight rows, then the 32 strands in order), so |out - ref| <= (8 ceil(nwg / 256) + 32) 2^-24
    sum_r |row r|.  The rows of a later u (32..63) and of the second trip (256 on) must hold data and,
    in some sum, more than twice that bound: leaving them out, or adding one twice, cannot pass.
    Columns 27..31 of a row are never read: the outputs are the same bits with NaN, 1e30 and NaN
    again there."""
    from diff_gaussian_rasterization import _C
    lib = _C.lib
    case, cams = _cloud_case(P), _cloud_cameras()
    H, W, nwg = H_CLOUD, W_CLOUD, (P + 255) // 256
    sc = {k: v.to(DEV).contiguous() for k, v in case["scene"].items()}
    bg, empty = case["bg"].to(DEV), torch.Tensor([])
    gcs, gis = _batch_grads(3, H, W)
    state = []  # per view: the camera on the device, num_rendered and the buffers after the render backward
    for v, cam in enumerate(cams):
        t = [x.to(DEV).contiguous() for x in (cam.world_view_transform, cam.full_proj_transform, cam.camera_center)]
        L, _, radii, geom, binning, img, _ = _C.rasterize_gaussians(
            bg, sc["means3D"], empty, sc["opacities"], sc["scales"], sc["rotations"], 1.0, empty, t[0], t[1],
            cam.tanfovx, cam.tanfovy, H, W, sc["shs"], 3, t[2], False, False, False)
        _C.rasterize_gaussians_backward(
            bg, sc["means3D"], radii, empty, sc["opacities"], sc["scales"], sc["rotations"], 1.0, empty, t[0], t[1],
            cam.tanfovx, cam.tanfovy, gcs[v].to(DEV).contiguous(), gis[v].to(DEV).contiguous(), sc["shs"], 3, t[2],
            geom, L, binning, img, False, False)
        assert L > 0
        state.append((t, int(L), geom, binning, cam))
    stream = torch.cuda.current_stream(DEV).cuda_stream
    vp = ctypes.c_void_p
    for V in (1, 3):
        assert lib.gsr_camera_grad_workspace_size(V, P) == V * nwg * CAM_ROW * 4
        st = state[:V]
        ws = torch.full((V, nwg, CAM_ROW), float("nan"), device=DEV)

        def run():
            g = [torch.full((V,) + s, float("nan"), device=DEV) for s in ((4, 4), (4, 4), (3,))]
            rc = lib.gsr_backward_camera_views(
                V, P, 3, 16, (ctypes.c_int * V)(*[s[1] for s in st]), W, H, sc["means3D"].data_ptr(), None,
                sc["shs"].data_ptr(), None, sc["opacities"].data_ptr(), sc["scales"].data_ptr(), 1.0,
                sc["rotations"].data_ptr(), None, (vp * V)(*[s[0][0].data_ptr() for s in st]),
                (vp * V)(*[s[0][1].data_ptr() for s in st]), (vp * V)(*[s[0][2].data_ptr() for s in st]),
                (ctypes.c_float * V)(*[s[4].tanfovx for s in st]), (ctypes.c_float * V)(*[s[4].tanfovy for s in st]),
                (vp * V)(*[s[2].data_ptr() for s in st]), (vp * V)(*[s[3].data_ptr() for s in st]), True, False,
                ws.data_ptr(), g[0].data_ptr(), g[1].data_ptr(), g[2].data_ptr(), False, stream)
            assert rc == 0, lib.gsr_last_error()
            torch.cuda.synchronize()
            return [t.cpu() for t in g], ws.cpu()

        g, rows = run()
        assert bool(torch.isfinite(rows[:, :, :CAM_SUMS]).all()), "a sum of a row was not written"
        assert bool(rows[:, :, CAM_SUMS:].isnan().all()), "a row is 27 sums: the rest is the caller's"
        # conditions on the rows: the later loads and trips carry data that the bound cannot hide
        r64 = rows[:, :, :CAM_SUMS].double()
        ref, mag = r64.sum(1), r64.abs().sum(1)
        bound = (8 * ((nwg + 255) // 256) + 32) * 2.0 ** -24 * mag
        for lo, hi in ((32, 64), (256, nwg)):
            if lo < nwg:
                part = r64[:, lo:hi]
                assert bool((part != 0).flatten(1).any(1).all()), (V, lo)
                assert bool((part.sum(1).abs() > 2 * bound).any(1).all()), (V, lo)
        # the structural zeros, exactly
        assert torch.count_nonzero(g[0][:, :, 3]) == 0 and torch.count_nonzero(g[1][:, :, 2]) == 0
        err = (_sums_of(*g) - ref).abs()
        worst = float((err / bound.clamp_min(1e-300)).max())
        print(f"finish kernel P={P} V={V}: max |out - float64 sum| / bound {worst:.3f}")
        assert bool((err <= bound).all()), (V, worst)
        # columns 27..31 are not read
        for fill in (1e30, float("nan")):
            ws[:, :, CAM_SUMS:] = fill
            g2, rows2 = run()
            assert torch.equal(rows2[:, :, :CAM_SUMS], rows[:, :, :CAM_SUMS])
            assert all(torch.equal(a, b) for a, b in zip(g, g2)), fill


# ---- 6. pose refinement end to end ------------------------------------------------------------------------------

def test_pose_refinement_reduces_loss_and_pose_error():
    """The recipe scene at 160x112; target: the render from ring view 0; start: pose_camera(cam,
    delta0), delta0 = (0.01, -0.015, 0.008 | 0.03, -0.02, 0.04); K = 20 Adam steps, lr 2e-3, on delta
    with the L1 image loss.  The identical loop on dense_ref in float64 (the same math, on the CPU)
    goes from loss 1.64e-2 to 2.75e-3, translation error 5.39e-2 to 2.24e-2 and rotation error
    1.97e-2 rad to 4.66e-3 rad, so the three assertions hold with a wide margin."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import multiview
    case, cam = cc.recipe(), cc.camera(0)
    sc = {k: v.to(DEV) for k, v in case["scene"].items()}
    rast = dgr.GaussianRasterizer(_settings(cam, case, False))
    args = dict(means3D=sc["means3D"], means2D=torch.zeros_like(sc["means3D"]), opacities=sc["opacities"],
                shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    with torch.no_grad():
        target = rast(**args)[0]

    def pose_error(view):
        Rt, R = cam.world_view_transform.double()[:3, :3], view.double()[:3, :3]
        angle = math.acos(max(-1.0, min(1.0, (float(torch.trace(R.T @ Rt)) - 1.0) / 2.0)))
        return float((torch.linalg.inv(view.double())[3, :3] - cam.camera_center.double()).norm()), angle

    delta = torch.tensor([0.01, -0.015, 0.008, 0.03, -0.02, 0.04], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([delta], lr=2e-3)
    K, hist = 20, []
    for k in range(K + 1):
        # pose refinement in three lines
        camera = tuple(t.float().to(DEV) for t in multiview.pose_camera(cam, delta))
        loss = (rast(camera=camera, **args)[0] - target).abs().mean()
        hist.append((float(loss.detach()),) + pose_error(camera[0].detach().cpu()))
        if k == K:
            break
        opt.zero_grad()
        loss.backward()
        opt.step()
    print(f"pose refinement: loss {hist[0][0]:.3e} -> {hist[-1][0]:.3e}, translation {hist[0][1]:.3e} -> "
          f"{hist[-1][1]:.3e}, rotation {hist[0][2]:.3e} -> {hist[-1][2]:.3e}")
    assert hist[-1][0] < hist[0][0] and hist[-1][1] < hist[0][1] and hist[-1][2] < hist[0][2], hist
