"""Camera pose gradients: what can be checked without a GPU.

* the new names are exported and the library has the two entry points;
* _C.backward_camera_views reports a wrong shape, dtype or stride of each camera tensor and of each
  gradient output by name, before it reports where a tensor lives; CPU tensors have no path;
* camera= / cameras= refuse deferred_backward() and grad_chunk_hook by name;
* multiview.pose_camera reproduces the base camera at delta = 0 and is differentiable;
* the translation identity test_camera_grads.py relies on holds for the float64 dense reference.
"""
import pytest
import torch

import camera_cases as cc
import synthetic

CAMS = ("viewmatrices", "projmatrices", "campos")
OUTS = ("dL_dviewmatrices", "dL_dprojmatrices", "dL_dcampos")


def _shape(name, V):
    return (V, 3) if name.endswith("campos") else (V, 4, 4)


def _call(V=2, P=5, **override):
    """backward_camera_views on CPU tensors of the right shapes, `override` replacing some."""
    from diff_gaussian_rasterization import _C
    t = {n: torch.zeros(_shape(n, V)) for n in CAMS}
    t.update({n: None for n in OUTS})
    t.update(override)
    empty = torch.Tensor([])
    buf = torch.zeros(16, dtype=torch.uint8)
    return _C.backward_camera_views(
        torch.zeros(P, 3), empty, torch.zeros(P, 1), torch.ones(P, 3), torch.ones(P, 4), 1.0, empty,
        t["viewmatrices"], t["projmatrices"], t["campos"], [0.5] * V, [0.5] * V, 32, 32, torch.zeros(P, 16, 3), 3,
        [buf] * V, [0] * V, [buf] * V, False, False, False, dL_dviewmatrices=t["dL_dviewmatrices"],
        dL_dprojmatrices=t["dL_dprojmatrices"], dL_dcampos=t["dL_dcampos"])


def test_names_exported():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C, multiview
    for name in ("rasterize_gaussians_camera", "rasterize_views_camera"):
        assert name in dgr.__all__ and callable(getattr(dgr, name))
    assert issubclass(dgr._RasterizeGaussiansCamera, torch.autograd.Function)
    assert issubclass(dgr._RasterizeViewsCamera, torch.autograd.Function)
    assert callable(_C.backward_camera_views) and callable(multiview.pose_camera)
    assert hasattr(_C.lib, "gsr_backward_camera_views") and hasattr(_C.lib, "gsr_camera_grad_workspace_size")
    import inspect
    assert "camera" in inspect.signature(dgr.GaussianRasterizer.forward).parameters
    assert "cameras" in inspect.signature(dgr.MultiViewRasterizer.forward).parameters


def test_workspace_size_monotone():
    from diff_gaussian_rasterization import _C
    sizes = [[_C.camera_grad_workspace_size(V, P) for P in (0, 1, 256, 257, 549, 5000, 1 << 20)] for V in (1, 2, 3, 16)]
    for row in sizes:
        assert all(a <= b for a, b in zip(row, row[1:])) and row[0] > 0 and row[-1] > row[1]
    for a, b in zip(sizes, sizes[1:]):
        assert all(x <= y for x, y in zip(a, b)) and a[-1] < b[-1]


def test_cpu_tensors_have_no_path():
    with pytest.raises(RuntimeError, match="no CPU path"):
        _call()


@pytest.mark.parametrize("name", CAMS + OUTS)
def test_bad_argument_reported_by_name(name):
    V = 2
    good = _shape(name, V)
    with pytest.raises(RuntimeError, match=rf"^{name} must have shape"):
        _call(V, **{name: torch.zeros(good[:-1] + (good[-1] + 1,))})
    with pytest.raises(RuntimeError, match=rf"^{name} must be float32"):
        _call(V, **{name: torch.zeros(good, dtype=torch.float64)})
    strided = torch.zeros(good[:-1] + (2 * good[-1],))[..., ::2]
    assert strided.shape == good and not strided.is_contiguous()
    with pytest.raises(RuntimeError, match=rf"^{name} must be contiguous"):
        _call(V, **{name: strided})
    if name == "viewmatrices":
        with pytest.raises(RuntimeError, match=r"^viewmatrices must have shape \(views, 4, 4\)"):
            _call(V, viewmatrices=torch.zeros(4, 4))
        with pytest.raises(RuntimeError, match="1 to 16 views"):
            _call(17)


def _cpu_rasterizer_args():
    import diff_gaussian_rasterization as dgr
    cam = synthetic.Camera(32, 32, 0)
    s = dgr.GaussianRasterizationSettings(32, 32, cam.tanfovx, cam.tanfovy, torch.zeros(3), 1.0,
                                          cam.world_view_transform, cam.full_proj_transform, 3, cam.camera_center,
                                          False, False, False)
    P = 4
    kw = dict(means3D=torch.zeros(P, 3), means2D=torch.zeros(P, 3), opacities=torch.ones(P, 1),
              shs=torch.zeros(P, 16, 3), scales=torch.ones(P, 3), rotations=torch.ones(P, 4))
    triple = (cam.world_view_transform.clone().requires_grad_(True), cam.full_proj_transform.clone(),
              cam.camera_center.clone())
    return dgr, s, kw, triple


def test_camera_refuses_deferred_backward_and_chunk_hook():
    dgr, s, kw, triple = _cpu_rasterizer_args()
    with dgr.deferred_backward():
        with pytest.raises(RuntimeError, match=r"camera= cannot be combined with deferred_backward\(\)"):
            dgr.GaussianRasterizer(s)(camera=triple, **kw)
    with dgr.grad_chunk_hook(2, lambda *a: None, lambda: None):
        with pytest.raises(RuntimeError, match="camera= cannot be combined with grad_chunk_hook"):
            dgr.GaussianRasterizer(s)(camera=triple, **kw)
    kw["means2D"] = torch.zeros(2, 4, 3)
    stacked = tuple(torch.stack([t, t]) for t in triple)
    with dgr.deferred_backward():
        with pytest.raises(RuntimeError, match=r"cameras= cannot be combined with deferred_backward\(\)"):
            dgr.MultiViewRasterizer([s, s])(cameras=stacked, **kw)
    with dgr.grad_chunk_hook(2, lambda *a: None, lambda: None):
        with pytest.raises(RuntimeError, match="cameras= cannot be combined with grad_chunk_hook"):
            dgr.MultiViewRasterizer([s, s])(cameras=[triple, triple], **kw)


def test_camera_triple_checked_by_name():
    dgr, s, kw, triple = _cpu_rasterizer_args()
    with pytest.raises(RuntimeError, match="camera=: campos must be a float32 tensor of shape"):
        dgr.GaussianRasterizer(s)(camera=(triple[0], triple[1], torch.zeros(4)), **kw)
    with pytest.raises(RuntimeError, match="camera=: viewmatrix must be a float32 tensor of shape"):
        dgr.GaussianRasterizer(s)(camera=(triple[0].double(), triple[1], triple[2]), **kw)
    kw["means2D"] = torch.zeros(2, 4, 3)
    with pytest.raises(RuntimeError, match="cameras=: 2 views, got 1 cameras"):
        dgr.MultiViewRasterizer([s, s])(cameras=[triple], **kw)


@pytest.mark.parametrize("view", [0, 3, 5])
def test_pose_camera_identity_at_zero(view):
    from diff_gaussian_rasterization import multiview
    cam = synthetic.Camera(160, 112, view)
    v, p, c = multiview.pose_camera(cam, torch.zeros(6))
    assert v.dtype == torch.float32
    assert torch.allclose(v, cam.world_view_transform, rtol=0, atol=1e-6)
    assert torch.allclose(p, cam.full_proj_transform, rtol=0, atol=1e-6)
    assert torch.allclose(c, cam.camera_center, rtol=0, atol=1e-6)


def test_pose_camera_moves_the_camera_frame():
    """p_view' = R(w) p_view + t: a pure translation shifts every view-space point by t, a rotation
    about z by +90 degrees takes the view-space x axis to y."""
    import math
    from diff_gaussian_rasterization import multiview
    cam = synthetic.Camera(160, 112, 2)
    base = cam.world_view_transform.double()
    pts = torch.cat([torch.randn(5, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(3)),
                     torch.ones(5, 1, dtype=torch.float64)], 1)
    t = torch.tensor([0.0, 0.0, 0.0, 0.1, -0.2, 0.3], dtype=torch.float64)
    v, _, c = multiview.pose_camera(cam, t)
    assert torch.allclose((pts @ v)[:, :3], (pts @ base)[:, :3] + t[3:], atol=1e-12)
    assert torch.allclose((torch.cat([c, torch.ones(1, dtype=c.dtype)]) @ v)[:3], torch.zeros(3, dtype=c.dtype),
                          atol=1e-12), "campos is the point the view maps to the origin"
    r = torch.tensor([0.0, 0.0, math.pi / 2, 0.0, 0.0, 0.0], dtype=torch.float64)
    v, _, _ = multiview.pose_camera(cam, r)
    pv, pb = (pts @ v)[:, :3], (pts @ base)[:, :3]
    assert torch.allclose(pv[:, 1], pb[:, 0], atol=1e-12) and torch.allclose(pv[:, 0], -pb[:, 1], atol=1e-12)


def test_pose_camera_gradcheck():
    from diff_gaussian_rasterization import multiview
    cam = synthetic.Camera(160, 112, 3)
    for d in (torch.zeros(6, dtype=torch.float64), torch.tensor([0.02, -0.3, 0.1, 0.5, -0.1, 0.2], dtype=torch.float64)):
        d = d.clone().requires_grad_(True)
        assert torch.autograd.gradcheck(lambda x: multiview.pose_camera(cam, x), (d,), eps=1e-6, atol=1e-7)
    with pytest.raises(RuntimeError, match=r"delta must have shape \(6,\)"):
        multiview.pose_camera(cam, torch.zeros(7))


@pytest.mark.parametrize("spread,kind,antialiasing", [(1.0, "sh", False), (1.0, "colors_cov", True), (4.0, "sh", True)])
def test_translation_identity_float64(spread, kind, antialiasing):
    """dL/dcampos - R dL/dview[3,:3] - (R Pm[:3,:]) dL/dproj[3,:] == -sum_i dL/dmeans3D[i] for the
    dense float64 reference, view, proj and campos being three independent leaves (measured: at most
    1e-8 of S = sum_i |dL/dmeans3D[i]|; the issue's figure is 5e-8).  The spread variant asserts its
    clamped Gaussians, which dense_ref differentiates exactly (its clamp has zero slope)."""
    for view in cc.RECIPE_VIEWS:
        r = cc.dense_camera_grads_cached(spread, view, kind, antialiasing, True)
        n_vis = int((r["radii"] > 0).sum())
        if spread == 1.0:
            assert 395 <= n_vis <= 425 and r["clamped"] == 0 and int(r["tie"].sum()) <= 1 and r["alpha_max"] < 0.99
        else:
            assert r["clamped"] >= 1 and n_vis < cc.P_RECIPE
        assert r["view"][:, 3].abs().max() == 0 and r["proj"][:, 2].abs().max() == 0
        if kind == "colors_cov":
            assert r["campos"].abs().max() == 0
        lhs, rhs, S = cc.translation_identity(r["view"], r["proj"], r["campos"], r["means3D"], cc.camera(view))
        assert float(((lhs - rhs).abs() / S).max()) < 5e-8
