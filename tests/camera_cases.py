"""Scenes and float64 references shared by test_camera_grads.py (GPU) and test_camera_grads_cpu.py.

The recipe scene is small enough for tests/dense_ref.py (every (pixel, Gaussian) pair in float64) and
still takes every path of the camera-gradient kernel: Gaussians culled by the frustum, Gaussians of
more than 32 tiles (the records beyond a Gaussian's own mask), a ragged last workgroup
(549 = 2 * 256 + 37), SH colours with a view direction, and -- in the `spread` variant -- Gaussians
whose projection is clamped at 1.3 tan(fov/2).
"""
import functools

import torch

import dense_ref
import synthetic

P_RECIPE, W_RECIPE, H_RECIPE = 549, 160, 112
RECIPE_VIEWS = (0, 3)
BG = (0.1, 0.4, 0.7)


def cov3d_of(scales, rotations):
    """(P,6) upper triangle of R S^2 R^T, in the inputs' dtype."""
    R = dense_ref.quat_to_R(rotations)
    M = R @ torch.diag_embed(scales)
    S = M @ M.transpose(1, 2)
    return torch.stack([S[:, 0, 0], S[:, 0, 1], S[:, 0, 2], S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]], 1).contiguous()


@functools.lru_cache(maxsize=None)
def recipe(spread=1.0):
    """The recipe scene as a common.make_case dictionary (float32 tensors on the CPU); spread != 1
    multiplies the second half of the means once more (Gaussians leave the frustum sideways)."""
    sc = synthetic.make_scene(P_RECIPE, seed=7)
    half = P_RECIPE // 2
    m = sc["means3D"].clone()
    m[:half] *= 0.45
    m[half:] *= 2.2 * spread
    s = sc["scales"] * 4.0
    o = sc["opacities"].clone()
    s[:4] = 0.6
    m[:4] *= 0.3
    o[:4] = 0.3
    o = o.clamp(max=0.95)
    m[-3:] = torch.tensor([[9.0, 0.0, 0.0], [0.0, 0.0, 9.0], [5.0, -0.5, 0.1]])
    if spread != 1.0:
        # Spreading alone leaves no visible Gaussian clamped (dense_ref: none in any ring view at x4: the
        # Gaussians that leave the frustum sideways are too small to reach back into the image).  So the
        # variant also puts two wide Gaussians (scale 0.3) per recipe view just outside the clamp limit,
        # at view-space (1.45 tan(fov_x/2) z, 0, z) and (0, -1.45 tan(fov_y/2) z, z), z = 2: their
        # centres are clamped at 1.3 tan(fov/2), their 3-sigma extent still covers image tiles.
        for j, view in enumerate(RECIPE_VIEWS):
            cam = camera(view)
            z = 2.0
            pv = torch.tensor([[1.45 * cam.tanfovx * z, 0.0, z, 1.0], [0.0, -1.45 * cam.tanfovy * z, z, 1.0]])
            m[half + 2 * j:half + 2 * j + 2] = (pv @ cam.world_view_transform.inverse())[:, :3]
            s[half + 2 * j:half + 2 * j + 2] = 0.3
    scene = {"means3D": m.contiguous(), "scales": s.contiguous(), "rotations": sc["rotations"],
             "opacities": o.contiguous(), "shs": sc["shs"]}
    g = torch.Generator().manual_seed(11)
    gc, gi = synthetic.make_grads(H_RECIPE, W_RECIPE, seed=8)
    return dict(scene=scene, H=H_RECIPE, W=W_RECIPE, bg=torch.tensor(BG, dtype=torch.float32), sh_degree=3,
                grad_color=gc, grad_invdepth=gi, colors_precomp=torch.rand(P_RECIPE, 3, generator=g),
                cov3D_precomp=cov3d_of(s, sc["rotations"]))


def camera(view, W=W_RECIPE, H=H_RECIPE):
    return synthetic.Camera(W, H, view)


def dense_inputs(case, kind):
    """dense_ref's input dictionary in float64; kind 'sh' (SH colours, scales + rotations) or
    'colors_cov' (precomputed colours and covariances)."""
    sc = case["scene"]
    inp = {"means3D": sc["means3D"], "opacities": sc["opacities"]}
    if kind == "sh":
        inp.update(shs=sc["shs"], scales=sc["scales"], rotations=sc["rotations"])
    else:
        inp.update(colors_precomp=case["colors_precomp"], cov3D_precomp=case["cov3D_precomp"])
    return {k: v.double().clone() for k, v in inp.items()}


def clamped_visible(means3D, cam, radii):
    """Visible Gaussians whose view-space x/z or y/z lies outside 1.3 tan(fov/2) (forward.cu:81-86)."""
    m = means3D.double()
    t = torch.cat([m, torch.ones(len(m), 1, dtype=m.dtype)], 1) @ cam.world_view_transform.double()
    out = ((t[:, 0] / t[:, 2]).abs() > 1.3 * cam.tanfovx) | ((t[:, 1] / t[:, 2]).abs() > 1.3 * cam.tanfovy)
    return out & (radii > 0)


def dense_camera_grads(case, cam, kind, antialiasing, with_invdepth):
    """float64 autograd of dense_ref at `cam`: dL/dview, dL/dproj, dL/dcampos (three independent
    leaves) and dL/dmeans3D for the loss sum(color * grad_color) + sum(invdepth * grad_invdepth), the
    upstream gradients zeroed at the reference's tie pixels.  Returns the gradients with the tie mask
    (H,W), radii, alpha_max and the number of visible clamped Gaussians."""
    inp = dense_inputs(case, kind)
    inp["means3D"].requires_grad_(True)
    dcam = dense_ref.ring_cam(cam)
    leaves = [dcam[k].clone().requires_grad_(True) for k in ("view", "proj", "campos")]
    dcam.update(view=leaves[0], proj=leaves[1], campos=leaves[2])
    H, W = case["H"], case["W"]
    out = dense_ref.dense_render(inp, dcam, H, W, case["sh_degree"], case["bg"].double(), antialiasing=antialiasing,
                                 aa_quirk=True)
    keep = (~out["tie"]).reshape(1, H, W).double()
    gc = case["grad_color"].double() * keep
    gi = case["grad_invdepth"].double() * keep * (1.0 if with_invdepth else 0.0)
    g = torch.autograd.grad(dense_ref.loss_of(out, gc, gi), leaves + [inp["means3D"]], allow_unused=True)
    g = [torch.zeros_like(x) if y is None else y for x, y in zip(leaves + [inp["means3D"]], g)]
    return {"view": g[0], "proj": g[1], "campos": g[2], "means3D": g[3], "tie": out["tie"].reshape(H, W),
            "radii": out["radii"], "alpha_max": float(out["alpha_max"]),
            "clamped": int(clamped_visible(case["scene"]["means3D"], cam, out["radii"]).sum())}


_dense_cache = {}


def dense_camera_grads_cached(spread, view, kind, antialiasing, with_invdepth):
    key = (spread, view, kind, bool(antialiasing), bool(with_invdepth))
    if key not in _dense_cache:
        _dense_cache[key] = dense_camera_grads(recipe(spread), camera(view), kind, antialiasing, with_invdepth)
    return _dense_cache[key]


def translation_identity(g_view, g_proj, g_campos, g_means3D, cam):
    """Both sides of the identity (moving the camera centre by d = moving every mean by -d):
        dL/dcampos - R dL/dview[3,:3] - (R Pm[:3,:]) dL/dproj[3,:]  ==  -sum_i dL/dmeans3D[i]
    with R = view[:3,:3] and Pm = the camera's projection_matrix, and S = sum_i |dL/dmeans3D[i]|, the
    scale of the rounding of either side.  float64 tensors (3,)."""
    view = cam.world_view_transform.double()
    R, Pm = view[:3, :3], cam.projection_matrix.double()
    lhs = g_campos.double() - R @ g_view.double()[3, :3] - (R @ Pm[:3, :]) @ g_proj.double()[3, :]
    gm = g_means3D.double()
    return lhs, -gm.sum(0), gm.abs().sum(0)
