"""DataParallelTrainer(fused_tail=True) -- the views' L1 + D-SSIM loss as one fused_l1_ssim_loss call
and their densification statistics as one add_batch_stats launch -- against the default torch
tail from the same start: a 2,000-Gaussian synthetic scene, 64x80, 3 views, 3 steps without
densification.

Per-view losses agree within 2e-6 (the tolerance of the loss kernels, tests/test_photo_loss.py).
The statistics are checked as in tests/test_batch_stats.py, against add_view_stats on CPU copies
of the very gradients and radii the fused trainer fed to the kernel.  The parameters after the
steps differ by fp32 summation order in the loss gradient (which Adam's normalisation amplifies
where a gradient is nearly zero).  Measured on an MI355X, as max|a - b| / max|b| per parameter
group: xyz 7.7e-8, f_dc 9.5e-8, f_rest 3.2e-7, opacity 4.6e-6, scaling 7.1e-8, rotation 1.3e-6 (the
losses differed by at most 7.5e-9); the largest is PARAM_REL_MEASURED, asserted with a 4x margin.
A batch with an alpha-mask view takes the torch loss and reproduces its losses bit for bit.
"""
import numpy as np
import pytest
import torch

from test_batch_stats import check_against_view_stats

pytestmark = pytest.mark.gpu

P, H, W, VIEWS, ITERS = 2000, 64, 80, 3, 3
PARAM_REL_MEASURED = 4.65e-6  # opacity (see above)


def _setup(dev, fused_tail, alpha=False):
    import synthetic
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import multiview
    gt = synthetic.make_scene(P, seed=0)
    g = torch.Generator().manual_seed(5)
    raw = {"xyz": gt["means3D"] + 0.02 * torch.randn(P, 3, generator=g),
           "f_dc": gt["shs"][:, :1] + 0.3 * torch.randn(P, 1, 3, generator=g),
           "f_rest": gt["shs"][:, 1:].clone(),
           "opacity": torch.full((P, 1), -1.0),
           "scaling": torch.log(gt["scales"]) + 0.3 * torch.randn(P, 3, generator=g),
           "rotation": gt["rotations"] + 0.1 * torch.randn(P, 4, generator=g)}
    trainer = multiview.DataParallelTrainer({k: v.to(dev) for k, v in raw.items()}, lr={"xyz": 4.8e-4},
                                            fused_tail=fused_tail)
    gt_t = {k: v.to(dev) for k, v in gt.items()}
    views = []
    for v in range(VIEWS):
        c = synthetic.Camera(W, H, view=v)
        s = dgr.GaussianRasterizationSettings(
            H, W, c.tanfovx, c.tanfovy, torch.zeros(3, device=dev), 1.0, c.world_view_transform.to(dev),
            c.full_proj_transform.to(dev), 3, c.camera_center.to(dev), False, False, False)
        with torch.no_grad():
            target = dgr.GaussianRasterizer(s)(means3D=gt_t["means3D"], means2D=torch.zeros_like(gt_t["means3D"]),
                                               shs=gt_t["shs"], opacities=gt_t["opacities"], scales=gt_t["scales"],
                                               rotations=gt_t["rotations"])[0].clamp(0, 1)
        extras = {}
        if alpha and v == 1:
            extras["alpha_mask"] = (torch.rand((1, H, W), generator=g) > 0.3).float().to(dev)
        views.append((s, target, extras))
    return trainer, views


def _train(dev, fused_tail):
    """ITERS steps; (losses per step, parameters, statistics after step 1, what _track was fed)."""
    trainer, views = _setup(dev, fused_tail)
    fed, track = [], trainer._track

    def spy(grads, radii, track_stats):
        fed.append((grads.detach().clone().cpu(), radii.clone().cpu()))
        track(grads, radii, track_stats)
    trainer._track = spy
    losses, first = [], None
    for it in range(ITERS):
        losses.append([float(l) for l in trainer.step(views)])
        if it == 0:
            first = {k: trainer.stats[k].clone().cpu() for k in ("xyz_gradient_accum", "denom", "max_radii2D")}
    torch.cuda.synchronize()
    return trainer, losses, {k: p.detach().cpu().numpy() for k, p in trainer.params.items()}, first, fed


def test_fused_tail_matches_torch_tail():
    dev = torch.device("cuda", 0)
    ref, ref_losses, ref_params, ref_first, _ = _train(dev, False)
    fus, fus_losses, fus_params, fus_first, fed = _train(dev, True)
    assert fus.fused_tail and not ref.fused_tail and len(fed) == ITERS
    # losses
    d = np.abs(np.array(fus_losses) - np.array(ref_losses))
    print(f"per-view losses: max |fused - torch| = {d.max():.3e}")
    assert d.max() < 2e-6
    # statistics after the first step (same parameters, so the same radii): counts and radii exact
    assert torch.equal(fus_first["denom"], ref_first["denom"])
    assert torch.equal(fus_first["max_radii2D"], ref_first["max_radii2D"])
    assert float(ref_first["denom"].max()) > 0
    np.testing.assert_allclose(fus_first["xyz_gradient_accum"].numpy(), ref_first["xyz_gradient_accum"].numpy(),
                               rtol=1e-4, atol=1e-9)
    # ... and, over all steps, what add_view_stats makes of the kernel's own inputs
    zeros = {"accum": torch.zeros((P, 1)), "denom": torch.zeros((P, 1)), "max_radii2D": torch.zeros((P,)),
             "visible_count": torch.zeros((P,))}
    grads, radii = torch.cat([f[0] for f in fed]), torch.cat([f[1] for f in fed])
    check_against_view_stats(fus.stats, None, grads, radii, zeros)
    assert torch.equal(fus.visible_count.cpu(), (fed[-1][1] > 0).sum(dim=0).float())  # (zeroed every step)
    # parameters
    rel = {k: float(np.abs(fus_params[k] - ref_params[k]).max() / np.abs(ref_params[k]).max()) for k in ref_params}
    print("parameters after %d steps: max|fused - torch| / max|torch| = %s" % (ITERS, rel))
    assert max(rel.values()) <= 4 * PARAM_REL_MEASURED


def test_alpha_mask_batch_takes_the_torch_loss():
    dev = torch.device("cuda", 0)
    out = {}
    for fused in (False, True):
        trainer, views = _setup(dev, fused, alpha=True)
        trainer.zero_grad()
        losses = trainer.render_and_backward(views)
        torch.cuda.synchronize()
        out[fused] = (torch.stack(losses).cpu(), trainer.flat.clone().cpu(),
                      {k: trainer.stats[k].clone().cpu() for k in ("xyz_gradient_accum", "denom", "max_radii2D")})
    assert torch.equal(out[True][0], out[False][0])
    assert torch.equal(out[True][1], out[False][1])  # same loss graph: the same gradients and counts
    assert torch.equal(out[True][2]["denom"], out[False][2]["denom"])
    assert torch.equal(out[True][2]["max_radii2D"], out[False][2]["max_radii2D"])
    assert float(out[True][2]["denom"].max()) > 0


@pytest.mark.parametrize("batched", [True, False], ids=["batched", "per-view"])
def test_exposure_is_applied_before_the_fused_loss(batched):
    """Per-camera exposures (applied in torch, once, before the fused loss clamps): the losses and
    the exposure gradients of the two tails agree."""
    dev = torch.device("cuda", 0)
    g = torch.Generator().manual_seed(9)
    exposures = torch.eye(3, 4)[None].repeat(VIEWS, 1, 1) + 0.05 * torch.randn((VIEWS, 3, 4), generator=g)
    out = {}
    for fused in (False, True):
        trainer, views = _setup(dev, fused)
        trainer = type(trainer)({k: p.detach() for k, p in trainer.params.items()}, lr={"xyz": 4.8e-4},
                                fused_tail=fused, exposures=exposures, batched=batched)
        views = [(s, t, {"cam": j}) for j, (s, t, _) in enumerate(views)]
        trainer.zero_grad()
        losses = trainer.render_and_backward(views)
        torch.cuda.synchronize()
        out[fused] = (torch.stack(losses).cpu().numpy(), trainer.exposures.grad.clone().cpu().numpy())
    assert np.abs(out[True][0] - out[False][0]).max() < 2e-6
    a, b = out[True][1], out[False][1]
    assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-4 * np.abs(b).max()


def test_single_view_branch():
    """batched=False: one view at a time, the fused loss and the statistics kernel with V = 1."""
    dev = torch.device("cuda", 0)
    out = {}
    for fused in (False, True):
        trainer, views = _setup(dev, fused)
        trainer.batched = False
        trainer.zero_grad()
        losses = trainer.render_and_backward(views)
        torch.cuda.synchronize()
        out[fused] = (torch.stack(losses).cpu().numpy(), trainer.flat.clone().cpu().numpy(),
                      trainer.stats["denom"].clone().cpu())
    assert np.abs(out[True][0] - out[False][0]).max() < 2e-6
    a, b = out[True][1], out[False][1]
    assert np.abs(a - b).max() <= 1e-4 * np.abs(b).max() + 1e-9, np.abs(a - b).max()
    assert torch.equal(out[True][2], out[False][2])
