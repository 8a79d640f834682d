"""fused_activations -- exp(scaling), normalize(rotation), sigmoid(opacity) and their backward as one
HIP launch each (csrc/activations.hip) -- against torch's own chain.

Values: the reference is torch's chain (exp, sigmoid, F.normalize, autograd) on the CPU in float64,
fed the same float32 inputs.  Errors are in units that stay meaningful where an ulp of the result
does not: one fp32 ulp of the reference value for scales and dL/dscaling; 2^-23 absolute for
rotations and opacities; 2^-23 |g|_2 / max(|q|_2, 1e-12) for dL/drotation; 2^-23 |g| / 4 for
dL/dopacity.  The bound, per output, is  fused <= 2 * torch_fp32 + 1  units, torch_fp32 being the
error of torch's fp32 chain on the GPU on the same inputs, measured in the same test: both sides
evaluate the same formulas in fp32 with a different sequence of roundings (a reciprocal in place
of a division, another exp), where a wrong formula is off by hundreds of units or more.  Measured
on an MI355X at P = 200,003 (fused / torch fp32 on the GPU, in units): scales 0.84 / 0.84, rotations
1.14 / 1.31, opacities 0.74 / 0.74, dL/dscaling 1.80 / 1.80, dL/drotation 2.47 / 2.73, dL/dopacity
2.97 / 2.97; every figure is printed by the test.

Trainer: DataParallelTrainer(fused_activations=True) against the default trainer from the same
start, the scene and steps of tests/test_fused_tail_train.py.  PARAM_REL_MEASURED is set from the
measurement on an MI355X recorded below.
"""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import common

pytestmark = pytest.mark.gpu

GROUPS = ("scaling", "rotation", "opacity")
OUTPUTS = ("scales", "rotations", "opacities", "dL/dscaling", "dL/drotation", "dL/dopacity")
U = 2.0 ** -23
EDGE_QUATS = [[0.0] * 4, [1e-20] * 4, [1e-13, 0.0, 0.0, 0.0], [3e-12, 4e-12, 0.0, 0.0]]
EDGE_ROTATIONS = [[0.0] * 4, [1e-8] * 4, [0.1, 0.0, 0.0, 0.0], [0.6, 0.8, 0.0, 0.0]]


@functools.lru_cache(maxsize=None)
def _case(P, seed=0):
    """Seeded float32 inputs and incoming gradients (CPU), with the float64 reference and the
    error units of every output.  Computed once per P and shared; never modified."""
    g = torch.Generator().manual_seed(seed + P)
    x = {"scaling": 1.5 * torch.randn((P, 3), generator=g) - 4.0,
         "rotation": torch.randn((P, 4), generator=g) * torch.exp(2.0 * torch.randn((P, 1), generator=g)),
         "opacity": 4.0 * torch.randn((P, 1), generator=g)}
    gr = {"scaling": torch.randn((P, 3), generator=g), "rotation": torch.randn((P, 4), generator=g),
          "opacity": torch.randn((P, 1), generator=g)}
    if P >= 4:
        x["scaling"][0] = torch.tensor([-30.0, 0.0, 80.0])
        x["rotation"][:4] = torch.tensor(EDGE_QUATS)
        x["opacity"][:4, 0] = torch.tensor([-100.0, 100.0, -20.0, 20.0])
    x64 = {k: v.double().requires_grad_(True) for k, v in x.items()}
    out = (torch.exp(x64["scaling"]), F.normalize(x64["rotation"]), torch.sigmoid(x64["opacity"]))
    torch.autograd.backward(out, [gr[k].double() for k in GROUPS])
    ref = [o.detach().numpy() for o in out] + [x64[k].grad.numpy() for k in GROUPS]

    def ulp(v):
        return np.spacing(np.abs(v).astype(np.float32)).astype(np.float64)
    qn = np.maximum(np.linalg.norm(x["rotation"].double().numpy(), axis=1, keepdims=True), 1e-12)
    gn = np.linalg.norm(gr["rotation"].double().numpy(), axis=1, keepdims=True)
    units = [ulp(ref[0]), U, U, ulp(ref[3]), U * gn / qn * np.ones((1, 4)), U * np.abs(gr["opacity"].double().numpy()) / 4]
    return x, gr, dict(zip(OUTPUTS, ref)), dict(zip(OUTPUTS, units))


def _run(fn, x, gr, dev):
    """The six outputs of a (scaling, rotation, opacity) -> (scales, rotations, opacities) chain on
    the GPU, as float64 numpy arrays."""
    leaves = [x[k].to(dev).requires_grad_(True) for k in GROUPS]
    out = fn(*leaves)
    torch.autograd.backward(out, [gr[k].to(dev) for k in GROUPS])
    return dict(zip(OUTPUTS, [t.detach().cpu().double().numpy() for t in list(out) + [l.grad for l in leaves]]))


def _torch_chain(scaling, rotation, opacity):
    return torch.exp(scaling), F.normalize(rotation), torch.sigmoid(opacity)


def _errors(got, ref, units):
    return {k: float((np.abs(got[k] - ref[k]) / units[k]).max()) for k in OUTPUTS}


@pytest.mark.parametrize("P", [1, 63, 64, 65, 255, 256, 257, 1001, 200003])
def test_values_against_float64_reference(P):
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda", 0)
    x, gr, ref, units = _case(P)
    fused = _run(dgr.fused_activations, x, gr, dev)
    chain = _run(_torch_chain, x, gr, dev)
    for k in OUTPUTS:
        assert fused[k].shape == ref[k].shape
        with np.errstate(over="ignore"):
            finite = np.isfinite(ref[k].astype(np.float32))
        assert np.array_equal(np.isfinite(fused[k]), finite), k
        assert finite.all(), k  # (inf outputs are out of scope: the inputs stay below them)
    ef, et = _errors(fused, ref, units), _errors(chain, ref, units)
    for k in OUTPUTS:
        print(f"P={P} {k}: fused {ef[k]:.3f} units, torch fp32 on the GPU {et[k]:.3f} units")
    for k in OUTPUTS:
        assert ef[k] <= 2.0 * et[k] + 1.0, (k, ef[k], et[k])
    if P >= 4:  # the edge rows: both sides of eps, and the 3-4-5 row
        assert np.abs(fused["rotations"][:4] - np.array(EDGE_ROTATIONS)).max() <= 4 * U
        g3 = gr["rotation"][:3].double().numpy()
        assert np.abs(fused["dL/drotation"][:3] - g3 / 1e-12).max() <= 1e-6 * np.abs(g3 / 1e-12).max()
        assert fused["opacities"][0, 0] == 0.0 and fused["opacities"][1, 0] == 1.0


def _flat_leaves(P, dev, seed, gaps=(1, 1)):
    """Raw leaves whose .grad are views of one flat buffer in DataParallelTrainer._install's order
    (xyz, f_dc, f_rest, opacity, scaling, rotation, then the visibility counts), pre-filled with
    random values, with gaps[0] sentinel floats between the opacity and the scaling view and
    gaps[1] between the scaling and the rotation view; everything outside the three views is a
    sentinel too.  Returns (flat, {group: (offset, size)}, {group: leaf}, incoming gradients)."""
    x, gr, _, _ = _case(P)
    g = torch.Generator().manual_seed(seed)
    sizes = [("xyz", 3 * P), ("f_dc", 3 * P), ("f_rest", 45 * P), ("opacity", P), ("gap0", gaps[0]),
             ("scaling", 3 * P), ("gap1", gaps[1]), ("rotation", 4 * P), ("visible_count", P)]
    flat = torch.randn((sum(n for _, n in sizes),), generator=g).to(dev)
    views, off = {}, 0
    for k, n in sizes:
        views[k] = (off, n)
        off += n
    leaves = {}
    for k in GROUPS:
        t = x[k].to(dev).requires_grad_(True)
        o, n = views[k]
        t.grad = flat[o:o + n].view_as(t)
        leaves[k] = t
    return flat, views, leaves, gr


@pytest.mark.parametrize("gaps", [(1, 1), (2, 3)], ids=["rotation-grad-unaligned", "rotation-grad-aligned"])
def test_in_place_accumulation_is_autograds(monkeypatch, gaps):
    """Run A (inside accumulate_grads_in_place: the kernel adds into .grad and the function returns
    None) and run B (outside: autograd adds the returned gradients) leave bit-identical .grad views,
    and nothing else in the flat buffer changes.  With P = 1001 the rotation view of the trainer's
    layout starts at float offset 55 * 1001 (+ the gaps): with gaps (1, 1) it is not 16-byte
    aligned and the kernel takes its dword path, with (2, 3) it is and the 16-byte path adds."""
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda", 0)
    P = 1001
    masks = []
    real = _C.activate_backward

    def spy(*a, **kw):
        masks.append(kw.get("accumulate_mask", a[9] if len(a) > 9 else 0))
        return real(*a, **kw)
    monkeypatch.setattr(_C, "activate_backward", spy)
    res = {}
    for run in ("A", "B"):
        flat, views, leaves, gr = _flat_leaves(P, dev, seed=11, gaps=gaps)
        assert (views["rotation"][0] % 4 != 0) == (gaps == (1, 1))
        assert (leaves["rotation"].grad.data_ptr() % 16 != 0) == (gaps == (1, 1))
        before = flat.clone()
        masks.clear()
        if run == "A":
            with dgr.accumulate_grads_in_place():
                out = dgr.fused_activations(*[leaves[k] for k in GROUPS])
        else:
            out = dgr.fused_activations(*[leaves[k] for k in GROUPS])
        torch.autograd.backward(out, [gr[k].to(dev) for k in GROUPS])
        torch.cuda.synchronize()
        assert masks == [7 if run == "A" else 0]  # A: all three added in the kernel, None returned
        touched = torch.zeros_like(flat, dtype=torch.bool)
        for k in GROUPS:
            o, n = views[k]
            assert leaves[k].grad.data_ptr() == flat[o:].data_ptr()  # still the view of the flat buffer
            touched[o:o + n] = True
        assert int((~touched).sum()) == 52 * P + sum(gaps)
        assert torch.equal(flat[~touched], before[~touched])  # every sentinel float unchanged
        assert bool((flat[touched] != before[touched]).float().mean() > 0.9)
        res[run] = flat.clone()
    assert torch.equal(res["A"], res["B"])


def test_partial_use(monkeypatch):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda", 0)
    calls = []
    real = _C.activate_backward

    def spy(*a, **kw):
        calls.append(a)
        return real(*a, **kw)
    monkeypatch.setattr(_C, "activate_backward", spy)
    x, gr, _, _ = _case(257)
    # only scales enters the loss: the other two raw .grad stay untouched
    flat, views, leaves, _ = _flat_leaves(1001, dev, seed=3)
    before = flat.clone()
    with dgr.accumulate_grads_in_place():
        scales, _, _ = dgr.fused_activations(*[leaves[k] for k in GROUPS])
    scales.backward(torch.ones_like(scales))
    torch.cuda.synchronize()
    o, n = views["scaling"]
    assert torch.equal(flat[:o], before[:o]) and torch.equal(flat[o + n:], before[o + n:])
    assert torch.equal(flat[o:o + n].view(-1, 3), before[o:o + n].view(-1, 3) + scales.detach())
    assert len(calls) == 1 and calls[0][4] is None and calls[0][5] is None  # rotation, opacity skipped
    # one input without requires_grad: no gradient for it, the others as the reference
    calls.clear()
    leaves = [x[k].to(dev).requires_grad_(k != "rotation") for k in GROUPS]
    out = dgr.fused_activations(*leaves)
    torch.autograd.backward(out, [gr[k].to(dev) for k in GROUPS])
    assert leaves[1].grad is None and len(calls) == 1 and calls[0][4] is None and calls[0][7] is None
    full = _run(dgr.fused_activations, x, gr, dev)  # the other two groups: the bits of a full backward
    for j, k in ((0, "dL/dscaling"), (2, "dL/dopacity")):
        assert np.array_equal(leaves[j].grad.cpu().double().numpy(), full[k]), k
    # no_grad, and inputs that need no gradient: the forward alone
    calls.clear()
    with torch.no_grad():
        out = dgr.fused_activations(*leaves)
    assert all(not t.requires_grad for t in out)
    out = dgr.fused_activations(*[l.detach() for l in leaves])
    assert all(not t.requires_grad and t.grad_fn is None for t in out)
    assert np.array_equal(out[1].cpu().double().numpy(), full["rotations"])
    assert calls == []
    # P = 0: empty tensors of the right shapes, no launch in either direction
    launches = []
    monkeypatch.setattr(_C.lib, "gsr_activate_forward", lambda *a: launches.append(a) or 0)
    monkeypatch.setattr(_C.lib, "gsr_activate_backward", lambda *a: launches.append(a) or 0)
    for op_shape in ((0, 1), (0,)):
        e = [torch.empty(s, device=dev, requires_grad=True) for s in ((0, 3), (0, 4), op_shape)]
        out = dgr.fused_activations(*e)
        assert [tuple(t.shape) for t in out] == [(0, 3), (0, 4), op_shape]
        assert all(t.is_contiguous() and t.dtype == torch.float32 and t.device == dev for t in out)
        sum(t.sum() for t in out).backward()
    assert launches == []


def test_opacity_as_a_vector():
    """opacity (P,) instead of (P,1): outputs and gradients keep the input's shape."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda", 0)
    x, gr, ref, units = _case(65)
    leaves = [x["scaling"].to(dev).requires_grad_(True), x["rotation"].to(dev).requires_grad_(True),
              x["opacity"][:, 0].contiguous().to(dev).requires_grad_(True)]
    out = dgr.fused_activations(*leaves)
    assert tuple(out[2].shape) == (65,)
    torch.autograd.backward(out, [gr["scaling"].to(dev), gr["rotation"].to(dev), gr["opacity"][:, 0].to(dev)])
    assert tuple(leaves[2].grad.shape) == (65,)
    two = _run(dgr.fused_activations, x, gr, dev)
    assert np.array_equal(out[2].detach().cpu().double().numpy(), two["opacities"][:, 0])
    assert np.array_equal(leaves[2].grad.cpu().double().numpy(), two["dL/dopacity"][:, 0])


def test_reproducible():
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda", 0)
    x, gr, _, _ = _case(200003)
    a, b = _run(dgr.fused_activations, x, gr, dev), _run(dgr.fused_activations, x, gr, dev)
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k


def test_through_the_rasterizer():
    """The fused outputs feeding GaussianRasterizer: the raw gradients against the torch chain's
    feeding the same rasterizer (the plumbing, not the arithmetic)."""
    import diff_gaussian_rasterization as dgr
    dev = torch.device("cuda", 0)
    case = common.make_case(P=1000, H=64, W=64)
    cam, sc = case["cam"], case["scene"]
    s = dgr.GaussianRasterizationSettings(64, 64, cam.tanfovx, cam.tanfovy, case["bg"].to(dev), 1.0,
                                          cam.world_view_transform.to(dev), cam.full_proj_transform.to(dev), 3,
                                          cam.camera_center.to(dev), False, False, False)
    op = sc["opacities"].clamp(1e-4, 1 - 1e-4)
    raw0 = {"scaling": torch.log(sc["scales"]), "rotation": 1.7 * sc["rotations"], "opacity": torch.log(op / (1 - op))}
    weight = torch.rand((3, 64, 64), generator=torch.Generator().manual_seed(2)).to(dev)
    grads = {}
    for name, fn in (("torch", _torch_chain), ("fused", dgr.fused_activations)):
        raw = {k: v.clone().to(dev).requires_grad_(True) for k, v in raw0.items()}
        means3D, shs = sc["means3D"].to(dev), sc["shs"].to(dev)
        scales, rotations, opacities = fn(raw["scaling"], raw["rotation"], raw["opacity"])
        img, radii, _ = dgr.GaussianRasterizer(s)(means3D=means3D, means2D=torch.zeros_like(means3D), shs=shs,
                                                  opacities=opacities, scales=scales, rotations=rotations)
        (img * weight).sum().backward()
        assert int((radii > 0).sum()) > 100
        grads[name] = {k: raw[k].grad.cpu().numpy() for k in GROUPS}
    for k in GROUPS:
        assert np.abs(grads["torch"][k]).max() > 0
        ok, rel = common.allclose_rel(grads["fused"][k], grads["torch"][k])
        assert ok, (k, rel)


# ---- the trainer -------------------------------------------------------------------------------
TP, TH, TW, VIEWS, ITERS = 2000, 64, 80, 3, 3  # the scene and steps of tests/test_fused_tail_train.py
PARAM_REL_MEASURED = 4.74e-6  # opacity, per view (see test_trainer's docstring)


def _trainer(dev, **kw):
    import synthetic
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import multiview
    gt = synthetic.make_scene(TP, seed=0)
    g = torch.Generator().manual_seed(5)
    raw = {"xyz": gt["means3D"] + 0.02 * torch.randn(TP, 3, generator=g),
           "f_dc": gt["shs"][:, :1] + 0.3 * torch.randn(TP, 1, 3, generator=g),
           "f_rest": gt["shs"][:, 1:].clone(),
           "opacity": torch.full((TP, 1), -1.0),
           "scaling": torch.log(gt["scales"]) + 0.3 * torch.randn(TP, 3, generator=g),
           "rotation": gt["rotations"] + 0.1 * torch.randn(TP, 4, generator=g)}
    trainer = multiview.DataParallelTrainer({k: v.to(dev) for k, v in raw.items()}, lr={"xyz": 4.8e-4}, **kw)
    gt_t = {k: v.to(dev) for k, v in gt.items()}
    views = []
    for v in range(VIEWS):
        c = synthetic.Camera(TW, TH, view=v)
        s = dgr.GaussianRasterizationSettings(
            TH, TW, c.tanfovx, c.tanfovy, torch.zeros(3, device=dev), 1.0, c.world_view_transform.to(dev),
            c.full_proj_transform.to(dev), 3, c.camera_center.to(dev), False, False, False)
        with torch.no_grad():
            target = dgr.GaussianRasterizer(s)(means3D=gt_t["means3D"], means2D=torch.zeros_like(gt_t["means3D"]),
                                               shs=gt_t["shs"], opacities=gt_t["opacities"], scales=gt_t["scales"],
                                               rotations=gt_t["rotations"])[0].clamp(0, 1)
        views.append((s, target, {}))
    return trainer, views


@functools.lru_cache(maxsize=None)
def _trained(batched, fused_tail, fused_activations):
    """(first step's losses, parameters after ITERS steps, visibility counts and denom after the
    first step's render_and_backward) of a trainer; computed once per configuration and shared."""
    dev = torch.device("cuda", 0)
    trainer, views = _trainer(dev, batched=batched, fused_tail=fused_tail, fused_activations=fused_activations)
    assert trainer.fused_activations == fused_activations
    losses, counts = [], None
    for it in range(ITERS):
        losses.append([float(l) for l in trainer.step(views)])
        if it == 0:  # (the optimizer step leaves both as render_and_backward left them)
            counts = (trainer.visible_count.clone().cpu(), trainer.stats["denom"].clone().cpu())
    torch.cuda.synchronize()
    return losses[0], {k: p.detach().cpu().numpy() for k, p in trainer.params.items()}, counts


@pytest.mark.parametrize("batched,fused_tail", [(True, False), (False, False), (True, True)],
                         ids=["batched", "per-view", "batched-fused-tail"])
def test_trainer(batched, fused_tail):
    """DataParallelTrainer(fused_activations=True) against the same trainer with the flag off: the
    first step's losses within 2e-6 (the loss kernels' tolerance, tests/test_fused_tail_train.py),
    the visibility counts and denom of that step equal, the parameters after ITERS steps within 4x
    PARAM_REL_MEASURED as max|a - b| / max|b| per group.  Measured on an MI355X (the losses of the
    first step were bit-equal in all three):
      batched:            xyz 7.7e-8, f_dc 4.8e-8, f_rest 6.6e-8, opacity 4.55e-6, scaling 7.1e-8, rotation 1.72e-6
      per view:           xyz 7.7e-8, f_dc 4.8e-8, f_rest 6.6e-8, opacity 4.74e-6, scaling 7.1e-8, rotation 1.82e-6
      batched, fused tail: xyz 7.7e-8, f_dc 4.8e-8, f_rest 1.8e-7, opacity 3.6e-7, scaling 7.1e-8, rotation 2.07e-6
    The largest, 4.74e-6, is PARAM_REL_MEASURED -- the size of the 4.65e-6 that
    tests/test_fused_tail_train.py records for the fused tail on this scene: a last-bit difference in
    an activation's gradient, amplified by Adam's normalisation where a gradient is nearly zero."""
    ref_loss, ref_params, ref_counts = _trained(batched, fused_tail, False)
    fus_loss, fus_params, fus_counts = _trained(batched, fused_tail, True)
    d = np.abs(np.array(fus_loss) - np.array(ref_loss)).max()
    print(f"first step's per-view losses: max |fused - torch| = {d:.3e}")
    assert d < 2e-6
    assert torch.equal(fus_counts[0], ref_counts[0]) and torch.equal(fus_counts[1], ref_counts[1])
    assert float(ref_counts[0].max()) > 0 and float(ref_counts[1].max()) > 0
    rel = {k: float(np.abs(fus_params[k] - ref_params[k]).max() / np.abs(ref_params[k]).max()) for k in ref_params}
    print("parameters after %d steps: max|fused - torch| / max|torch| = %s" % (ITERS, rel))
    assert max(rel.values()) <= 4 * PARAM_REL_MEASURED
