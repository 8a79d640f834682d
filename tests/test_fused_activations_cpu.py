"""fused_activations without a GPU: the surface exists, validates its arguments by name and has no
CPU path; DataParallelTrainer's flag is off by default and changes nothing then."""
import pytest
import torch


def _inputs(P=5):
    g = torch.Generator().manual_seed(0)
    return (torch.randn((P, 3), generator=g), torch.randn((P, 4), generator=g), torch.randn((P, 1), generator=g))


def test_exported():
    import diff_gaussian_rasterization as dgr
    assert "fused_activations" in dgr.__all__ and callable(dgr.fused_activations)


def test_cpu_tensors_raise():
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    s, r, o = _inputs()
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.activate_forward(s, r, o)
    with pytest.raises(RuntimeError, match="no CPU path"):
        dgr.fused_activations(s.requires_grad_(True), r, o)
    with pytest.raises(RuntimeError, match="no CPU path"):
        _C.activate_backward(s.detach(), r, o, s.detach(), r, o, torch.empty_like(s), torch.empty_like(r),
                             torch.empty_like(o))


@pytest.mark.parametrize("bad,name", [
    (lambda s, r, o: (s[:, :2].contiguous(), r, o), "scaling"),
    (lambda s, r, o: (s.reshape(-1), r, o), "scaling"),
    (lambda s, r, o: (s, r[:, :3].contiguous(), o), "rotation"),
    (lambda s, r, o: (s, r[:4], o), "rotation"),
    (lambda s, r, o: (s, r, torch.cat([o, o], dim=1)), "opacity"),
    (lambda s, r, o: (s, r, o[:3]), "opacity"),
    (lambda s, r, o: (s.double(), r, o), "scaling"),
    (lambda s, r, o: (s, r.double(), o), "rotation"),
    (lambda s, r, o: (s, r, o.double()), "opacity"),
    (lambda s, r, o: (torch.randn(3, 5).t(), r, o), "scaling"),
    (lambda s, r, o: (s, torch.randn(5, 8)[:, ::2], o), "rotation"),
    (lambda s, r, o: (s, r, torch.randn(5, 2)[:, :1]), "opacity"),
], ids=["scaling-cols", "scaling-1d", "rotation-cols", "rotation-rows", "opacity-cols", "opacity-rows",
        "scaling-f64", "rotation-f64", "opacity-f64", "scaling-strided", "rotation-strided", "opacity-strided"])
def test_bad_arguments_are_named(bad, name):
    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    args = bad(*_inputs())
    for fn in (_C.activate_forward, dgr.fused_activations):
        with pytest.raises(RuntimeError, match=name) as e:
            fn(*args)
        assert "no CPU path" not in str(e.value)  # the argument's own fault is reported, not the device


def test_backward_binding_names_bad_arguments():
    from diff_gaussian_rasterization import _C
    s, r, o = _inputs()
    ok = dict(scales=s, rotation=r, opacities=o, dL_dscales=s, dL_drotations=r, dL_dopacities=o,
              dL_dscaling=torch.empty_like(s), dL_drotation=torch.empty_like(r), dL_dopacity=torch.empty_like(o))
    for name, t in (("dL_drotation", torch.empty(5, 8)[:, ::2]), ("dL_dscales", s.double()),
                    ("dL_dopacity", torch.empty(4, 1)), ("opacities", torch.empty(5, 2))):
        with pytest.raises(RuntimeError, match=name):
            _C.activate_backward(**dict(ok, **{name: t}))
    with pytest.raises(RuntimeError, match="accumulate_mask"):
        _C.activate_backward(**ok, accumulate_mask=8)
    # a skipped group's arguments are not looked at
    with pytest.raises(RuntimeError, match="scales"):
        _C.activate_backward(**dict(ok, dL_drotations=None, rotation=None, dL_dopacity=None))


def _raw(P=6):
    g = torch.Generator().manual_seed(1)
    return {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g),
            "f_rest": torch.randn(P, 15, 3, generator=g), "opacity": torch.randn(P, 1, generator=g),
            "scaling": torch.randn(P, 3, generator=g), "rotation": torch.randn(P, 4, generator=g)}


def test_trainer_flag():
    from diff_gaussian_rasterization import multiview
    raw = _raw()
    default = multiview.DataParallelTrainer(raw)
    assert default.fused_activations is False
    act = default.activations()
    assert torch.equal(act["scales"], torch.exp(raw["scaling"]))
    assert torch.equal(act["opacities"], torch.sigmoid(raw["opacity"]))
    assert torch.equal(act["rotations"], torch.nn.functional.normalize(raw["rotation"]))
    assert act["means3D"] is default.params["xyz"] and act["dc"] is default.params["f_dc"]
    assert act["shs"] is default.params["f_rest"]
    fused = multiview.DataParallelTrainer(raw, fused_activations=True)  # constructing it needs no GPU
    assert fused.fused_activations is True
    with pytest.raises(RuntimeError, match="no CPU path"):
        fused.activations()
