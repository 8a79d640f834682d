"""multiview.add_batch_stats (densify_stats_kernel) against add_view_stats applied view by view to
CPU copies, with xyz_gradient_accum recomputed in float64.

denom, max_radii2D and visible_count must be exact (small integers and a running max).  accum
may differ from the float64 value by (3V + 1) 2^-24 relative: every term is positive, so per
view the norm's own rounding (two squares and their sum, halved by the square root, then the
root's) stays within 2 x 2^-24 of the term and the running sum adds 2^-24 of the partial sum;
the "+ 1" covers the float32 start value.  Gaussians no view sees keep their rows bit for bit.  The accumulators start non-zero and
are used both as the columns of one (P,2) buffer (the trainer) and as separate (P,1) tensors
(GaussianModel).
"""
import numpy as np
import pytest
import torch

from diff_gaussian_rasterization import multiview as mv


def _inputs(P, V, seed):
    g = torch.Generator().manual_seed(seed)
    grads = torch.randn((V, P, 3), generator=g) * 1e-3
    radii = torch.randint(-1, 40, (V, P), generator=g, dtype=torch.int32)
    radii[torch.rand((V, P), generator=g) < 0.4] = 0
    if P > 4:
        radii[:, 0:P:5] = 0                                   # visible in no view
        radii[:, 1:P:5] = torch.randint(1, 40, (V, len(range(1, P, 5))), generator=g, dtype=torch.int32)  # in every view
    start = {"accum": torch.rand((P, 1), generator=g), "denom": torch.randint(0, 9, (P, 1), generator=g).float(),
             "max_radii2D": torch.randint(0, 30, (P,), generator=g).float(),
             "visible_count": torch.randint(0, 3, (P,), generator=g).float()}
    return grads, radii, start


def _stats(start, columns, device):
    """The accumulators on `device`: columns of one (P,2) buffer, or tensors of their own."""
    P = start["accum"].shape[0]
    if columns:
        st = mv.densification_stats(P, device)
    else:
        st = {"xyz_gradient_accum": torch.zeros((P, 1), device=device), "denom": torch.zeros((P, 1), device=device),
              "max_radii2D": torch.zeros((P,), device=device)}
    st["xyz_gradient_accum"].copy_(start["accum"])
    st["denom"].copy_(start["denom"])
    st["max_radii2D"].copy_(start["max_radii2D"])
    return st


def check_against_view_stats(stats_gpu, count_gpu, grads, radii, start, columns=True):
    """Shared with the trainer test: the statistics equal add_view_stats over the views in order."""
    V, P = radii.shape
    ref = _stats(start, columns, "cpu")
    count = start["visible_count"].clone()
    accum64 = start["accum"].double().clone()
    for v in range(V):
        mv.add_view_stats(ref, grads[v], radii[v])
        vis = radii[v] > 0
        count += vis.float()
        accum64[vis] += torch.linalg.vector_norm(grads[v][vis, :2].double(), dim=-1, keepdim=True)
    assert torch.equal(stats_gpu["denom"].cpu(), ref["denom"])
    assert torch.equal(stats_gpu["max_radii2D"].cpu(), ref["max_radii2D"])
    if count_gpu is not None:
        assert torch.equal(count_gpu.cpu(), count)
    got = stats_gpu["xyz_gradient_accum"].cpu().double()
    rel = ((got - accum64).abs() / accum64.abs().clamp_min(1e-300)).max().item() if P else 0.0
    print(f"P={P} V={V}: accum max rel err {rel:.3e} (bound {(3 * V + 1) * 2.0 ** -24:.3e})")
    assert rel <= (3 * V + 1) * 2.0 ** -24
    unseen = (radii <= 0).all(dim=0)
    assert np.array_equal(got[unseen].numpy(), start["accum"].double()[unseen].numpy())
    return unseen


@pytest.mark.gpu
@pytest.mark.parametrize("columns", [True, False], ids=["P2-buffer", "P1-tensors"])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("P", [1, 1037])
def test_matches_view_stats(P, V, columns):
    grads, radii, start = _inputs(P, V, 10 * P + V)
    if P == 1:
        radii[:] = 3  # the one Gaussian is seen (the unseen case: test_unseen_single below)
    st = _stats(start, columns, "cuda")
    count = start["visible_count"].cuda()
    mv.add_batch_stats(st, grads.cuda(), radii.cuda(), count)
    unseen = check_against_view_stats(st, count, grads, radii, start, columns)
    if P > 4:
        assert unseen.any() and (radii > 0).all(dim=0).any()
    # without the optional count
    st2 = _stats(start, columns, "cuda")
    mv.add_batch_stats(st2, grads.cuda(), radii.cuda())
    for k in ("xyz_gradient_accum", "denom", "max_radii2D"):
        assert torch.equal(st2[k], st[k])


@pytest.mark.gpu
def test_unseen_single():
    grads, radii, start = _inputs(1, 3, 5)
    radii[:] = 0
    st = _stats(start, True, "cuda")
    count = start["visible_count"].cuda()
    before = st["_sums"].clone()
    mv.add_batch_stats(st, grads.cuda(), radii.cuda(), count)
    assert torch.equal(st["_sums"], before) and torch.equal(count.cpu(), start["visible_count"])
    assert torch.equal(st["max_radii2D"].cpu(), start["max_radii2D"])


@pytest.mark.gpu
def test_rejects_bad_input():
    st = mv.densification_stats(4, "cuda")
    g, r = torch.zeros((2, 4, 3), device="cuda"), torch.ones((2, 4), dtype=torch.int32, device="cuda")
    with pytest.raises(RuntimeError, match="GPU only"):
        mv.add_batch_stats(mv.densification_stats(4), g.cpu(), r.cpu())
    with pytest.raises(RuntimeError, match="radii"):
        mv.add_batch_stats(st, g, r.long())
    with pytest.raises(RuntimeError, match="radii"):
        mv.add_batch_stats(st, g, r[:1])
    with pytest.raises(RuntimeError, match="visible_count"):
        mv.add_batch_stats(st, g, r, torch.zeros(5, device="cuda"))


def test_capi_checks_arguments_without_a_device():
    import ctypes
    from diff_gaussian_rasterization import _C
    lib = _C.lib
    buf = (ctypes.c_float * 16)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gsr_densification_stats(0, 4, p, p, p, p, 1, p, 1, None, None) == 0
    assert lib.gsr_densification_stats(2, 0, None, None, None, None, 1, None, 1, None, None) == 0
    assert lib.gsr_densification_stats(-1, 4, p, p, p, p, 1, p, 1, None, None) == 1
    assert lib.gsr_densification_stats(1, 4, p, p, p, p, 0, p, 1, None, None) == 1
    assert lib.gsr_densification_stats(1, 4, p, None, p, p, 2, p, 2, None, None) == 1
    assert b"null" in lib.gsr_last_error()
