"""multiview.fused_densify_and_prune (gsr_densify_plan + gsr_densify_apply, csrc/densify.hip) against
the reference's own step-by-step sequence on CPU tensors (_ref_densify of tests/test_multiview.py),
fed the very samples the fused call drew.

Decisions compare a float with a threshold, so the inputs are moved off the thresholds first: g,
the largest scale, sigmoid(opacity) and a child's largest scale are multiplied by 1.01 wherever they
lie within 1e-3 (relative, float64) of a threshold they are compared with, and the tests assert
that margin.  No row is left out of any comparison.  Everything that is copied (kept rows, clones, a
child's rotation / f_dc / f_rest / opacity, every moment including the zeros) must be bit-identical.
What is computed is compared with its float64 evaluation from the same fp32 inputs:
  a child's scaling  within 2^-21 max(1, |ref64|): expf 1 ulp, the division 1/2 ulp and logf 1 ulp are
                     about 1.5 x 2^-23 absolute plus 2^-23 relative, times ~2.5;
  a child's xyz      per component within 2^-19 (|xyz_i| + sum_k |exp(s_k) z_k|): about 14 roundings of
                     2^-24 through the quaternion's normalisation, the entries of R, the scale and
                     the three-term sum, times ~2.
The CPU reference must meet the same two bounds, so they are no looser than its own error.
"""
import ctypes

import pytest
import torch

from test_multiview import _ref_densify

NAMES = ("xyz", "f_dc", "f_rest", "opacity", "scaling", "rotation")
PD = 0.01
MARGIN = 1e-3


# ---- inputs off the thresholds -------------------------------------------------------------------
def _thresholds(extent, max_screen_size, N):
    """(thresholds the largest scale is compared with, the world-size threshold or None)."""
    big = 0.1 * extent if max_screen_size else None
    smax_thr = [PD * extent] + ([big, big * 0.8 * N] if big is not None else [])
    return smax_thr, big


def _near(x, thr):
    return (x / thr - 1.0).abs() < MARGIN


def _quantities(raw, accum, denom):
    g = accum.double().squeeze(-1) / denom.double().squeeze(-1)
    g[g.isnan()] = 0.0
    return g, raw["scaling"].double().exp().max(dim=1).values, torch.sigmoid(raw["opacity"].double()).squeeze(-1)


def _off_thresholds(raw, accum, denom, max_grad, min_opacity, extent, max_screen_size, N):
    """Multiplies by 1.01 every compared quantity within MARGIN of its threshold (in place)."""
    smax_thr, _ = _thresholds(extent, max_screen_size, N)
    for _ in range(4):
        g, smax, sig = _quantities(raw, accum, denom)
        accum[_near(g, max_grad)] *= 1.01
        near = torch.zeros_like(smax, dtype=torch.bool)
        for t in smax_thr:
            near |= _near(smax, t)
        raw["scaling"][near] += float(torch.log(torch.tensor(1.01)))
        n = _near(sig, min_opacity)
        s = (1.01 * sig[n])
        raw["opacity"][n] = torch.log(s / (1 - s)).float()[:, None]


def _assert_margins(raw, accum, denom, max_grad, min_opacity, extent, max_screen_size, N):
    smax_thr, _ = _thresholds(extent, max_screen_size, N)
    g, smax, sig = _quantities(raw, accum, denom)
    assert not _near(g, max_grad).any() and not _near(sig, min_opacity).any()
    for t in smax_thr:  # (the children's smax / (0.8 N) against big is smax against big * 0.8 N)
        assert not _near(smax, t).any()


def _case(P, N, max_screen_size, seed, max_grad=5e-4, min_opacity=0.05, extent=1.3, M=15):
    g = torch.Generator().manual_seed(seed)
    raw = {"xyz": torch.randn(P, 3, generator=g), "f_dc": torch.randn(P, 1, 3, generator=g),
           "f_rest": 0.1 * torch.randn(P, M, 3, generator=g), "opacity": torch.randn(P, 1, generator=g) * 3.0,
           # largest scales from 0.003 to 0.6: below and above 0.01 extent, 0.1 extent and 0.1 extent x 0.8 N
           "scaling": torch.log(torch.tensor(0.003)) + torch.rand(P, 3, generator=g) * torch.log(torch.tensor(200.0)),
           "rotation": torch.randn(P, 4, generator=g)}
    raw["f_dc"][:, 0, 0] = torch.arange(P, dtype=torch.float32)  # the source row travels with every output row
    accum = torch.rand(P, 1, generator=g) * 2e-3
    denom = torch.randint(0, 3, (P, 1), generator=g).float()  # zeros: 0/0 -> 0 and x/0 -> inf
    if P > 8:
        accum[0:P:7] = 0.0
        denom[0:P:7] = 0.0
    state = {k: (torch.randn(raw[k].shape, generator=g), torch.rand(raw[k].shape, generator=g)) for k in NAMES}
    _off_thresholds(raw, accum, denom, max_grad, min_opacity, extent, max_screen_size, N)
    _assert_margins(raw, accum, denom, max_grad, min_opacity, extent, max_screen_size, N)
    return raw, accum, denom, state, (max_grad, min_opacity, extent, max_screen_size)


def _stats(accum, denom, dev):
    from diff_gaussian_rasterization import multiview as mv
    st = mv.densification_stats(accum.shape[0], dev)
    st["xyz_gradient_accum"].copy_(accum)
    st["denom"].copy_(denom)
    return st


def _spy_randn(monkeypatch):
    drawn, randn = [], torch.randn

    def spy(*a, **kw):
        drawn.append(randn(*a, **kw))
        return drawn[-1]
    monkeypatch.setattr(torch, "randn", spy)
    return drawn


# ---- float64 evaluation of the children -----------------------------------------------------------
def _rot64(q):
    q = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    return torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                        2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                        2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], dim=1).view(-1, 3, 3)


def _children64(raw, src, z):
    """float64 (xyz, its bound, exp(scaling), exp(scaling) z) of children with source rows `src`, samples z."""
    s = raw["scaling"][src].double().exp()
    v = s * z.double()
    xyz0 = raw["xyz"][src].double()
    xyz = torch.bmm(_rot64(raw["rotation"][src].double()), v[:, :, None]).squeeze(-1) + xyz0
    xyz_bound = 2.0 ** -19 * (xyz0.abs() + v.abs().sum(dim=1, keepdim=True))
    return xyz, xyz_bound, s, v


def _check_children(tag, got_xyz, got_scaling, raw, src, z, N):
    xyz, xyz_bound, s, _ = _children64(raw, src, z)
    scaling = torch.log(s / (0.8 * N))
    sc_bound = 2.0 ** -21 * scaling.abs().clamp_min(1.0)
    ex = (got_xyz.double() - xyz).abs() / xyz_bound
    es = (got_scaling.double() - scaling).abs() / sc_bound
    print(f"{tag}: children {len(src)}: max xyz error / bound {float(ex.max()):.3f}, "
          f"max scaling error / bound {float(es.max()):.3f}")
    assert float(ex.max()) <= 1.0 and float(es.max()) <= 1.0


def _compare(tag, got_T, got_S, ref_T, ref_S, raw, accum, denom, thr, N, z, moments, n_children, src=None):
    """got (CPU copies of the fused result) against ref: copies bit for bit, children within bounds.
    src: the children's source rows (default: read from f_dc[:, 0, 0], where _case put them)."""
    max_grad, _, extent, _ = thr
    P1 = ref_T["xyz"].shape[0]
    first_child = P1 - n_children
    for k in NAMES:
        assert got_T[k].shape == ref_T[k].shape, k
        rows = first_child if k in ("xyz", "scaling") else P1
        assert torch.equal(got_T[k][:rows], ref_T[k][:rows]), k
        if moments:
            assert torch.equal(got_S[k]["exp_avg"], ref_S[k]["exp_avg"]), k
            assert torch.equal(got_S[k]["exp_avg_sq"], ref_S[k]["exp_avg_sq"]), k
        else:
            assert "exp_avg" not in got_S[k] and "exp_avg_sq" not in got_S[k]
    # a child's source row (carried by f_dc), its rank among all split rows, its r
    g, smax, _ = _quantities(raw, accum, denom)
    split = (g >= max_grad) & (smax > PD * extent)
    rank = torch.cumsum(split.long(), 0) - 1
    n_split, n_ks = int(split.sum()), n_children // N
    if src is None:
        src = ref_T["f_dc"][first_child:, 0, 0].long()
    assert len(src) == n_children and bool(split[src].all()) and torch.equal(src[:n_ks].repeat(N), src)
    r = torch.arange(n_children) // max(n_ks, 1)
    zc = z[r * n_split + rank[src]]
    _check_children(tag + " fused", got_T["xyz"][first_child:], got_T["scaling"][first_child:], raw, src, zc, N)
    _check_children(tag + " torch", ref_T["xyz"][first_child:], ref_T["scaling"][first_child:], raw, src, zc, N)


def _rows_per_workgroup():
    from diff_gaussian_rasterization import _C
    return _C.densify_rows_per_workgroup()


# ---- 1. kernel against the reference ----------------------------------------------------------------
# densify_offsets_kernel: 256 threads, thread t owns the per = ceil(nw / 256) waves from t per on.  Up
# to 256 waves (the first two sizes) a thread's loop runs at most once; the last three sizes, in
# rows per wave (w), are 256 waves (every thread one wave: the serial pass sees 256 partial sums), 257
# waves (per = 2: threads 0..127 two waves, thread 128 the last wave of one row, the others none)
# and 770 waves less 19 rows (per = 4: threads 0..191 four waves, thread 192 two).
LARGE_P = ("256w", "256w+1", "770w-19")


def _sequence_cases():
    """P x N x moments x world-size prune; the largest P with N = 2 and the world-size prune only."""
    for P in (1037, "3wg+5") + LARGE_P:
        for N in (2, 3):
            for moments in (True, False):
                for mss in (None, 20):
                    if P != "770w-19" or (N == 2 and mss):
                        yield pytest.param(P, N, moments, mss, id=f"{P}-{N}-{'moments' if moments else 'no-moments'}-"
                                                                  f"{'world-size' if mss else 'no-world-size'}")


def _decision_masks(raw, accum, denom, thr, N):
    """The five decisions densify_decide_kernel counts per wave, from the float64 quantities (off
    the thresholds, so the fp32 decisions of the reference are the same)."""
    max_grad, min_opacity, extent, max_screen_size = thr
    g, smax, sig = _quantities(raw, accum, denom)
    hot = g >= max_grad
    clone, split = hot & (smax <= PD * extent), hot & (smax > PD * extent)
    low = sig < min_opacity
    big = smax > 0.1 * extent if max_screen_size else torch.zeros_like(low)
    bigchild = smax / (0.8 * N) > 0.1 * extent if max_screen_size else torch.zeros_like(low)
    keep = ~(low | big)
    return {"keep_orig": ~split & keep, "keep_clone": clone & keep, "split": split,
            "keep_split": split & ~(low | bigchild), "clone": clone}


def _assert_waves_beyond_the_first(masks, P, rpw):
    """Every count is non-zero in a wave of a thread t >= 1 (its offset comes from the serial pass over
    the partial sums) and, where threads own several waves, in the second wave of some thread (its
    offset is the partial sum plus the thread's first wave) and in the wave before it."""
    nw = (P + rpw - 1) // rpw
    per = (nw + 255) // 256
    wave = torch.arange(nw)
    for name, m in masks.items():
        cnt = torch.zeros(nw * rpw, dtype=torch.long)
        cnt[:P] = m.long()
        cnt = cnt.view(nw, rpw).sum(1)
        assert bool((cnt[wave // per >= 1] > 0).any()), name
        if per > 1:
            second = (wave % per == 1) & (cnt > 0)
            assert bool((second & (cnt[(wave - 1).clamp_min(0)] > 0)).any()), name


@pytest.mark.gpu
@pytest.mark.parametrize("P,N,moments,max_screen_size", list(_sequence_cases()))
def test_matches_reference_sequence(P, N, moments, max_screen_size, monkeypatch):
    from diff_gaussian_rasterization import multiview as mv
    large = P in LARGE_P
    rpw = _rows_per_workgroup() // 4  # rows per wave
    if P == "3wg+5":
        P = 3 * _rows_per_workgroup() + 5
        assert P >= 10000
    elif large:
        P = {"256w": 256 * rpw, "256w+1": 256 * rpw + 1, "770w-19": 770 * rpw - 19}[P]
    # (one f_rest coefficient at the large sizes: the plan does not read it, the copies stay quick)
    raw, accum, denom, state, thr = _case(P, N, max_screen_size, seed=P + 10 * N, M=1 if large else 15)
    masks = _decision_masks(raw, accum, denom, thr, N)
    if large:
        _assert_waves_beyond_the_first(masks, P, rpw)
    dev = torch.device("cuda", 0)
    step = torch.tensor(3.0)
    S = {k: {"step": step, "exp_avg": state[k][0].to(dev), "exp_avg_sq": state[k][1].to(dev)} for k in NAMES} \
        if moments else {}
    drawn = _spy_randn(monkeypatch)
    T1, S1, counts = mv.fused_densify_and_prune({k: v.to(dev) for k, v in raw.items()}, S, _stats(accum, denom, dev),
                                                thr[0], thr[1], thr[2], thr[3], PD, N,
                                                torch.Generator(device=dev).manual_seed(1))
    torch.cuda.synchronize()
    assert len(drawn) == 1 and tuple(drawn[0].shape) == (N * counts["split"], 3)
    z = drawn[0].cpu()
    grads = accum / denom
    grads[grads.isnan()] = 0.0
    ref_counts = {}
    ref_T, ref_S = _ref_densify(raw, state, grads, thr[0], thr[1], thr[2], thr[3], None, pd=PD, N=N,
                                normal=lambda stds: z * stds, counts=ref_counts)
    print("counts:", counts)
    assert {k: counts[k] for k in ref_counts} == ref_counts and counts["P_before"] == P
    assert counts["cloned"] > 0 and counts["split"] > 0 and counts["pruned"] > 0
    # the masks sliced by wave above are the reference's decisions
    n = {k: int(m.sum()) for k, m in masks.items()}
    assert (n["clone"], n["split"]) == (ref_counts["cloned"], ref_counts["split"])
    assert n["keep_orig"] + n["keep_clone"] + N * n["keep_split"] == ref_counts["P_after"]
    # the children: the output rows whose source row (carried by f_dc) was split
    src_all = ref_T["f_dc"][:, 0, 0].long()
    g, smax, _ = _quantities(raw, accum, denom)
    split = (g >= thr[0]) & (smax > PD * thr[2])
    n_children = int(split[src_all].sum())
    assert n_children % N == 0 and n_children // N < counts["split"], "some split parent is pruned"
    assert n_children > 0
    got_T = {k: v.cpu() for k, v in T1.items()}
    got_S = {k: {n: (t.cpu() if torch.is_tensor(t) else t) for n, t in S1[k].items()} for k in NAMES}
    if moments:
        assert all(S1[k]["step"] is step for k in NAMES)
    _compare(f"P={P} N={N}", got_T, got_S, ref_T, ref_S, raw, accum, denom, thr, N, z, moments, n_children)


# ---- 2. single rows and no rows -------------------------------------------------------------------
def _single(outcome, P=1):
    raw = {"xyz": torch.tensor([[0.5, -1.0, 2.0]]), "f_dc": torch.tensor([[[0.1, 0.2, 0.3]]]),
           "f_rest": torch.arange(45, dtype=torch.float32).view(1, 15, 3), "opacity": torch.tensor([[0.3]]),
           "scaling": torch.log(torch.tensor([[0.01, 0.005, 0.002]])), "rotation": torch.tensor([[0.9, 0.1, -0.3, 0.2]])}
    accum, denom = torch.tensor([[0.1]]), torch.tensor([[1.0]])
    if outcome in ("cloned", "split"):
        accum[:] = 1.0
    if outcome == "split":
        raw["scaling"] = torch.log(torch.tensor([[0.05, 0.01, 0.02]]))
    if outcome == "pruned":
        raw["opacity"][:] = -10.0
    if P == 0:
        raw = {k: v[:0] for k, v in raw.items()}
        accum, denom = accum[:0], denom[:0]
    return raw, accum, denom


@pytest.mark.gpu
@pytest.mark.parametrize("outcome", ["kept", "cloned", "split", "pruned", "empty"])
def test_single_row(outcome, monkeypatch):
    from diff_gaussian_rasterization import multiview as mv
    dev = torch.device("cuda", 0)
    raw, accum, denom = _single(outcome, P=0 if outcome == "empty" else 1)
    P = raw["xyz"].shape[0]
    S = {k: {"step": torch.tensor(1.0), "exp_avg": torch.full_like(v, 2.0).to(dev),
             "exp_avg_sq": torch.full_like(v, 3.0).to(dev)} for k, v in raw.items()}
    drawn = _spy_randn(monkeypatch)
    T1, S1, c = mv.fused_densify_and_prune({k: v.to(dev) for k, v in raw.items()}, S, _stats(accum, denom, dev),
                                           0.5, 0.05, 1.3, 20, PD, 2, torch.Generator(device=dev).manual_seed(2))
    torch.cuda.synchronize()
    want = {"kept": (0, 0, 0, 1), "cloned": (1, 0, 0, 2), "split": (0, 1, 0, 2), "pruned": (0, 0, 1, 0),
            "empty": (0, 0, 0, 0)}[outcome]
    assert (c["cloned"], c["split"], c["pruned"], c["P_after"]) == want and c["P_before"] == P
    for k in NAMES:
        assert tuple(T1[k].shape) == (want[3],) + tuple(raw[k].shape[1:]), k
        assert S1[k]["exp_avg"].shape == T1[k].shape and S1[k]["exp_avg_sq"].shape == T1[k].shape
        got = T1[k].cpu()
        if outcome in ("kept", "cloned"):
            assert torch.equal(got, raw[k].repeat((want[3],) + (1,) * (raw[k].dim() - 1))), k
            m = torch.tensor([2.0] + [0.0] * (want[3] - 1))
            assert torch.equal(S1[k]["exp_avg"].cpu().flatten(1)[:, 0], m)
            assert torch.equal(S1[k]["exp_avg_sq"].cpu().flatten(1)[:, 0], 1.5 * m)
        if outcome == "split":
            assert float(S1[k]["exp_avg"].abs().sum()) == 0.0 and float(S1[k]["exp_avg_sq"].abs().sum()) == 0.0
            if k not in ("xyz", "scaling"):
                assert torch.equal(got, raw[k].repeat((2,) + (1,) * (raw[k].dim() - 1))), k
    if outcome == "split":
        src = torch.zeros(2, dtype=torch.long)
        _check_children("single split", T1["xyz"].cpu(), T1["scaling"].cpu(), raw, src, drawn[0].cpu(), 2)


# ---- 3. + 4. the trainer and its generator ---------------------------------------------------------
def _trained(dev, fused_densify):
    from test_fused_tail_train import _setup
    trainer, views = _setup(dev, False)
    trainer.fused_densify = fused_densify
    for _ in range(2):
        trainer.step(views)
    torch.cuda.synchronize()
    return trainer, views


@pytest.mark.gpu
def test_trainer_and_generator(monkeypatch):
    dev = torch.device("cuda", 0)
    N = 2
    ref, views = _trained(dev, False)
    fus, _ = _trained(dev, True)
    assert fus.fused_densify and not ref.fused_densify
    # the same start for both (the two runs above are the same computation; this makes it so by construction)
    with torch.no_grad():
        for k in NAMES:
            fus.params[k].copy_(ref.params[k])
            for m in ("exp_avg", "exp_avg_sq"):
                fus.optimizer.state[fus.params[k]][m].copy_(ref.optimizer.state[ref.params[k]][m])
        fus.stats["_sums"].copy_(ref.stats["_sums"])
    raw = {k: p.detach().cpu().clone() for k, p in ref.params.items()}
    accum, denom = ref.stats["xyz_gradient_accum"].cpu().clone(), ref.stats["denom"].cpu().clone()
    assert float(denom.max()) > 0
    # thresholds from the data (some of the seen rows hot, half of those small, some rows
    # transparent), off every value they are compared with
    g, smax, sig = _quantities(raw, accum, denom)

    def in_widest_gap(values, lo, hi):
        """A threshold in the middle of the widest relative gap between the lo and hi quantiles of the
        distinct values (trained values lie densely, and many opacities are still equal)."""
        v = torch.unique(values[values > 0])
        v = v[int(lo * (len(v) - 1)):int(hi * (len(v) - 1)) + 2]
        k = int((v[1:] / v[:-1]).argmax())
        return float((v[k] * v[k + 1]).sqrt())
    max_grad = in_widest_gap(g, 0.3, 0.7)
    min_opacity = in_widest_gap(sig, 0.02, 0.3)
    extent = float(smax[g >= max_grad].median()) / PD
    for _ in range(2000):  # raised in steps wider than the margin's window until all three are clear
        if not any(_near(smax, t).any() for t in _thresholds(extent, 20, N)[0]):
            break
        extent *= 1.003
    _assert_margins(raw, accum, denom, max_grad, min_opacity, extent, 20, N)
    thr = (max_grad, min_opacity, extent, 20)
    drawn = _spy_randn(monkeypatch)
    did_ref = ref.densify_and_prune(*thr, N=N)
    assert len(drawn) == 0  # the default path draws with torch.normal, as before
    did_fus = fus.densify_and_prune(*thr, N=N)
    torch.cuda.synchronize()
    print("trainer counts:", did_fus)
    assert did_fus == did_ref and fus.P == ref.P == did_ref["P_after"]
    assert did_ref["cloned"] > 0 and did_ref["split"] > 0 and did_ref["pruned"] > 0
    # 4. the generators moved alike
    assert torch.equal(fus.gen.get_state(), ref.gen.get_state())
    z = drawn[0].cpu()
    got_T = {k: p.detach().cpu() for k, p in fus.params.items()}
    ref_T = {k: p.detach().cpu() for k, p in ref.params.items()}
    got_S = {k: {m: fus.optimizer.state[p][m].cpu() for m in ("exp_avg", "exp_avg_sq")} for k, p in fus.params.items()}
    ref_S = {k: {m: ref.optimizer.state[p][m].cpu() for m in ("exp_avg", "exp_avg_sq")} for k, p in ref.params.items()}
    # the children are the rows with zero moments behind the kept originals and the clones: count
    # them from the decisions (float64, off the thresholds)
    split = (g >= max_grad) & (smax > PD * extent)
    low = sig < min_opacity
    child_big = smax / (0.8 * N) > 0.1 * extent
    n_children = N * int((split & ~(low | child_big)).sum())
    assert 0 < n_children < ref.P
    # the children's source rows: the kept split parents in source order, N times over
    src = torch.nonzero(split & ~(low | child_big)).squeeze(1).repeat(N)
    _compare("trainer", got_T, got_S, ref_T, ref_S, raw, accum, denom, thr, N, z, True, n_children, src)
    for tr in (fus, ref):
        for k, p in tr.params.items():  # gradients: zeroed views of the rebuilt flat buffer
            assert p.grad.shape == p.shape and p.grad.untyped_storage().data_ptr() == tr.flat.untyped_storage().data_ptr()
            assert tr.optimizer.state[p]["step"] is not None
        assert float(tr.flat.abs().sum()) == 0.0 and tr._skip_step == set(NAMES)
        assert tr.stats["denom"].shape == (tr.P, 1)
        losses = tr.step(views)
        assert all(bool(torch.isfinite(l)) for l in losses)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_randn_times_std_is_torch_normal():
    dev = torch.device("cuda", 0)
    stds = (torch.rand((2 * 777, 3), generator=torch.Generator().manual_seed(4)) * 0.1).to(dev)
    a, b = torch.Generator(device=dev).manual_seed(11), torch.Generator(device=dev).manual_seed(11)
    x = torch.normal(mean=torch.zeros_like(stds), std=stds, generator=a)
    y = torch.randn(stds.shape, generator=b, device=dev) * stds
    assert torch.equal(x, y) and torch.equal(a.get_state(), b.get_state())


# ---- 5. bindings -----------------------------------------------------------------------------------
@pytest.mark.gpu
def test_bindings_reject_bad_input():
    from diff_gaussian_rasterization import _C
    dev = torch.device("cuda", 0)
    P = 4
    accum, denom = torch.ones((P, 1)), torch.ones((P, 1))
    scaling, opacity = torch.zeros((P, 3)), torch.zeros((P, 1))
    args = (1.0, 0.01, 0.05, None, 2)
    with pytest.raises(RuntimeError, match="GPU only"):
        _C.densify_plan(accum, denom, scaling, opacity, *args)
    accum, denom, scaling, opacity = accum.to(dev), denom.to(dev), scaling.to(dev), opacity.to(dev)
    with pytest.raises(RuntimeError, match="scaling"):
        _C.densify_plan(accum, denom, scaling.double(), opacity, *args)
    with pytest.raises(RuntimeError, match="scaling"):
        _C.densify_plan(accum, denom, scaling[:, :2].contiguous(), opacity, *args)
    with pytest.raises(RuntimeError, match="opacity"):
        _C.densify_plan(accum, denom, scaling, opacity.double(), *args)
    with pytest.raises(RuntimeError, match="opacity"):
        _C.densify_plan(accum, denom, scaling, opacity[:3], *args)
    ws, counts = _C.densify_plan(accum, denom, scaling, opacity, *args)  # g = 1 >= 1, scales 1 > 0.01: all split
    assert counts == {"cloned": 0, "split": P, "pruned": 0, "P_after": 2 * P}
    names = ["xyz", "scaling", "rotation"]
    src = {"xyz": torch.zeros((P, 3), device=dev), "scaling": scaling, "rotation": torch.ones((P, 4), device=dev)}
    dst = {k: torch.empty((2 * P,) + tuple(v.shape[1:]), device=dev) for k, v in src.items()}
    with pytest.raises(RuntimeError, match="samples"):
        _C.densify_apply(ws, counts, 2, names, src, {}, dst, {}, torch.zeros((2 * P, 3), device=dev).double())
    with pytest.raises(RuntimeError, match="samples"):
        _C.densify_apply(ws, counts, 2, names, src, {}, dst, {}, torch.zeros((2 * P - 1, 3), device=dev))
    with pytest.raises(RuntimeError, match="GPU only"):
        _C.densify_apply(ws, counts, 2, names, {k: v.cpu() for k, v in src.items()}, {}, dst, {},
                         torch.zeros((2 * P, 3), device=dev))
    with pytest.raises(RuntimeError, match="new xyz"):
        _C.densify_apply(ws, counts, 2, names, src, {}, dict(dst, xyz=dst["xyz"][:P]), {},
                         torch.zeros((2 * P, 3), device=dev))


# ---- 6. the C ABI's argument checks (no device) ------------------------------------------------------
def test_capi_checks_arguments_without_a_device():
    from diff_gaussian_rasterization import _C
    lib = _C.lib
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    counts = (ctypes.c_int * 4)(7, 7, 7, 7)

    def plan(P=4, accum=p, sa=1, denom=p, sd=1, scaling=p, opacity=p, N=2, ws=p, cnt=counts):
        return lib.gsr_densify_plan(P, accum, sa, denom, sd, scaling, opacity, 1.0, 0.01, 0.05, -1.0, N, ws, cnt, None)

    assert plan(P=0, accum=None, denom=None, scaling=None, opacity=None, ws=None) == 0 and list(counts) == [0, 0, 0, 0]
    for kw, word in (({"P": -1}, b"P must"), ({"N": 0}, b"N must"), ({"sa": 0}, b"strides"), ({"sd": 0}, b"strides"),
                     ({"accum": None}, b"null"), ({"denom": None}, b"null"), ({"scaling": None}, b"null"),
                     ({"opacity": None}, b"null"), ({"ws": None}, b"null"), ({"cnt": None}, b"null")):
        assert plan(**kw) == 1, kw
        assert word in lib.gsr_last_error(), (kw, lib.gsr_last_error())

    n = 3
    ptrs = (ctypes.c_void_p * n)(p.value, p.value, p.value)
    nulls = (ctypes.c_void_p * n)(None, None, None)

    def apply(P=4, P_after=6, n_split=1, N=2, n_groups=n, Ms=(3, 3, 4), roles=(0, 1, 2), src=ptrs, src_m=nulls,
              src_v=nulls, dst=ptrs, dst_m=nulls, dst_v=nulls, samples=p, ws=p):
        return lib.gsr_densify_apply(P, P_after, n_split, N, n_groups, (ctypes.c_int * len(Ms))(*Ms), *roles, src,
                                     src_m, src_v, dst, dst_m, dst_v, samples, ws, None)

    assert apply(P=0, src=None, src_m=None, src_v=None, dst=None, dst_m=None, dst_v=None, samples=None, ws=None) == 0
    one_null = (ctypes.c_void_p * n)(p.value, None, p.value)
    for kw, word in (({"P": -1}, b"must be >= 0"), ({"P_after": -1}, b"must be >= 0"), ({"n_split": -1}, b"must be >= 0"),
                     ({"n_groups": -1}, b"must be >= 0"), ({"N": 0}, b"N must"), ({"n_groups": 9}, b"n_groups"),
                     ({"roles": (3, 1, 2)}, b"xyz_group"), ({"roles": (0, -1, 2)}, b"scaling_group"),
                     ({"roles": (0, 1, 3)}, b"rotation_group"), ({"Ms": (4, 3, 4)}, b"xyz group"),
                     ({"Ms": (3, 1, 4)}, b"scaling group"), ({"Ms": (3, 3, 3)}, b"rotation group"),
                     ({"samples": None}, b"samples"), ({"src": None}, b"null"), ({"dst_m": None}, b"null"),
                     ({"ws": None}, b"null"), ({"src": one_null}, b"null group"), ({"dst": one_null}, b"null group"),
                     ({"dst_m": ptrs}, b"moment")):
        assert apply(**kw) == 1, kw
        assert word in lib.gsr_last_error(), (kw, lib.gsr_last_error())

    lib.gsr_densify_workspace_size.restype = ctypes.c_size_t
    sizes = [lib.gsr_densify_workspace_size(P) for P in (0, 1, 1000, 4096, 4097, 100000, 1 << 20)]
    assert sizes[0] == 0 and sizes == sorted(sizes) and sizes[-1] > sizes[1] > 0
    assert lib.gsr_densify_rows_per_workgroup() >= 1024
