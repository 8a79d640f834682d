"""DataParallelTrainer(compact_reduce=True) against the dense all-reduce on real rasterizer
gradients (needs an MI355X: -m gpu; gloo ranks share the one GPU, as in test_dp_train.py).

The scene is test_dp_train's with every position multiplied by 3.0, so that a view sees about a
third of the 2000 Gaussians and a step of 4 views about 0.6 of them (the C oracle's figures:
1204 / 1227 of 2000): the union is well below COMPACT_BELOW and every step must compact.

World 2: one spawn; each worker builds pairs of trainers from identical starts (compact_reduce off
and on), steps both on the same views through the same process group and compares after every step:
parameters and both Adam moments bit for bit (int32 views), the flat buffer with torch.equal.  a + b
commutes and compaction only leaves out rows whose terms are all zero, so nothing may differ.  (The
sign of a zero cannot differ either: rows outside the union hold the +0 of zero_grad() on both
sides, +0 + +0 being +0.)

World 3: a ring sums in an order that depends on how the buffer is split, so the compact and the
dense run may round differently; every rank must still be bit-identical to every other, and every
parameter within K_ULP * 2^-24 * max|tensor| of the dense run after 3 steps.  Measured on gloo
(three ranks on one MI355X, this scene), the ratio |compact - dense| / (2^-24 max|tensor|) per tensor,
the same on every rank: pipelined (pair A) xyz 0.007, f_dc 0.80, f_rest 1.10, opacity 1.53, scaling
1.21, rotation 0.84; unpipelined (pair B) f_rest 0.55 and 0 for the other five.  The largest is 1.53;
K_ULP is 4 x that, rounded up to one decimal.
"""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

P, H, W, VIEWS, BATCH, ITERS = 2000, 96, 128, 8, 4, 3
SPREAD = 3.0
K_ULP = 6.2  # 4 x 1.53, the largest ratio that occurred (docstring)
EXTENT = 1.3
D_ITERS = 4  # iterations 1..4: densify at 2 and 4, opacity reset at 3


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _collect(q, procs, timeout=240):
    """The workers' results; fails fast (instead of waiting out the timeout) when a worker dies --
    its peer may then wait in a collective forever, so every worker is terminated."""
    import queue
    import time
    res, t0 = [], time.monotonic()
    try:
        while len(res) < len(procs):
            try:
                res.append(q.get(timeout=2))
            except queue.Empty:
                dead = [p.exitcode for p in procs if p.exitcode not in (None, 0)]
                assert not dead, f"a worker failed (exit codes {[p.exitcode for p in procs]})"
                assert time.monotonic() - t0 < timeout, "workers timed out"
    finally:
        for p in procs:
            p.join(timeout=30 if len(res) == len(procs) else 1)
            if p.is_alive():
                p.terminate()
                p.join(timeout=10)
    return sorted(res, key=lambda r: r[0])


def _densify_opt(threshold):
    from diff_gaussian_rasterization import multiview
    o = multiview.OptimizationDefaults()
    o.densify_from_iter, o.densification_interval, o.opacity_reset_interval = 0, 2, 3
    o.densify_until_iter, o.densify_grad_threshold = 100, threshold
    return o


def _scene(dev):
    """test_dp_train._setup's construction with the positions spread by 3.0: the perturbed start,
    the settings per view and the ground-truth images."""
    import synthetic
    import diff_gaussian_rasterization as dgr
    gt = synthetic.make_scene(P, seed=0)
    gt["means3D"] = gt["means3D"] * SPREAD
    g = torch.Generator().manual_seed(5)
    raw = {"xyz": gt["means3D"] + SPREAD * 0.02 * torch.randn(P, 3, generator=g),
           "f_dc": gt["shs"][:, :1] + 0.3 * torch.randn(P, 1, 3, generator=g),
           "f_rest": gt["shs"][:, 1:].clone(),
           "opacity": torch.full((P, 1), -1.0),
           "scaling": torch.log(gt["scales"]) + 0.3 * torch.randn(P, 3, generator=g),
           "rotation": gt["rotations"] + 0.1 * torch.randn(P, 4, generator=g)}
    raw = {k: v.to(dev) for k, v in raw.items()}
    settings = []
    for v in range(VIEWS):
        c = synthetic.Camera(W, H, view=v)
        settings.append(dgr.GaussianRasterizationSettings(
            H, W, c.tanfovx, c.tanfovy, torch.zeros(3, device=dev), 1.0, c.world_view_transform.to(dev),
            c.full_proj_transform.to(dev), 3, c.camera_center.to(dev), False, False, False))
    gt_t = {k: v.to(dev) for k, v in gt.items()}
    with torch.no_grad():
        targets = [dgr.GaussianRasterizer(s)(means3D=gt_t["means3D"], means2D=torch.zeros_like(gt_t["means3D"]),
                                             shs=gt_t["shs"], opacities=gt_t["opacities"], scales=gt_t["scales"],
                                             rotations=gt_t["rotations"])[0].clamp(0, 1) for s in settings]
    return raw, settings, targets


def _views(it, rank, world, settings, targets, cams=False):
    from diff_gaussian_rasterization import multiview
    batch = [(BATCH * it + j) % VIEWS for j in range(BATCH)]
    mine = [batch[j] for j in multiview.views_of_batch(rank, world, BATCH)]
    return [(settings[v], targets[v], {"cam": v}) if cams else (settings[v], targets[v]) for v in mine]


def _bits(t):
    return t.detach().contiguous().view(torch.int32)


def _same(a, b, what):
    """Trainers a (dense) and b (compact): parameters, moments and the flat buffer."""
    assert a.P == b.P, what
    for k in a.params:
        assert torch.equal(_bits(a.params[k]), _bits(b.params[k])), f"{what}: {k}"
        sa, sb = a.optimizer.state.get(a.params[k], {}), b.optimizer.state.get(b.params[k], {})
        assert set(sa) == set(sb), f"{what}: {k} state"
        for m in ("exp_avg", "exp_avg_sq"):
            if m in sa:
                assert torch.equal(_bits(sa[m]), _bits(sb[m])), f"{what}: {k} {m}"
    assert torch.equal(a.flat, b.flat), f"{what}: flat"
    if a.exposures is not None:
        assert torch.equal(_bits(a.exposures), _bits(b.exposures)), f"{what}: exposures"


def _compacted(t, what, log, P_then=None):
    """The last exchange of trainer t compacted, at a union fraction the scene was built for.
    P_then: the row count when it ran (an iteration that densifies changes t.P afterwards)."""
    r = t.last_reduce
    print(f"{what}: {r}", file=log, flush=True)
    assert r is not None and r["mode"] == "compact", (what, r)
    assert r["P"] == (t.P if P_then is None else P_then) and 0.3 < r["U"] / r["P"] < 0.75, (what, r)
    return r


def _pair(raw, **kw):
    from diff_gaussian_rasterization import multiview
    return (multiview.DataParallelTrainer(raw, lr={"xyz": 4.8e-4}, **kw),
            multiview.DataParallelTrainer(raw, lr={"xyz": 4.8e-4}, compact_reduce=True, **kw))


def _init(rank, world, port):
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "gaussian-splatting-npu_amd"), os.path.join(root, "tests")):
        sys.path.insert(0, p)
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    return dist, dev, sys.stderr  # (each exchange's figures go to the worker's stderr: pytest -s shows them)


def _steps(pair, name, rank, world, settings, targets, log, expect="compact"):
    """ITERS step()s of both trainers of a pair, compared after each."""
    dense, comp = pair
    for it in range(ITERS):
        views = _views(it, rank, world, settings, targets)
        dense.step(views)
        comp.step(views)
        assert dense.last_reduce is None
        if expect == "compact":
            _compacted(comp, f"{name} step {it}", log)
        else:
            assert comp.last_reduce["mode"] == expect, (name, comp.last_reduce)
        if world == 2:
            _same(dense, comp, f"{name} step {it}")


def _worker2(rank, port, q):
    world = 2
    dist, dev, log = _init(rank, world, port)
    try:
        from diff_gaussian_rasterization import _C, multiview
        raw, settings, targets = _scene(dev)
        words = (P + 31) // 32
        # A: sparse Adam, the pipelined reduce_and_step
        _steps(_pair(raw, pipeline_chunks=4), "A", rank, world, settings, targets, log)
        # B: sparse Adam, unpipelined, step() spelled out for reduce()'s byte count
        dense, comp = _pair(raw, pipeline_chunks=1)
        for it in range(ITERS):
            views = _views(it, rank, world, settings, targets)
            for t in (dense, comp):
                t.zero_grad()
                t.render_and_backward(views)
            assert dense.reduce() == 4 * dense.flat.numel()
            sent = comp.reduce()
            r = _compacted(comp, f"B step {it}", log)
            assert sent == r["bytes"] == 4 * (r["U"] * 60 + words * world), (sent, r)
            # the union is what the reduced counts say
            assert int((comp.visible_count > 0).sum()) == r["U"]
            for t in (dense, comp):
                t.optimizer_step()
            _same(dense, comp, f"B step {it}")
        # C: torch Adam
        _steps(_pair(raw, optimizer="adam"), "C", rank, world, settings, targets, log)
        # E: a threshold below the union fraction: the dense collective on both ranks, same results
        _steps(_pair(raw, pipeline_chunks=4, compact_below=0.1), "E", rank, world, settings, targets, log, expect="dense")
        _steps(_pair(raw, pipeline_chunks=1, compact_below=0.1), "E1", rank, world, settings, targets, log,
               expect="dense")
        # D: iteration() across two densifications and an opacity reset, with exposures
        g = torch.Generator().manual_seed(3)
        exposures = torch.eye(3, 4)[None].repeat(VIEWS, 1, 1) + 0.05 * torch.randn(VIEWS, 3, 4, generator=g)
        raw_d = {k: v.clone() for k, v in raw.items()}
        raw_d["opacity"][::10] = -6.0  # below min_opacity: pruned at the first densification
        # a threshold that selects about half of the Gaussians the first densification sees (a dry run of
        # iterations 1-2 with both ranks' views, the same on every rank)
        dry = multiview.DataParallelTrainer(raw_d, lr={"xyz": 4.8e-4}, opt=_densify_opt(1.0), seed=11)
        for it in (1, 2):
            dry.zero_grad()
            for r in range(world):
                dry.render_and_backward(_views(it, r, world, settings, targets))
        threshold = float(torch.nan_to_num(dry.stats["xyz_gradient_accum"] / dry.stats["denom"], 0.0).median())
        assert threshold > 0
        # (the densifications clone and split rows the step sees: the union grows to 0.66 of the rows, past
        # the default threshold, so this pair compacts up to the 0.75 that _compacted() allows -- what it
        # checks is the exchange across a change of P, not the default)
        dense, comp = _pair(raw_d, opt=_densify_opt(threshold), seed=11, exposures=exposures, compact_below=0.75)
        did = []
        for it in range(1, D_ITERS + 1):
            views = _views(it, rank, world, settings, targets, cams=True)
            P_then = comp.P
            da = dense.iteration(it, views, EXTENT)[1]
            db = comp.iteration(it, views, EXTENT)[1]
            assert da == db, (it, da, db)
            did.append(db)
            r = _compacted(comp, f"D iteration {it}", log, P_then)
            assert r["bytes"] == 4 * (r["U"] * 60 + ((r["P"] + 31) // 32) * world) + 4 * exposures.numel(), r
            _same(dense, comp, f"D iteration {it}")
        assert did[0] is None and did[2] is None and did[1] is not None and did[3] is not None, did
        assert did[1]["cloned"] > 0 and did[1]["split"] > 0 and did[1]["pruned"] > 0, did
        assert comp.P != P and comp._compact.P == comp.P, did
        torch.cuda.synchronize()
        q.put((rank, did))
    finally:
        dist.destroy_process_group()


def _spawn(world, target):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=target, args=(r, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = _collect(q, procs)
    assert all(p.exitcode == 0 for p in procs)
    return res


def test_two_ranks_compact_equals_dense_bitwise():
    res = _spawn(2, _worker2)
    assert res[0][1] == res[1][1]


def _worker3(rank, port, q):
    world = 3
    dist, dev, log = _init(rank, world, port)
    try:
        raw, settings, targets = _scene(dev)
        out = {}
        for name, chunks in (("A", 4), ("B", 1)):
            pair = _pair(raw, pipeline_chunks=chunks)
            _steps(pair, name, rank, world, settings, targets, log)
            dense, comp = pair
            ratios = {}
            for k in comp.params:
                d, c = dense.params[k].detach().double(), comp.params[k].detach().double()
                ratios[k] = float((d - c).abs().max() / (2.0 ** -24 * d.abs().max()))
            print(f"{name} ratios {ratios}", file=log, flush=True)
            out[name] = ({k: p.detach().cpu().numpy() for k, p in comp.params.items()}, ratios)
        torch.cuda.synchronize()
        q.put((rank, out))
    finally:
        dist.destroy_process_group()


def test_three_ranks_agree_and_stay_near_dense():
    res = _spawn(3, _worker3)
    for name in ("A", "B"):
        ref = res[0][1][name][0]
        for rank, out in res:
            params, ratios = out[name]
            for k in ref:
                np.testing.assert_array_equal(params[k].view(np.int32), ref[k].view(np.int32),
                                              err_msg=f"{name} rank {rank} {k}")
            print(f"pair {name} rank {rank}: |compact - dense| / (2^-24 max|tensor|) = {ratios}")
            for k, r in ratios.items():
                assert r <= K_ULP, (name, rank, k, r)
