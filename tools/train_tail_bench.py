#!/usr/bin/env python3
"""Times the tail of a training iteration -- what sits between the rasterizer step and the Adam step
-- in its torch form against its fused HIP form, in ONE process on the GPU:

  loss:   per view clamp, (img - gt).abs().mean(), fused_ssim, the scalar mix, and their backward
          (DataParallelTrainer._view_loss on the clamped image)   vs   one fused_l1_ssim_loss
          call (photo_loss_fwd_kernel + photo_loss_bwd_kernel) and its backward;
  view_loss: what train.py:112-141 does per view with `train_test_exp` exposures, an alpha mask and a depth
          target on every view -- DataParallelTrainer._expose, clamp, _view_loss (mask, L1, fused_ssim,
          the inverse-depth L1 term) and their backward   vs   one fused_view_loss call on the raw
          renders (DataParallelTrainer._fused_view_losses: view_loss_fwd_kernel + view_loss_bwd_kernel and
          their small reductions) and its backward.  Gradients go to the image, the inverse depths and the
          exposures on both sides.  The byte model is 42 floats per pixel and view: forward 3 raw, 3
          ground-truth and the mask in, 9 partial planes out, and inverse depth, target and depth mask in;
          backward the 9 planes, raw, ground truth and mask in, 3 out, and the depth term's 3 in, 1 out.
  stats:  V x multiview.add_view_stats (boolean-mask indexing, a host synchronisation each)
          vs   one multiview.add_batch_stats launch (densify_stats_kernel);
  densify: DataParallelTrainer.densify_and_prune as the torch chain (two appends and two mask
          selections over six tensors and their Adam moments)   vs   fused_densify=True (one
          gsr_densify_plan and one gsr_densify_apply).  Both sides start every call from clones of the
          same 1M-Gaussian start (made outside the timed region) and include the rebuild of the flat
          gradient buffer both share; "fused_call" is multiview.fused_densify_and_prune alone, which
          the GB/s figure refers to.  Thresholds are quantiles of the seed-0 data: about 5 % of the
          rows clone, 5 % split and 5 % are pruned (the fractions are recorded).
  activations: exp(scaling), sigmoid(opacity), F.normalize(rotation) and torch.autograd.backward on the
          three outputs with fixed random gradients   vs   fused_activations (activate_fwd_kernel +
          activate_bwd_kernel) inside accumulate_grads_in_place() with the same backward.  The raw
          parameters carry .grad views of one flat buffer on both sides, so the torch side ends in
          three AccumulateGrad additions and the fused side adds in its kernel.  The byte model is
          64 B per Gaussian forward (32 in, 32 out) and 128 B backward with accumulation (saved
          outputs, raw quaternion and incoming gradients 64 in; destinations 32 in and 32 out).
  iteration: bench.py's aux_train_iteration restated at its scale (one 1M-Gaussian view at
          --width x --height, dc=, SparseGaussianAdam) in its torch form (torch activations, torch L1 +
          fused_ssim) against the all-HIP form (fused_activations, fused_l1_ssim_loss with V = 1),
          the optimizer step the same.  Wall clock: time.perf_counter() around synchronised groups of
          --group iterations, the two sides alternating group by group -- the host's dispatch cost is
          part of what is compared.  A report, not a gate.
  compact: the device side of multiview.compact_allreduce on ONE GPU, without a collective: for a
          (P, 60) gradient buffer at SH degree 3 (six gradient groups and the count column) and union
          masks at 0.25 / 0.5 / 0.75 / 1.0 of P (random) and the bench scene's own 8-view union,
          _C.visibility_pack + _C.union_plan (with its stream synchronisation), _C.rows_gather and
          _C.rows_scatter, beside a plain clone() of the same buffer as the HBM yardstick -- the four
          alternate call by call.  Byte models: pack + plan 4 B in per Gaussian, three passes over the
          P / 8 B of bits, 1 B of mask out and 4 B per union row; gather and scatter 4 + 8 x 60 = 484 B
          per union row each; clone 2 x 240 B per Gaussian.  The block also records the union fraction
          U / P of the scenes the repository has (the trainer test's spread scene, the chair fixture,
          the config-3-scale cloud) and the compact_below the measured copies give with DESIGN.md §8's
          ASSUMED link rate.  Nothing here is timed on more than one GPU.
  camera: the backward of the bench's step (--views views of --points Gaussians at --width x --height,
          one MultiViewRasterizer node, the forward re-run untimed before every call) without and with
          cameras= (the camera gradient: camera_bwd_views_kernel + camera_bwd_finish_kernel), the two
          alternating call by call; then the kernels' own HIP-event time from the library's profile scopes
          (gsr_profile_read) over --reps more backward passes with cameras=, beside preprocess_bwd's of the
          same passes -- the yardstick: the camera kernel reads the same records and visible rows and
          writes nothing per Gaussian.  Written to the block "camera_grads".

Defaults are the bench's flagship shape: 8 views, 1920x1080, 1M Gaussians, seed-0 data.  The two
sides alternate call by call; every call is bracketed by device events and ends in a
synchronise.  `--rounds` rounds of `--reps` timed calls per side (after `--warmup` untimed ones)
give one median per round; reported are the median of the round medians and their spread
(max - min).  The result -- times, spreads, the algorithmic bytes of the fused forms (11 floats per
plane-pixel for the loss) and the two sides' agreement on these inputs -- goes to --out as JSON
and to stdout as one line.  `--legs` selects the legs to run; the others keep their block of an
existing --out file.  Without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-npu_amd"))


LEGS = ("loss", "view_loss", "stats", "densify", "activations", "iteration", "compact", "camera")


def timed(fn, torch):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(sides, warmup, reps, rounds, torch):
    """{name: (median of round medians, spread of round medians, round medians)} in ms."""
    for _ in range(warmup):
        for fn in sides.values():
            timed(fn, torch)
    meds = {k: [] for k in sides}
    for _ in range(rounds):
        t = {k: [] for k in sides}
        for _ in range(reps):
            for k, fn in sides.items():
                t[k].append(timed(fn, torch))
        for k in sides:
            meds[k].append(statistics.median(t[k]))
    return {k: (statistics.median(m), max(m) - min(m), m) for k, m in meds.items()}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--points", type=int, default=1_000_000)
    ap.add_argument("--lambda-dssim", type=float, default=0.2)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", default=",".join(LEGS), help="comma-separated: " + ", ".join(LEGS))
    ap.add_argument("--group", type=int, default=10, help="iterations per timed group of the iteration leg")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_tail.json"))
    args = ap.parse_args()
    if args.warmup < 3 or args.reps < 20:
        ap.error("at least 3 warm-ups and 20 timed repetitions per side")
    legs = set(args.legs.split(","))
    if not legs or legs - set(LEGS):
        ap.error("--legs takes " + ", ".join(LEGS))
    if args.group < 1:
        ap.error("--group must be >= 1")

    import torch
    if not torch.cuda.is_available():
        sys.exit("train_tail_bench: no GPU found (this tool measures on the device; there is no CPU path)")
    from diff_gaussian_rasterization import multiview
    from fused_ssim import fused_l1_ssim_loss, fused_ssim

    dev = torch.device("cuda", 0)
    V, H, W, P, lam = args.views, args.height, args.width, args.points, args.lambda_dssim

    def side(r, nbytes, of="fused"):
        out = {}
        for k, (med, spread, rounds) in r.items():
            out[k] = {"median_ms": med, "spread_ms": spread, "round_medians_ms": rounds}
        out[of]["algorithmic_bytes"] = nbytes
        out[of]["algorithmic_GBps"] = nbytes / (r[of][0] * 1e-3) / 1e9
        noise = max(r["torch"][1], r["fused"][1])
        out["fused_faster_beyond_spread"] = bool(r["torch"][0] - r["fused"][0] > noise)
        out["speedup"] = r["torch"][0] / r["fused"][0]
        return out

    result = {}
    if os.path.exists(args.out):  # legs not run now keep their blocks
        with open(args.out) as f:
            result = json.load(f)
    result.update({
        "tool": "tools/train_tail_bench.py", "device": torch.cuda.get_device_name(dev),
        "views": V, "width": W, "height": H, "points": P, "lambda_dssim": lam, "seed": 0,
        "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
        "timing": "device events around each call, synchronised; sides alternate call by call"})
    if legs & {"loss", "stats"}:
        loss_stats_legs(args, legs, result, side, torch, multiview, fused_l1_ssim_loss, fused_ssim, dev)
    if "view_loss" in legs:
        result["view_loss"] = view_loss_leg(args, side, torch, multiview, dev)
    if "densify" in legs:
        result["densify"] = densify_leg(args, side, torch, multiview, dev)
    if "activations" in legs:
        result["activations"] = activations_leg(args, side, torch, dev)
    if "iteration" in legs:
        result["iteration"] = iteration_leg(args, side, torch, fused_l1_ssim_loss, fused_ssim, dev)
    if "compact" in legs:
        result["compact"] = compact_leg(args, torch, multiview, dev)
    if "camera" in legs:
        result["camera_grads"] = camera_leg(args, torch, dev)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


def loss_stats_legs(args, legs, result, side, torch, multiview, fused_l1_ssim_loss, fused_ssim, dev):
    V, H, W, P, lam = args.views, args.height, args.width, args.points, args.lambda_dssim
    g = torch.Generator(device="cpu").manual_seed(0)
    img = (1.4 * torch.rand((V, 3, H, W), generator=g) - 0.2).to(dev).requires_grad_(True)
    gts = [torch.rand((3, H, W), generator=g).to(dev) for _ in range(V)]  # separate tensors, as the trainer's
    grads = (1e-3 * torch.randn((V, P, 3), generator=g)).to(dev)
    radii = torch.randint(0, 40, (V, P), generator=g, dtype=torch.int32)
    radii[torch.rand((V, P), generator=g) < 0.5] = 0
    radii = radii.to(dev)

    def torch_loss():
        img.grad = None
        losses = []
        for j in range(V):
            x = img[j].clamp(0, 1)
            l1 = (x - gts[j]).abs().mean()
            losses.append((1.0 - lam) * l1 + lam * (1.0 - fused_ssim(x[None], gts[j][None])))
        torch.stack(losses).sum().backward()
        return losses

    def fused_loss():
        img.grad = None
        losses = fused_l1_ssim_loss(img, gts, lam, clamp=True)
        losses.sum().backward()
        return losses

    stats = {k: multiview.densification_stats(P, dev) for k in ("torch", "fused")}
    counts = {k: torch.zeros((P,), device=dev) for k in stats}

    def torch_stats():
        for j in range(V):
            multiview.add_view_stats(stats["torch"], grads[j], radii[j])
            counts["torch"] += (radii[j] > 0).to(torch.float32)

    def fused_stats():
        multiview.add_batch_stats(stats["fused"], grads, radii, counts["fused"])

    # the two sides on these inputs (before any timing)
    agreement = result.setdefault("agreement", {})
    if "loss" in legs:
        lt = torch.stack([l.detach() for l in torch_loss()])
        gt_ = img.grad.clone()
        lf = fused_loss().detach()
        gf = img.grad.clone()
        agreement["loss_max_abs_diff"] = float((lt - lf).abs().max())
        agreement["grad_max_abs_diff_over_max"] = float((gt_ - gf).abs().max() / gt_.abs().max())
        del gt_, gf
        loss = alternate({"torch": torch_loss, "fused": fused_loss}, args.warmup, args.reps, args.rounds, torch)
        # forward: img, gt in, 3 partial planes out; backward: 3 planes, img, gt in, dL/dimg out
        result["loss"] = side(loss, 11 * 4 * V * 3 * H * W)
    if "stats" in legs:
        torch_stats()
        fused_stats()
        agreement["stats_counts_equal"] = bool(
            torch.equal(stats["torch"]["denom"], stats["fused"]["denom"]) and
            torch.equal(stats["torch"]["max_radii2D"], stats["fused"]["max_radii2D"]) and
            torch.equal(counts["torch"], counts["fused"]))
        agreement["accum_max_rel_diff"] = float(
            ((stats["torch"]["xyz_gradient_accum"] - stats["fused"]["xyz_gradient_accum"]).abs()
             / stats["torch"]["xyz_gradient_accum"].abs().clamp_min(1e-30)).max())
        stat = alternate({"torch": torch_stats, "fused": fused_stats}, args.warmup, args.reps, args.rounds, torch)
        # radii and (gx, gy) of every (view, Gaussian); accum, denom, max radius and count read and written
        result["stats"] = side(stat, V * P * 12 + P * 32)


def view_loss_leg(args, side, torch, multiview, dev):
    """The trainer's torch chain for exposure, clamp, mask, loss and depth term against fused_view_loss
    (see the module docstring)."""
    V, H, W, lam, weight = args.views, args.height, args.width, args.lambda_dssim, 0.5
    g = torch.Generator(device="cpu").manual_seed(0)
    img = (1.4 * torch.rand((V, 3, H, W), generator=g) - 0.2).to(dev).requires_grad_(True)
    inv = (0.1 + torch.rand((V, 1, H, W), generator=g)).to(dev).requires_grad_(True)
    exposures = torch.eye(3, 4)[None].repeat(V, 1, 1) + 0.05 * torch.randn((V, 3, 4), generator=g)
    views = []
    for j in range(V):  # separate tensors per view, as the trainer's
        keep = torch.rand((1, H, W), generator=g) >= 0.3
        extras = {"cam": j,
                  "alpha_mask": (keep * (0.25 + 0.75 * torch.rand((1, H, W), generator=g))).to(dev),
                  "invdepth": (0.1 + torch.rand((1, H, W), generator=g)).to(dev),
                  "depth_mask": (torch.rand((1, H, W), generator=g) > 0.2).float().to(dev)}
        views.append((None, torch.rand((3, H, W), generator=g).to(dev), extras))
    names = multiview.TRAIN_GROUPS
    tiny = {"xyz": torch.zeros((1, 3)), "f_dc": torch.zeros((1, 1, 3)), "f_rest": torch.zeros((1, 15, 3)),
            "opacity": torch.zeros((1, 1)), "scaling": torch.zeros((1, 3)), "rotation": torch.ones((1, 4))}
    tr = multiview.DataParallelTrainer({n: tiny[n].to(dev) for n in names}, lambda_dssim=lam, exposures=exposures)

    def reset():
        img.grad = None
        inv.grad = None
        tr.zero_grad()  # the exposure gradients live in the trainer's flat buffer

    def torch_chain():
        reset()
        losses = [tr._view_loss(tr._expose(img[j], j).clamp(0, 1), inv[j], v, weight) for j, v in enumerate(views)]
        torch.stack(losses).sum().backward()
        return losses

    def fused():
        reset()
        losses = tr._fused_view_losses(img, inv, views, weight)
        torch.stack(losses).sum().backward()
        return losses

    # the two sides on these inputs (before any timing)
    out = {}
    for k, fn in (("torch", torch_chain), ("fused", fused)):
        losses = torch.stack([l.detach() for l in fn()])
        out[k] = (losses, img.grad.clone(), tr.exposures.grad.clone(), inv.grad.clone())

    def rel(i):
        return float((out["torch"][i] - out["fused"][i]).abs().max() / out["torch"][i].abs().max())
    agreement = {"loss_max_abs_diff": float((out["torch"][0] - out["fused"][0]).abs().max()),
                 "dL_draw_max_abs_diff_over_max": rel(1), "dL_dexposure_max_abs_diff_over_max": rel(2),
                 "dL_dinvdepth_max_abs_diff_over_max": rel(3)}
    del out
    r = alternate({"torch": torch_chain, "fused": fused}, args.warmup, args.reps, args.rounds, torch)
    res = side(r, 42 * 4 * V * H * W)
    res["byte_model"] = ("per pixel and view, in floats: forward 3 raw + 3 gt + mask in, 9 partial planes out, "
                         "inverse depth + target + depth mask in (19); backward 9 planes + 3 raw + 3 gt + mask in, "
                         "3 out, inverse depth + target + depth mask in, 1 out (23)")
    res["scene"] = "every view with an exposure, an alpha mask (about 30 % zero) and a depth target with a depth mask"
    res["depth_weight"] = weight
    res["agreement"] = agreement
    return res


def densify_leg(args, side, torch, multiview, dev):
    """The torch densify_and_prune against the fused one (see the module docstring)."""
    P, N, pd = args.points, 2, 0.01
    names = multiview.TRAIN_GROUPS
    g = torch.Generator(device="cpu").manual_seed(0)
    start = {"xyz": torch.randn((P, 3), generator=g), "f_dc": torch.randn((P, 1, 3), generator=g),
             "f_rest": 0.1 * torch.randn((P, 15, 3), generator=g), "opacity": 2.0 * torch.randn((P, 1), generator=g),
             "scaling": torch.log(0.003 + 0.02 * torch.rand((P, 3), generator=g)),
             "rotation": torch.randn((P, 4), generator=g)}
    start = {k: v.to(dev) for k, v in start.items()}
    moments = {k: (torch.randn(v.shape, generator=g).to(dev), torch.rand(v.shape, generator=g).to(dev))
               for k, v in start.items()}
    stats = multiview.densification_stats(P, dev)
    stats["xyz_gradient_accum"].copy_((2e-3 * torch.rand((P, 1), generator=g)).to(dev))
    stats["denom"].copy_(torch.randint(1, 9, (P, 1), generator=g).float().to(dev))
    # thresholds: the hottest 10 % of the rows, half of them small (clone) and half large (split);
    # the 5 % most transparent rows are pruned.  No world-size test (max_screen_size None).
    grad = (stats["xyz_gradient_accum"] / stats["denom"]).squeeze(1)
    smax = start["scaling"].exp().max(dim=1).values
    sig = torch.sigmoid(start["opacity"]).squeeze(1)
    def clear(values, thr, window=1e-6):
        """thr raised until no value is within `window` (relative; a few fp32 ulps: torch's exp and
        sigmoid and the kernel's may round differently) of it, so both sides decide alike."""
        for _ in range(10000):
            if not bool(((values.double() / thr - 1.0).abs() < window).any()):
                break
            thr *= 1.0 + 3.0 * window
        return thr
    max_grad = clear(grad, float(torch.quantile(grad[::8], 0.9)))
    hot = grad >= max_grad
    extent = clear(smax, float(smax[hot].median())) / pd
    min_opacity = clear(sig, float(torch.quantile(sig[::8], 0.05)))
    clone, split, low = hot & (smax <= pd * extent), hot & (smax > pd * extent), sig < min_opacity
    n_ko, n_kc, n_ks = int((~split & ~low).sum()), int((clone & ~low).sum()), int((split & ~low).sum())
    P_after = n_ko + n_kc + N * n_ks

    trainers = {k: multiview.DataParallelTrainer({n: start[n][:1] for n in names}, fused_densify=(k == "fused"))
                for k in ("torch", "fused")}
    step = torch.tensor(1.0)

    def fresh():
        T = {n: start[n].clone() for n in names}
        S = {n: {"step": step, "exp_avg": moments[n][0].clone(), "exp_avg_sq": moments[n][1].clone()} for n in names}
        return T, S

    def reset(k):  # outside the timed region: both sides replace their inputs
        trainers[k]._install(*fresh())

    did = {}

    def run(k):
        def fn():
            did[k] = trainers[k].densify_and_prune(max_grad, min_opacity, extent, None, stats=stats, N=N)
        return fn

    held = {}

    def fused_call():
        T, S = held.pop("in")
        held["out"] = multiview.fused_densify_and_prune(T, S, stats, max_grad, min_opacity, extent, None, pd, N,
                                                        trainers["fused"].gen)

    # agreement of the two sides on these inputs, from equal generator states
    out = {}
    for k in ("torch", "fused"):
        trainers[k].gen.manual_seed(0)
        reset(k)
        run(k)()
        tr = trainers[k]
        out[k] = ({n: p.detach() for n, p in tr.params.items()},
                  {n: tr.optimizer.state[p] for n, p in tr.params.items()})
    first_child = P_after - N * n_ks
    copied_equal = did["torch"] == did["fused"] and did["fused"]["P_after"] == P_after
    for n in names:
        rows = first_child if n in ("xyz", "scaling") else P_after
        copied_equal = copied_equal and torch.equal(out["torch"][0][n][:rows], out["fused"][0][n][:rows])
        for m in ("exp_avg", "exp_avg_sq"):
            copied_equal = copied_equal and torch.equal(out["torch"][1][n][m], out["fused"][1][n][m])
    agreement = {
        "counts": did["fused"], "counts_equal": did["torch"] == did["fused"],
        "copied_rows_and_moments_bit_equal": bool(copied_equal),
        "generator_state_equal": bool(torch.equal(trainers["torch"].gen.get_state(),
                                                  trainers["fused"].gen.get_state())),
        "children_xyz_max_abs_diff": float((out["torch"][0]["xyz"][first_child:]
                                            - out["fused"][0]["xyz"][first_child:]).abs().max()),
        "children_scaling_max_abs_diff": float((out["torch"][0]["scaling"][first_child:]
                                                - out["fused"][0]["scaling"][first_child:]).abs().max()),
    }
    del out

    # timing: alternate() with the untimed reset before every timed call
    def timed_after(prepare, fn):
        def call():
            prepare()
            torch.cuda.synchronize()
            return fn
        return call
    sides = {"torch": timed_after(lambda: reset("torch"), run("torch")),
             "fused": timed_after(lambda: reset("fused"), run("fused")),
             "fused_call": timed_after(lambda: held.__setitem__("in", fresh()), fused_call)}
    r = alternate_prepared(sides, args.warmup, args.reps, args.rounds, torch)
    # plan: 24 B in and 1 B out per row, 1 B in again, the three lists written; apply: the lists read,
    # 236 B x (parameter + two moments) written per output row, the same read for kept originals, the
    # parameters alone read for clones and children, 12 B of samples per child
    lists = 4 * (n_ko + n_kc) + 8 * n_ks
    nbytes = 26 * P + 2 * lists + 3 * 236 * P_after + 3 * 236 * n_ko + 236 * (P_after - n_ko) + 12 * N * n_ks
    res = side(r, nbytes, of="fused_call")
    res["fractions"] = {"cloned": float(clone.sum()) / P, "split": float(split.sum()) / P,
                        "pruned_rows": float(low.sum()) / P}
    res["thresholds"] = {"max_grad": max_grad, "min_opacity": min_opacity, "extent": extent, "percent_dense": pd,
                         "N": N, "max_screen_size": None}
    res["includes"] = ("torch and fused: densify_and_prune with the rebuild of the flat gradient buffer both share; "
                       "fused_call: fused_densify_and_prune alone (plan, read-back, randn, allocation, apply)")
    res["agreement"] = agreement
    return res


def activations_leg(args, side, torch, dev):
    """The torch activation chain against fused_activations (see the module docstring)."""
    import diff_gaussian_rasterization as dgr
    F = torch.nn.functional
    P = args.points
    g = torch.Generator(device="cpu").manual_seed(0)
    start = {"scaling": torch.log(0.003 + 0.02 * torch.rand((P, 3), generator=g)),
             "rotation": torch.randn((P, 4), generator=g), "opacity": 2.0 * torch.randn((P, 1), generator=g)}
    names = ("scaling", "rotation", "opacity")
    gout = [torch.randn(start[k].shape, generator=g).to(dev) for k in names]
    fill = torch.randn((8 * P,), generator=g).to(dev)  # what the gradient views hold before every comparison
    raw, flat = {}, {}
    for k in ("torch", "fused"):  # each side's leaves, their .grad views of that side's flat buffer
        flat[k] = fill.clone()
        raw[k], off = [], 0
        for n in names:
            t = start[n].to(dev).requires_grad_(True)
            t.grad = flat[k][off:off + t.numel()].view_as(t)
            off += t.numel()
            raw[k].append(t)

    def torch_chain():
        s, r, o = raw["torch"]
        torch.autograd.backward((torch.exp(s), F.normalize(r), torch.sigmoid(o)), gout)

    def fused():
        with dgr.accumulate_grads_in_place():
            out = dgr.fused_activations(*raw["fused"])
        torch.autograd.backward(out, gout)

    # agreement on these inputs (before any timing): the outputs, and what one backward added
    with torch.no_grad():
        a = (torch.exp(raw["torch"][0]), F.normalize(raw["torch"][1]), torch.sigmoid(raw["torch"][2]))
        b = dgr.fused_activations(*raw["fused"])
    torch_chain()
    fused()
    torch.cuda.synchronize()
    agreement = {}
    for j, n in enumerate(("scales", "rotations", "opacities")):
        agreement[n + "_max_abs_diff"] = float((a[j] - b[j]).abs().max())
        agreement[n + "_max_rel_diff"] = float(((a[j] - b[j]).abs() / a[j].abs().clamp_min(1e-30)).max())
    off = 0
    for j, n in enumerate(names):
        k = raw["torch"][j].numel()
        da, db, before = flat["torch"][off:off + k], flat["fused"][off:off + k], fill[off:off + k]
        agreement["dL_d" + n + "_max_abs_diff_over_max"] = float((da - db).abs().max() / (da - before).abs().max())
        off += k
    agreement["grads_stay_views_of_the_flat_buffer"] = all(
        t.grad.data_ptr() == flat[k][sum(x.numel() for x in raw[k][:j]):].data_ptr()
        for k in raw for j, t in enumerate(raw[k]))
    del a, b
    r = alternate({"torch": torch_chain, "fused": fused}, args.warmup, args.reps, args.rounds, torch)
    res = side(r, (64 + 128) * P)
    res["byte_model"] = "64 B/Gaussian forward (32 in, 32 out) + 128 B/Gaussian backward with accumulation (64 in, 32 in and out)"
    res["agreement"] = agreement
    return res


def iteration_leg(args, side, torch, fused_l1_ssim_loss, fused_ssim, dev):
    """bench.py's aux_train_iteration in its torch form and in the all-HIP form (see the module
    docstring): ms per iteration, wall clock."""
    import time

    import diff_gaussian_rasterization as dgr
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import synthetic  # the bench's scene and camera
    F = torch.nn.functional
    P, H, W = args.points, args.height, args.width
    scene = {k: v.to(dev) for k, v in synthetic.make_scene(P, seed=0).items()}
    cam = synthetic.Camera(W, H, view=0)
    s = dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
        scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev), projmatrix=cam.full_proj_transform.to(dev),
        sh_degree=3, campos=cam.camera_center.to(dev), prefiltered=False, debug=False, antialiasing=False)
    rast = dgr.GaussianRasterizer(raster_settings=s)
    lr = {"xyz": 1.6e-4, "f_dc": 2.5e-3, "f_rest": 2.5e-3 / 20, "opacity": 2.5e-2, "scaling": 5e-3, "rotation": 1e-3}

    def make(fused):
        sh = scene["shs"]
        raw = {"xyz": scene["means3D"].clone(), "f_dc": sh[:, :1].contiguous(), "f_rest": sh[:, 1:].contiguous(),
               "opacity": torch.logit(scene["opacities"]), "scaling": torch.log(scene["scales"]),
               "rotation": scene["rotations"].clone()}
        raw = {k: torch.nn.Parameter(v) for k, v in raw.items()}
        opt = dgr.SparseGaussianAdam([{"params": [p], "lr": lr[k], "name": k} for k, p in raw.items()], lr=0.0,
                                     eps=1e-15)

        def render():
            means2D = torch.zeros_like(raw["xyz"], requires_grad=True)
            if fused:
                scales, rotations, opacities = dgr.fused_activations(raw["scaling"], raw["rotation"], raw["opacity"])
            else:
                scales, rotations, opacities = (torch.exp(raw["scaling"]), F.normalize(raw["rotation"]),
                                                torch.sigmoid(raw["opacity"]))
            return rast(means3D=raw["xyz"], means2D=means2D, dc=raw["f_dc"], shs=raw["f_rest"], opacities=opacities,
                        scales=scales, rotations=rotations)

        def iteration(gt):
            img, radii, _ = render()
            if fused:
                loss = fused_l1_ssim_loss(img[None], [gt], 0.2)[0]
            else:
                loss = 0.8 * (img - gt).abs().mean() + 0.2 * (1.0 - fused_ssim(img[None], gt[None]))
            loss.backward()
            opt.step(radii > 0, P)
            opt.zero_grad(set_to_none=True)
            return loss.detach()
        return render, iteration, raw

    sides = {"torch": make(False), "fused": make(True)}
    with torch.no_grad():
        g = torch.Generator(device="cpu").manual_seed(0)
        gt = (sides["torch"][0]()[0] + 0.05 * torch.randn((3, H, W), generator=g).to(dev)).clamp(0, 1)
    first = {k: float(sides[k][1](gt)) for k in sides}  # the first iteration: from equal parameters
    for _ in range(max(0, args.warmup - 1)):
        for k in sides:
            sides[k][1](gt)

    def group(k):
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(args.group):
            sides[k][1](gt)
        torch.cuda.synchronize()
        return (time.perf_counter() - t) / args.group * 1e3
    meds = {k: [] for k in sides}
    for _ in range(args.rounds):
        t = {k: [] for k in sides}
        for _ in range(args.reps):
            for k in sides:
                t[k].append(group(k))
        for k in sides:
            meds[k].append(statistics.median(t[k]))
    r = {k: (statistics.median(m), max(m) - min(m), m) for k, m in meds.items()}
    out = {}
    for k, (med, spread, rounds) in r.items():
        out[k] = {"median_ms_per_iteration": med, "spread_ms": spread, "round_medians_ms": rounds}
    out["fused_faster_beyond_spread"] = bool(r["torch"][0] - r["fused"][0] > max(r["torch"][1], r["fused"][1]))
    out["speedup"] = r["torch"][0] / r["fused"][0]
    out["gaussians"], out["resolution"], out["iterations_per_group"] = P, [W, H], args.group
    out["timing"] = ("time.perf_counter() around synchronised groups of iterations, the sides alternating group "
                     "by group; torch: torch activations, torch L1 + fused_ssim; fused: fused_activations, "
                     "fused_l1_ssim_loss (V = 1); both: GaussianRasterizer with dc=, SparseGaussianAdam.step")
    out["agreement"] = {"first_iteration_loss_torch": first["torch"], "first_iteration_loss_fused": first["fused"],
                        "first_iteration_loss_abs_diff": abs(first["torch"] - first["fused"])}
    return out


def _radii_union(torch, dgr, scene, cams, W, H, dev, subsets):
    """U / P of the union of the views' radii > 0 for each subset of `cams` (objects with the
    synthetic.Camera fields), from real forward passes."""
    sc = {k: v.to(dev) for k, v in scene.items()}
    P = sc["means3D"].shape[0]
    seen = []
    with torch.no_grad():
        for c in cams:
            s = dgr.GaussianRasterizationSettings(
                image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=torch.zeros(3, device=dev),
                scale_modifier=1.0, viewmatrix=c.world_view_transform.to(dev),
                projmatrix=c.full_proj_transform.to(dev), sh_degree=3, campos=c.camera_center.to(dev),
                prefiltered=False, debug=False, antialiasing=False)
            radii = dgr.GaussianRasterizer(raster_settings=s)(
                means3D=sc["means3D"], means2D=torch.zeros_like(sc["means3D"]), shs=sc["shs"],
                opacities=sc["opacities"], scales=sc["scales"], rotations=sc["rotations"])[1]
            seen.append(radii > 0)
    out = {"points": P, "resolution": [W, H], "per_view": [float(m.sum()) / P for m in seen]}
    for name, idx in subsets.items():
        out[name] = float(torch.stack([seen[i] for i in idx]).any(dim=0).sum()) / P
    return out, torch.stack(seen).any(dim=0)


def compact_leg(args, torch, multiview, dev):
    """pack + plan, gather and scatter against a clone of the buffer, and the union fractions of the
    repository's scenes (see the module docstring).  One GPU, no collective."""
    import numpy as np

    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    for p in (ROOT, os.path.join(ROOT, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import nerf_synthetic as ns
    import synthetic
    P, H, W = args.points, args.height, args.width
    Ms = (3, 3, 45, 1, 3, 4, 1)
    M = sum(Ms)

    # union fractions of the scenes at hand
    class Cam:
        def __init__(self, f, i):
            self.world_view_transform = torch.from_numpy(f["train_viewmatrix"][i].copy())
            self.full_proj_transform = torch.from_numpy(f["train_projmatrix"][i].copy())
            self.camera_center = torch.from_numpy(f["train_campos"][i].copy())
            self.tanfovx, self.tanfovy = float(f["train_tanfov"][i][0]), float(f["train_tanfov"][i][1])
    ring8 = {"views_0_3": [0, 1, 2, 3], "views_4_7": [4, 5, 6, 7], "all_8_views": list(range(8))}
    unions = {}
    spread = synthetic.make_scene(2000, seed=0)
    spread["means3D"] = spread["means3D"] * 3.0
    unions["trainer_test_scene_spread_3"], _ = _radii_union(
        torch, dgr, spread, [synthetic.Camera(128, 96, view=v) for v in range(8)], 128, 96, dev, ring8)
    unions["trainer_test_scene_spread_1"], _ = _radii_union(
        torch, dgr, synthetic.make_scene(2000, seed=0), [synthetic.Camera(128, 96, view=v) for v in range(8)], 128,
        96, dev, ring8)
    golden = os.path.join(ROOT, "tests", "golden", "chair")
    f, fr = dict(np.load(os.path.join(golden, "nerf_chair.npz"))), dict(np.load(os.path.join(golden, "chair_frames.npz")))
    chair = ns.initial_gaussians(f["xyz"], f["rgb"], f["dist2"], scale=f["scale"], opacity=f["opacity"])
    unions["chair_fixture_train_cameras"], _ = _radii_union(
        torch, dgr, chair, [Cam(fr, i) for i in range(8)], 800, 800, dev,
        {"views_0_3": [0, 1, 2, 3], "all_8_views": list(range(8))})
    unions["config3_scale_cloud"], _ = _radii_union(
        torch, dgr, synthetic.make_scene(6_000_000, seed=0), [synthetic.Camera(1297, 840, view=v) for v in range(8)],
        1297, 840, dev, {"views_0_3": [0, 1, 2, 3], "all_8_views": list(range(8))})
    torch.cuda.empty_cache()
    bench_union, bench_mask = _radii_union(
        torch, dgr, synthetic.make_scene(P, seed=0), [synthetic.Camera(W, H, view=v) for v in range(8)], W, H, dev,
        {"all_8_views": list(range(8))})
    unions["bench_scene"] = bench_union
    torch.cuda.empty_cache()

    g = torch.Generator(device="cpu").manual_seed(0)
    flat = torch.randn((P * M,), generator=g).to(dev)
    groups, off = [], 0
    for m in Ms:
        groups.append(flat[off:off + P * m].view(P, m))
        off += P * m
    masks = {f"random_{q}": (torch.rand((P,), generator=g) < q).to(dev) for q in (0.25, 0.5, 0.75)}
    masks["random_1.0"] = torch.ones((P,), dtype=torch.bool, device=dev)
    masks["bench_scene_8_views"] = bench_mask
    words = torch.empty((1, _C.visibility_words(P)), dtype=torch.int32, device=dev)
    rows = torch.empty((P,), dtype=torch.int32, device=dev)
    mask_out = torch.empty((P,), dtype=torch.bool, device=dev)
    ws = torch.empty((int(_C.lib.gsr_union_workspace_size(P)),), dtype=torch.uint8, device=dev)
    compact = torch.empty((P * M,), device=dev)
    out = {"groups": list(Ms), "floats_per_row": M, "points": P,
           "note": "one GPU, no collective: nothing here was timed on more than one GPU", "masks": {}}
    held = {}
    for name, mask in masks.items():
        count = mask.to(torch.float32)

        def pack_plan():
            _C.visibility_pack(count, out=words[0])
            held["U"] = _C.union_plan(words, P, rows=rows, mask=mask_out, workspace=ws)[0]
        pack_plan()
        U = held["U"]
        assert U == int(mask.sum()) and torch.equal(mask_out, mask)
        sides = {"clone": lambda: held.__setitem__("c", flat.clone()), "pack_plan": pack_plan,
                 "gather": lambda: _C.rows_gather(groups, rows, U, compact),
                 "scatter": lambda: _C.rows_scatter(groups, rows, U, compact)}
        # gather then scatter puts back what it took: the buffer stays as it was
        sides["gather"]()
        before = flat.clone()
        sides["scatter"]()
        assert torch.equal(before.view(torch.int32), flat.view(torch.int32))
        del before
        r = alternate(sides, args.warmup, args.reps, args.rounds, torch)
        nbytes = {"clone": 2 * 4 * M * P, "pack_plan": 4 * P + 3 * (P // 8) + P + 4 * U,
                  "gather": (4 + 8 * M) * U, "scatter": (4 + 8 * M) * U}
        block = {"U": U, "union_fraction": U / P}
        for k, (med, spread_ms, rounds) in r.items():
            block[k] = {"median_ms": med, "spread_ms": spread_ms, "round_medians_ms": rounds,
                        "algorithmic_bytes": nbytes[k], "algorithmic_GBps": nbytes[k] / (med * 1e-3) / 1e9}
        out["masks"][name] = block
    # compact_below from the measured copies (random_0.5) and DESIGN.md §8's ASSUMED link rate
    half = out["masks"]["random_0.5"]
    per_row_s = (half["gather"]["median_ms"] + half["scatter"]["median_ms"]) * 1e-3 / half["U"]
    fixed_s = half["pack_plan"]["median_ms"] * 1e-3
    bus = {2: 55.0, 4: 150.0, 8: 330.0}  # DESIGN.md §8's ASSUMED RCCL bus rates over xGMI, GB/s
    derived = {"assumed_bus_GBps": {str(k): v for k, v in bus.items()}, "dense_bytes_per_row": 4 * M,
               "measured_gather_plus_scatter_s_per_union_row": per_row_s,
               "measured_pack_plan_s": fixed_s, "by_world_size": {}}
    for N in (2, 4, 8):
        link_s = 2.0 * (N - 1) / N * 4 * M / (bus[N] * 1e9)  # link time of one row of the dense all-reduce
        # compaction pays while  f * per_row_s + fixed_s / P  <  (1 - f) * link_s
        f = (link_s - fixed_s / P) / (link_s + per_row_s)
        derived["by_world_size"][str(N)] = {"link_s_per_row": link_s, "break_even_fraction": f,
                                            "rounded_down_to_0.05": int(f / 0.05 + 1e-9) * 0.05}
    derived["note"] = ("break-even union fraction: gather + scatter time per union row (measured, one GPU) against the "
                       "link time saved per row left out (ring factor 2(N-1)/N, bus rates ASSUMED, not measured); "
                       "the shipped default follows N = 8")
    out["compact_below_derivation"] = derived
    out["shipped_compact_below"] = multiview.COMPACT_BELOW
    out["union_fractions"] = unions
    return out


def camera_leg(args, torch, dev):
    """The batched backward without and with cameras=, and the camera kernels' own time beside
    preprocess_bwd's (see the module docstring)."""
    import ctypes

    import diff_gaussian_rasterization as dgr
    from diff_gaussian_rasterization import _C
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import synthetic
    V, P, H, W = args.views, args.points, args.height, args.width
    scene = {k: v.to(dev).requires_grad_(True) for k, v in synthetic.make_scene(P, seed=0).items()}
    cams = [synthetic.Camera(W, H, view=v, n_views=max(V, 8)) for v in range(V)]
    bg = torch.zeros(3, device=dev)
    rast = dgr.MultiViewRasterizer([dgr.GaussianRasterizationSettings(
        image_height=H, image_width=W, tanfovx=c.tanfovx, tanfovy=c.tanfovy, bg=bg, scale_modifier=1.0,
        viewmatrix=c.world_view_transform.to(dev), projmatrix=c.full_proj_transform.to(dev), sh_degree=3,
        campos=c.camera_center.to(dev), prefiltered=False, debug=False, antialiasing=False) for c in cams])
    stacked = tuple(torch.stack([getattr(c, n) for c in cams]).to(dev).contiguous().requires_grad_(True)
                    for n in ("world_view_transform", "full_proj_transform", "camera_center"))
    gc = torch.randn((V, 3, H, W), generator=torch.Generator().manual_seed(1)).to(dev)
    means2D = torch.zeros((V, P, 3), device=dev, requires_grad=True)

    def prepare(with_cameras):
        def prep():
            for t in list(scene.values()) + list(stacked) + [means2D]:
                t.grad = None
            color = rast(means3D=scene["means3D"], means2D=means2D, opacities=scene["opacities"], shs=scene["shs"],
                         scales=scene["scales"], rotations=scene["rotations"],
                         **({"cameras": stacked} if with_cameras else {}))[0]
            return lambda: color.backward(gc)
        return prep

    r = alternate_prepared({"backward": prepare(False), "backward_with_cameras": prepare(True)}, args.warmup,
                           args.reps, args.rounds, torch)
    out = {k: {"median_ms": med, "spread_ms": spread, "round_medians_ms": rounds} for k, (med, spread, rounds) in r.items()}
    out["added_ms"] = r["backward_with_cameras"][0] - r["backward"][0]
    out["added_beyond_spread"] = bool(out["added_ms"] > max(r["backward"][1], r["backward_with_cameras"][1]))
    # the kernels' own time: the library's profile scopes around the launches, cameras= passes only
    lib = _C.lib
    lib.gsr_profile_kernel_name.restype = ctypes.c_char_p
    run = prepare(True)
    run()()  # one pass outside the profile (allocations)
    torch.cuda.synchronize()
    lib.gsr_profile_enable(1)
    for _ in range(args.reps):
        run()()
    torch.cuda.synchronize()
    tot, cnt = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
    n = lib.gsr_profile_read(tot, cnt, 16)
    lib.gsr_profile_enable(0)
    kern = {lib.gsr_profile_kernel_name(k).decode(): {"avg_ms": tot[k] / cnt[k], "launches": cnt[k]}
            for k in range(n) if cnt[k]}
    out["kernels_ms_per_batch"] = {k: kern[k] for k in ("camera_bwd", "preprocess_bwd", "render_bwd") if k in kern}
    if "camera_bwd" in kern and "preprocess_bwd" in kern:
        out["camera_bwd_over_preprocess_bwd"] = kern["camera_bwd"]["avg_ms"] / kern["preprocess_bwd"]["avg_ms"]
    out["visible_per_view"] = [float(x) / P for x in (rast(
        means3D=scene["means3D"].detach(), means2D=means2D.detach(), opacities=scene["opacities"].detach(),
        shs=scene["shs"].detach(), scales=scene["scales"].detach(),
        rotations=scene["rotations"].detach())[1] > 0).sum(1).tolist()]
    out["note"] = ("backward of one MultiViewRasterizer node, forward untimed; camera_bwd covers both camera kernels "
                   "(one scope), the profile scopes include the forward's kernels of the same passes under their own ids")
    return out


def alternate_prepared(sides, warmup, reps, rounds, torch):
    """alternate() for sides that need untimed preparation: side() prepares and returns the call to time."""
    for _ in range(warmup):
        for prep in sides.values():
            timed(prep(), torch)
    meds = {k: [] for k in sides}
    for _ in range(rounds):
        t = {k: [] for k in sides}
        for _ in range(reps):
            for k, prep in sides.items():
                t[k].append(timed(prep(), torch))
        for k in sides:
            meds[k].append(statistics.median(t[k]))
    return {k: (statistics.median(m), max(m) - min(m), m) for k, m in meds.items()}


if __name__ == "__main__":
    main()
