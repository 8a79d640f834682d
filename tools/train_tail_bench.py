#!/usr/bin/env python3
"""Times the tail of a training iteration -- what sits between the rasterizer step and the Adam step
-- in its torch form against its fused HIP form, in ONE process on the GPU:

  loss:   per view clamp, (img - gt).abs().mean(), fused_ssim, the scalar mix, and their backward
          (DataParallelTrainer._view_loss on the clamped image)   vs   one fused_l1_ssim_loss
          call (photo_loss_fwd_kernel + photo_loss_bwd_kernel) and its backward;
  stats:  V x multiview.add_view_stats (boolean-mask indexing, a host synchronisation each)
          vs   one multiview.add_batch_stats launch (densify_stats_kernel).

Defaults are the bench's flagship shape: 8 views, 1920x1080, 1M Gaussians, seed-0 data.  The two
sides alternate call by call; every call is bracketed by device events and ends in a
synchronise.  `--rounds` rounds of `--reps` timed calls per side (after `--warmup` untimed ones)
give one median per round; reported are the median of the round medians and their spread
(max - min).  The result -- times, spreads, the algorithmic bytes of the fused forms (11 floats per
plane-pixel for the loss) and the two sides' agreement on these inputs -- goes to --out as JSON
and to stdout as one line.  Without a GPU it fails.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-npu_amd"))


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_tail.json"))
    args = ap.parse_args()
    if args.warmup < 3 or args.reps < 20:
        ap.error("at least 3 warm-ups and 20 timed repetitions per side")

    import torch
    if not torch.cuda.is_available():
        sys.exit("train_tail_bench: no GPU found (this tool measures on the device; there is no CPU path)")
    from diff_gaussian_rasterization import multiview
    from fused_ssim import fused_l1_ssim_loss, fused_ssim

    dev = torch.device("cuda", 0)
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
    lt = torch.stack([l.detach() for l in torch_loss()])
    gt_ = img.grad.clone()
    lf = fused_loss().detach()
    gf = img.grad.clone()
    torch_stats()
    fused_stats()
    agreement = {
        "loss_max_abs_diff": float((lt - lf).abs().max()),
        "grad_max_abs_diff_over_max": float((gt_ - gf).abs().max() / gt_.abs().max()),
        "stats_counts_equal": bool(torch.equal(stats["torch"]["denom"], stats["fused"]["denom"]) and
                                   torch.equal(stats["torch"]["max_radii2D"], stats["fused"]["max_radii2D"]) and
                                   torch.equal(counts["torch"], counts["fused"])),
        "accum_max_rel_diff": float(((stats["torch"]["xyz_gradient_accum"] - stats["fused"]["xyz_gradient_accum"]).abs()
                                     / stats["torch"]["xyz_gradient_accum"].abs().clamp_min(1e-30)).max()),
    }
    del gt_, gf

    loss = alternate({"torch": torch_loss, "fused": fused_loss}, args.warmup, args.reps, args.rounds, torch)
    stat = alternate({"torch": torch_stats, "fused": fused_stats}, args.warmup, args.reps, args.rounds, torch)

    def side(r, nbytes):
        out = {}
        for k, (med, spread, rounds) in r.items():
            out[k] = {"median_ms": med, "spread_ms": spread, "round_medians_ms": rounds}
        out["fused"]["algorithmic_bytes"] = nbytes
        out["fused"]["algorithmic_GBps"] = nbytes / (r["fused"][0] * 1e-3) / 1e9
        noise = max(r["torch"][1], r["fused"][1])
        out["fused_faster_beyond_spread"] = bool(r["torch"][0] - r["fused"][0] > noise)
        out["speedup"] = r["torch"][0] / r["fused"][0]
        return out

    result = {
        "tool": "tools/train_tail_bench.py", "device": torch.cuda.get_device_name(dev),
        "views": V, "width": W, "height": H, "points": P, "lambda_dssim": lam, "seed": 0,
        "warmup": args.warmup, "reps": args.reps, "rounds": args.rounds,
        "timing": "device events around each call, synchronised; sides alternate call by call",
        # forward: img, gt in, 3 partial planes out; backward: 3 planes, img, gt in, dL/dimg out
        "loss": side(loss, 11 * 4 * V * 3 * H * W),
        # radii and (gx, gy) of every (view, Gaussian); accum, denom, max radius and count read and written
        "stats": side(stat, V * P * 12 + P * 32),
        "agreement": agreement,
    }
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
