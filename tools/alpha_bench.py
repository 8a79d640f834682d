#!/usr/bin/env python3
"""What the alpha output (return_alpha=True) costs on the bench scene, and that it costs the step
without it nothing: writes profiles/alpha_output.json.

The workload is bench.py's default step -- 1M synthetic Gaussians (seed 0), ring views 0..7 at
1920x1080 as ONE MultiViewRasterizer batch, forward + backward under the seeded image gradients --
timed with HIP events around every step (median of --steps steps after --warmup), and the library's
own per-launch events (gsr_profile_enable, a separate instrumented pass as in bench.py) for
render_bwd.  Three legs:

  (a) parent comparison: the step WITHOUT return_alpha on this tree and on a built checkout of the
      parent commit (--parent-root), in fresh processes that alternate parent / this, --runs times
      each, in one session on one machine.  The requirement is no regression: this tree's median
      over its runs must lie inside the parent's observed [min, max] widened on both sides by the
      parent's own spread (max - min).  Every run's value is written down.
  (b) the feature: the same step with return_alpha=True and a gradient on every view's alpha, and
      gsr_alpha_views alone (8 views per launch).
  (c) what it replaces: the same loss from a second MultiViewRasterizer pass with
      colors_precomp = 1 and bg = 0, whose channel 0 is alpha.

(b) and (c) have no target; (b)/(a) and (c)/(a) are reported.  A run without a GPU fails: there is
no fallback and no number.

  python tools/alpha_bench.py --parent-root ../parent-checkout     # built with its own build()
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P, W, H, VIEWS = 1_000_000, 1920, 1080, 8


def parse(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent-root", default="", help="a checkout of the parent commit, built (leg (a)); "
                                                      "without it leg (a) holds this tree's runs only")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3, help="fresh processes per tree, alternating")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "alpha_output.json"))
    ap.add_argument("--timeout", type=int, default=240, help="seconds per measuring process")
    ap.add_argument("--P", type=int, default=P)
    ap.add_argument("--width", type=int, default=W)
    ap.add_argument("--height", type=int, default=H)
    ap.add_argument("--child", default="", choices=("", "plain", "all"), help=argparse.SUPPRESS)
    ap.add_argument("--root", default=ROOT, help=argparse.SUPPRESS)
    args = ap.parse_args(argv)
    if args.steps < 20:
        ap.error("--steps must be at least 20 (a median of fewer steps is not reported)")
    return args


# ---- one measuring process ---------------------------------------------------------------------
def child(args):
    """The legs of one tree in this process: "plain" = the step without alpha (works on the parent);
    "all" = that, the step with alpha, the second-pass step and gsr_alpha_views alone.  Prints one
    JSON line."""
    root = os.path.abspath(args.root)
    sys.path[:0] = [root, os.path.join(root, "gaussian-splatting-npu_amd")]
    import ctypes

    import torch

    import synthetic
    if not torch.cuda.is_available():
        raise SystemExit("alpha_bench: no GPU (HIP device); nothing is measured without one")
    import diff_gaussian_rasterization as dgr
    assert os.path.abspath(dgr.__file__).startswith(root + os.sep), dgr.__file__
    lib = dgr._C.lib
    lib.gsr_profile_read.argtypes = [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.gsr_profile_kernel_name.restype = ctypes.c_char_p
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    Hh, Ww = args.height, args.width

    scene = synthetic.make_scene(args.P, seed=0)
    params = {k: v.to(dev).requires_grad_(True) for k, v in scene.items()}
    cams, gcs, gis, gas = [], [], [], []
    for v in range(VIEWS):
        cam = synthetic.Camera(Ww, Hh, view=v, n_views=VIEWS)
        cams.append(dgr.GaussianRasterizationSettings(
            image_height=Hh, image_width=Ww, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=torch.zeros(3, device=dev),
            scale_modifier=1.0, viewmatrix=cam.world_view_transform.to(dev),
            projmatrix=cam.full_proj_transform.to(dev), sh_degree=3, campos=cam.camera_center.to(dev),
            prefiltered=False, debug=False, antialiasing=False))
        gc, gi = synthetic.make_grads(Hh, Ww, seed=1 + v)
        gcs.append(gc)
        gis.append(gi)
        gas.append(synthetic.make_grads(Hh, Ww, seed=101 + v)[0][:1])
    gc, gi, ga = (torch.stack(x).to(dev) for x in (gcs, gis, gas))
    ga3 = torch.cat([ga, torch.zeros_like(ga), torch.zeros_like(ga)], dim=1)  # dL/d(colour) of the second pass
    ones = torch.ones((args.P, 3), device=dev)
    mv = dgr.MultiViewRasterizer(cams)
    means2D = torch.zeros((VIEWS, args.P, 3), device=dev, requires_grad=True)
    means2D_b = torch.zeros((VIEWS, args.P, 3), device=dev, requires_grad=True)
    geo = dict(means3D=params["means3D"], opacities=params["opacities"], scales=params["scales"],
               rotations=params["rotations"])

    def clear():
        for p in list(params.values()) + [means2D, means2D_b]:
            p.grad = None

    def plain():
        clear()
        color, radii, inv = mv(means2D=means2D, shs=params["shs"], **geo)
        torch.autograd.backward([color, inv], [gc, gi])

    def alpha():
        clear()
        color, radii, inv, a = mv(means2D=means2D, shs=params["shs"], return_alpha=True, **geo)
        torch.autograd.backward([color, inv, a], [gc, gi, ga])

    def second_pass():
        clear()
        color, radii, inv = mv(means2D=means2D, shs=params["shs"], **geo)
        sil, _, _ = mv(means2D=means2D_b, colors_precomp=ones, **geo)
        torch.autograd.backward([color, inv, sil], [gc, gi, ga3])

    def timed(fn):
        """(median step ms over args.steps steps, render_bwd ms per step from an instrumented pass)."""
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
        marks[0].record()
        for i in range(args.steps):
            fn()
            marks[i + 1].record()
        torch.cuda.synchronize()
        ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps)]
        lib.gsr_set_prefix_stream(0)  # one stream: a kernel's duration is its own (as bench.py's pass)
        lib.gsr_profile_enable(1)
        for _ in range(args.steps):
            fn()
        torch.cuda.synchronize()
        lib.gsr_set_prefix_stream(1)
        tot, cnt = (ctypes.c_double * 16)(), (ctypes.c_int * 16)()
        n = lib.gsr_profile_read(tot, cnt, 16)
        lib.gsr_profile_enable(0)
        kern = {lib.gsr_profile_kernel_name(k).decode(): tot[k] / args.steps for k in range(n) if cnt[k]}
        return {"step_ms_median": statistics.median(ms), "step_ms_min": min(ms), "step_ms_max": max(ms),
                "render_bwd_ms_per_step": kern.get("render_bwd"), "render_fwd_ms_per_step": kern.get("render_fwd")}

    out = {"tree": "this" if root == ROOT else "parent", "device": torch.cuda.get_device_name(dev),
           "lib_version": lib.gsr_version().decode(), "steps": args.steps, "warmup": args.warmup,
           "plain": timed(plain)}
    if args.child == "all":
        out["alpha"] = timed(alpha)
        out["second_pass"] = timed(second_pass)
        # gsr_alpha_views alone, on the image states of one batched forward
        e = torch.Tensor([])
        outs = (torch.empty((VIEWS, 3, Hh, Ww), device=dev),
                torch.empty((VIEWS, args.P), dtype=torch.int32, device=dev),
                torch.empty((VIEWS, 1, Hh, Ww), device=dev))
        with torch.no_grad():
            _, _, _, imgs = dgr._C.rasterize_gaussians_views(
                cams[0].bg, params["means3D"], e, params["opacities"], params["scales"], params["rotations"], 1.0, e,
                [s.viewmatrix for s in cams], [s.projmatrix for s in cams], [s.tanfovx for s in cams],
                [s.tanfovy for s in cams], Hh, Ww, params["shs"], 3, [s.campos for s in cams], False, False, False,
                out=outs)
            dst = torch.empty((VIEWS, 1, Hh, Ww), device=dev)
            for _ in range(args.warmup):
                dgr._C.render_alpha(imgs, Hh, Ww, out=dst)
            reps = 5 * args.steps
            marks = [torch.cuda.Event(enable_timing=True) for _ in range(reps + 1)]
            marks[0].record()
            for i in range(reps):
                dgr._C.render_alpha(imgs, Hh, Ww, out=dst)
                marks[i + 1].record()
            torch.cuda.synchronize()
        ms = [marks[i].elapsed_time(marks[i + 1]) for i in range(reps)]
        nbytes = 8 * VIEWS * Hh * Ww  # 4 B read + 4 B written per pixel
        out["alpha_views_alone"] = {"ms_median": statistics.median(ms), "ms_min": min(ms), "calls": reps,
                                    "algorithmic_bytes": nbytes,
                                    "GBps_at_median": nbytes / statistics.median(ms) / 1e6}
    print("ALPHA_BENCH " + json.dumps(out), flush=True)


# ---- the session -------------------------------------------------------------------------------
def run_child(args, root, which):
    """One fresh measuring process on the tree at `root`; its JSON.  A process that fails ends the session."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", which, "--root", root, "--steps", str(args.steps),
           "--warmup", str(args.warmup), "--P", str(args.P), "--width", str(args.width), "--height", str(args.height)]
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=args.timeout, cwd=root)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("ALPHA_BENCH ")]
    if r.returncode != 0 or not lines:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"alpha_bench: the measuring process on {root} failed (status {r.returncode})")
    return json.loads(lines[-1][len("ALPHA_BENCH "):])


def spread_check(parent, this):
    """this' median inside [min(parent) - s, max(parent) + s], s = max(parent) - min(parent)."""
    lo, hi = min(parent), max(parent)
    s = hi - lo
    m = statistics.median(this)
    return {"parent_runs": parent, "this_runs": this, "parent_min": lo, "parent_max": hi, "parent_spread": s,
            "this_median": m, "allowed": [lo - s, hi + s], "inside": bool(lo - s <= m <= hi + s),
            "this_median_over_parent_median": m / statistics.median(parent)}


def main(argv=None):
    args = parse(argv)
    if args.child:
        return child(args)
    parent_root = os.path.abspath(args.parent_root) if args.parent_root else ""
    runs = {"parent": [], "this": []}
    for _ in range(args.runs):  # alternating: parent, this, parent, this, ...
        if parent_root:
            runs["parent"].append(run_child(args, parent_root, "plain"))
        runs["this"].append(run_child(args, ROOT, "all"))
    med = lambda leg, key: [r[leg][key] for r in runs["this"]]  # noqa: E731
    result = {"workload": {"P": args.P, "width": args.width, "height": args.height, "views": VIEWS,
                           "execution": "one MultiViewRasterizer batch, forward + backward, bench.py's seeded inputs"},
              "method": "HIP events around every step, median of `steps` steps after `warmup`; render_bwd from the "
                        "library's per-launch events in a separate instrumented pass; fresh processes, alternating "
                        "parent / this",
              "steps": args.steps, "warmup": args.warmup, "runs_per_tree": args.runs,
              "device": runs["this"][0]["device"], "runs": runs}
    a_step = statistics.median(med("plain", "step_ms_median"))
    if parent_root:
        result["a_parent_comparison"] = {
            key: spread_check([r["plain"][key] for r in runs["parent"]], med("plain", key))
            for key in ("step_ms_median", "render_bwd_ms_per_step")}
        result["a_no_regression"] = all(v["inside"] or v["this_median"] < v["parent_min"]
                                        for v in result["a_parent_comparison"].values())
    b_step = statistics.median(med("alpha", "step_ms_median"))
    c_step = statistics.median(med("second_pass", "step_ms_median"))
    result["b_feature"] = {"step_ms_runs": med("alpha", "step_ms_median"), "step_ms": b_step,
                           "render_bwd_ms_per_step_runs": med("alpha", "render_bwd_ms_per_step"),
                           "alpha_views_alone": [r["alpha_views_alone"] for r in runs["this"]],
                           "b_over_a": b_step / a_step}
    result["c_second_pass"] = {"step_ms_runs": med("second_pass", "step_ms_median"), "step_ms": c_step,
                               "c_over_a": c_step / a_step}
    result["a_step_ms"] = a_step
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: result[k] for k in result if k not in ("runs", "method", "workload")}, indent=1))


if __name__ == "__main__":
    main()
