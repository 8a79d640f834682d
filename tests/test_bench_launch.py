"""bench.py --gpus N launches N ranks itself (the driver's scaling command is `python bench.py
--gpus N`): one torch.distributed.run child, one rank per GPU, never a re-exec.
CPU only: the ranks run with --rank-probe, which reports the rank environment and exits before
anything touches a GPU."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _env(**kw):
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "LOCAL_WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    env.update(kw)
    return env


def test_rank_launch_cmd():
    import bench
    argv = ["--gpus", "4", "--steps", "7"]
    args = bench.parse(argv)
    cmd = bench.rank_launch_cmd(args, argv, 29555, pmc_file="/tmp/x.json")
    i = cmd.index("torch.distributed.run")
    assert cmd[i - 1] == "-m" and "--nproc-per-node=4" in cmd and "--nnodes=1" in cmd
    assert cmd[cmd.index("--master-addr") + 1] == "127.0.0.1" and cmd[cmd.index("--master-port") + 1] == "29555"
    script = cmd.index(os.path.join(ROOT, "bench.py"))
    assert cmd[script + 1:] == argv + ["--pmc-file", "/tmp/x.json"]
    # no PMC figures: the ranks must not run their own PMC passes
    assert bench.rank_launch_cmd(args, argv, 1)[-1] == "--no-pmc"


def test_gpus2_spawns_two_ranks():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rank-probe", "--steps", "3"],
                       cwd=ROOT, env=_env(GSR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert sorted(d["rank"] for d in lines) == [0, 1]
    assert all(d["world"] == 2 for d in lines)
    assert sorted(d["local_rank"] for d in lines) == [0, 1]
    # every rank got the launcher's arguments (and no PMC passes of its own)
    assert all(d["argv"][:5] == ["--gpus", "2", "--rank-probe", "--steps", "3"] and "--no-pmc" in d["argv"]
               for d in lines)


@pytest.mark.parametrize("mode", ["strong", "weak"])
def test_gpus2_views_per_mode(mode):
    """Both modes the driver may run at N = 2: strong scaling (the default: config 4's fixed batch of
    8 views, 4 per rank) and weak scaling (--views-per-rank 8: 8 distinct views per rank, 16 per
    step).  The ranks' views are disjoint and cover the step."""
    extra = ["--views-per-rank", "8"] if mode == "weak" else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rank-probe"] + extra,
                       cwd=ROOT, env=_env(GSR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = sorted((json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")), key=lambda d: d["rank"])
    assert [d["rank"] for d in lines] == [0, 1] and all(d["scaling"] == mode for d in lines)
    views = [v for d in lines for v in d["views"]]
    assert len(views) == len(set(views)) == lines[0]["views_step"]
    if mode == "weak":
        assert all(len(d["views"]) == 8 for d in lines) and lines[0]["views_step"] == 16
        assert lines[0]["n_ring"] == 16 and sorted(views) == list(range(16))
    else:
        assert all(len(d["views"]) == 4 for d in lines) and sorted(views) == list(range(8))


def test_world_size_mismatch_fails():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--rank-probe"],
                       cwd=ROOT, env=_env(WORLD_SIZE="2", RANK="0"), capture_output=True, text=True, timeout=120)
    assert r.returncode != 0 and "WORLD_SIZE=2" in r.stderr


@pytest.mark.skipif(os.environ.get("GSR_DIST_BACKEND", "nccl") != "nccl", reason="default backend overridden")
def test_rccl_needs_enough_gpus():
    import torch
    if torch.cuda.device_count() >= 2:
        pytest.skip("this host has the GPUs")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rank-probe"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=120)
    assert r.returncode == 2 and "needs 2 GPUs" in r.stderr


def test_dump_outputs_writes_fixed_float32_sample(tmp_path, monkeypatch):
    """--dump-outputs: every array as <name>.npy, flat float32; above DUMP_SAMPLE elements the same
    seeded sample in every run; an absent array (None) is skipped."""
    import numpy as np
    import torch
    import bench
    monkeypatch.setattr(bench, "DUMP_SAMPLE", 100)
    big = torch.arange(3 * 7 * 11, dtype=torch.float32).reshape(3, 7, 11)
    arrays = {"color": big, "radii": torch.arange(10, dtype=torch.int32), "grad_means2D": None,
              "grad_shs": -big.double()}
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), arrays)
    a = {n: np.load(tmp_path / "a" / (n + ".npy")) for n in ("color", "radii", "grad_shs")}
    assert sorted(os.listdir(tmp_path / "a")) == ["color.npy", "grad_shs.npy", "radii.npy"]
    assert all(v.dtype == np.float32 and v.ndim == 1 for v in a.values())
    assert np.array_equal(a["radii"], np.arange(10)) and a["color"].size == a["grad_shs"].size == 100
    # the sampled values are elements of the array (an arange: each value is its own flat index)
    assert (a["color"] == np.round(a["color"])).all() and a["color"].min() >= 0 and a["color"].max() < big.numel()
    assert len(set(a["color"].tolist())) > 50 and (a["grad_shs"] <= 0).all()
    for n, v in a.items():
        assert np.array_equal(v, np.load(tmp_path / "b" / (n + ".npy")))


SMALL = ["--gpus", "1", "--steps", "2", "--warmup", "1", "--P", "5000", "--width", "200", "--height", "120"]
FULL_ONLY = ("roofline", "cpu_baseline", "aux", "allreduce")


@pytest.mark.gpu
@pytest.mark.parametrize("extra", [[], ["--per-view"]], ids=["batch", "per-view"])
def test_plain_run_is_lean_and_dumps_outputs(extra, tmp_path):
    """A plain run times the steps and prints the result line with none of the --full legs; with
    --dump-outputs it writes the last timed step's images, radii and gradients, finite and of the
    step's sizes (8 views of 5000 Gaussians at 200x120; shs: 16 x 3 floats per Gaussian)."""
    import numpy as np
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + extra + ["--dump-outputs", str(out)],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["value"] > 0 and d["full"] is False
    assert d["unit"] == "Mpix/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert all(d[k] is None for k in FULL_ONLY) and d.get("config2_single_view") is None
    V, P, N = 8, 5000, 200 * 120
    sizes = {"color": V * 3 * N, "invdepth": V * N, "radii": V * P, "grad_means3D": P * 3, "grad_scales": P * 3,
             "grad_rotations": P * 4, "grad_opacities": P, "grad_shs": P * 48, "grad_means2D": V * P * 3}
    assert sorted(os.listdir(out)) == sorted(n + ".npy" for n in sizes)
    for n, size in sizes.items():
        a = np.load(out / (n + ".npy"))
        assert a.dtype == np.float32 and a.size == size and np.isfinite(a).all() and np.count_nonzero(a) > 0, n


@pytest.mark.gpu
def test_full_run_measures_the_side_legs():
    """--full: the per-kernel pass and the geometry run again (the PMC passes, CPU baselines, aux and
    single-view legs switched off one by one here, as the --no-* options allow)."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL
                       + ["--full", "--no-pmc", "--no-cpu-baseline", "--no-aux", "--no-single-view"],
                       cwd=ROOT, env=_env(), capture_output=True, text=True, timeout=200)
    assert r.returncode == 0, r.stderr[-3000:]
    d = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
    assert d["full"] is True and d["steps"] == 2 and d["ms_per_step"] > 0
    assert {"render_fwd", "render_bwd", "preprocess_bwd"} <= set(d["roofline"]["kernels"])
    assert d["config"]["num_rendered"] > 0 and 0 < d["config"]["visible"] <= 5000


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["strong", "weak"])
def test_gpus2_gloo_rehearsal_on_one_gpu(mode):
    """The driver's `python bench.py --gpus 2` on the one GPU of the test box, both scaling modes, with
    the ranks over gloo (GSR_DIST_BACKEND; the 8-GPU nodes use RCCL): two ranks start from one
    torch.distributed.run child, each renders its views, the gradients are all-reduced, rank 0 prints
    one JSON line with n_gpus 2 and the mode's scaling and views per step (config 4's step at full
    size: 1M Gaussians, 1080p)."""
    extra = ["--views-per-rank", "8"] if mode == "weak" else []
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1",
                        "--no-cpu-baseline", "--no-aux", "--no-pmc", "--no-single-view"] + extra,
                       cwd=ROOT, env=_env(GSR_DIST_BACKEND="gloo"), capture_output=True, text=True, timeout=400)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [json.loads(ln) for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    d = lines[0]
    assert d["n_gpus"] == 2 and d["scaling"] == mode and d["value"] > 0 and d["steps"] == 2
    assert d["config"]["views_per_step"] == (16 if mode == "weak" else 8), d["config"]
