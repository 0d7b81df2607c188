"""bench.py's plain and --full runs and --dump-outputs.

CPU: dump_outputs writes float32 .npy files, in full up to the element limit
and above it as a 1-D sample at flat indices drawn from a fixed seed, the same
in every call.

GPU (a small Cornell frame, 96x64 at 4 spp, two timed steps): a plain run
times exactly --steps frames, runs neither the serialised roofline frame nor
the CPU baseline, and dumps the frame its last step returned: rgba.npy and
film.npy equal, bit for bit, a render of the same scene made in this process.
A --full run of the same arguments adds the roofline frame and the CPU
baseline and dumps the same arrays (the dump is taken before the extra frame
reuses the film).
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bench
from core_amd.scene import probe_scene
from tests.conftest import ROOT

W, H, SPP, STEPS = 96, 64, 4, 2
ARGS = ["--gpus", "1", "--scene", "cornell", "--width", str(W), "--height", str(H), "--spp", str(SPP),
        "--steps", str(STEPS), "--warmup", "1"]


def test_dump_outputs_full_and_sampled(tmp_path):
    a = torch.arange(1000, dtype=torch.float32).reshape(10, 100) * 0.5
    b = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    for d in ("one", "two"):
        bench.dump_outputs(str(tmp_path / d), {"a": (a, 64), "b": (b, 64)})
    got_a, got_b = np.load(tmp_path / "one" / "a.npy"), np.load(tmp_path / "one" / "b.npy")
    assert got_b.dtype == np.float32 and got_b.shape == (2, 3, 4) and (got_b == b.numpy()).all()
    idx = np.random.default_rng(bench.DUMP_SEED).integers(0, 1000, 64)
    assert got_a.dtype == np.float32 and got_a.shape == (64,)
    assert (got_a == a.numpy().reshape(-1)[idx]).all()
    assert (np.load(tmp_path / "two" / "a.npy") == got_a).all()


def test_default_dump_fits_64_mb():
    # the headline frame: rgba in full, the film sampled
    assert 1920 * 1080 * 4 <= bench.DUMP_RGBA_ELEMS
    assert 4 * (bench.DUMP_RGBA_ELEMS + bench.DUMP_FILM_ELEMS) + 1024 <= 64 * 10**6


def _bench(extra, outdir):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + ARGS + extra + ["--dump-outputs", outdir],
                       env=env, cwd=ROOT, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), np.load(os.path.join(outdir, "rgba.npy")), np.load(os.path.join(outdir, "film.npy"))


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    return _bench([], str(tmp_path_factory.mktemp("plain")))


@pytest.mark.gpu
def test_plain_run_is_lean_and_dumps_last_frame(gpu_device, plain):
    out, rgba, film = plain
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert k in out, k
    assert out["unit"] == "Mrays/s" and out["higher_is_better"] is True and out["dtype"] == "f32"
    assert out["steps"] == STEPS and out["warmup"] == 1
    assert out["config"]["camera_samples"] == W * H * SPP * STEPS  # the counters cover exactly the timed steps
    rays = out["config"]["closest_rays"] + out["config"]["shadow_rays"]
    assert out["value"] == pytest.approx(rays / (out["ms_per_step"] * STEPS * 1e-3) / 1e6, rel=1e-3, abs=2e-3)
    assert out["cpu_baseline"] is None
    assert out["roofline"]["timing"].startswith("timed frames")
    assert rgba.dtype == np.float32 and rgba.shape == (H, W, 4)
    assert film.dtype == np.float32 and film.shape == (H, W, 5)
    s, p = probe_scene("cornell_pt", W, H)
    p.aa_samples = SPP
    gpu_device.upload(s)
    f = gpu_device.new_film(p)
    gpu_device.render_shard(p, f)
    want_rgba = gpu_device.film_resolve(p, f).cpu().numpy()
    assert (film.view(np.uint32) == f.cpu().numpy().view(np.uint32)).all()
    assert (rgba.view(np.uint32) == want_rgba.view(np.uint32)).all()
    assert rgba[..., :3].max() > 0


@pytest.mark.gpu
def test_full_run_adds_roofline_frame_and_cpu_baseline(plain, tmp_path):
    out, rgba, film = _bench(["--full", "--cpu-seconds", "0.2"], str(tmp_path))
    assert out["steps"] == STEPS and out["config"]["camera_samples"] == W * H * SPP * STEPS
    assert out["roofline"]["timing"].startswith("serialised frame")
    assert out["cpu_baseline"]["value"] > 0 and out["cpu_baseline"]["kind"] == "port"
    for k in ("closest_rays", "shadow_rays"):
        assert out["config"][k] == plain[0]["config"][k]
    assert (rgba.view(np.uint32) == plain[1].view(np.uint32)).all()
    assert (film.view(np.uint32) == plain[2].view(np.uint32)).all()
