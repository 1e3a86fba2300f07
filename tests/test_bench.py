"""bench.py's own contract: --dump-outputs (float64, within its budget, the accumulator of the timed frames) and a plain run that
times exactly --steps frames once, with what --full adds left out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

import bench


def test_dump_outputs_float64_within_budget(tmp_path):
    acc = np.arange(1920 * 1080 * 3, dtype=np.int32).reshape(1920, 1080, 3)
    bench.dump_outputs(str(tmp_path / "a"), {"accumulator": acc})
    got = np.load(str(tmp_path / "a" / "accumulator.npy"))
    assert got.dtype == np.float64 and np.array_equal(got, acc)
    big = np.arange(3840 * 2160 * 3, dtype=np.int32).reshape(3840, 2160, 3)       # C5's frame: 199 MB in float64, sampled
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"accumulator": big})
    files = sorted(os.listdir(str(tmp_path / "b")))
    assert files == ["accumulator.npy", "accumulator_pixels.npy"]
    assert sum(os.path.getsize(str(tmp_path / "b" / f)) for f in files) <= bench.DUMP_LIMIT_BYTES
    idx = np.load(str(tmp_path / "b" / "accumulator_pixels.npy")).astype(np.int64)
    assert np.array_equal(np.load(str(tmp_path / "b" / "accumulator.npy")), big.reshape(-1, 3)[idx])
    for f in files:                       # a fixed sample: the same pixels every time
        assert np.array_equal(np.load(str(tmp_path / "b" / f)), np.load(str(tmp_path / "c" / f)))


@pytest.mark.gpu
def test_plain_run_times_the_steps_and_dumps_their_frames(tmp_path):
    """A plain run on a small heightfield: one region of exactly --steps frames, none of the --full figures, and the dumped
    accumulator is what the library computes for the timed frames' seeds."""
    K, warmup, W, H = 5, 2, 320, 192
    cache, out = str(tmp_path / "cache"), str(tmp_path / "out")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", str(warmup), "--verts", "71",
           "--width", str(W), "--height", str(H), "--cache", cache, "--dump-outputs", out]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    j = json.loads(r.stdout.strip().splitlines()[-1])
    assert j["steps"] == K and j["warmup"] == warmup and j["repeats"] == 1 and j["full"] is False
    assert j["unit"] == "Mrays/s" and j["higher_is_better"] is True and j["dtype"] == "f32" and j["value"] > 0 and j["ms_per_step"] > 0
    assert j.get("cpu_baseline") is None and j["single_frame_ms"] is None and j["roofline"]["traffic"] is None
    assert j["per_ray"]["reference_order"] is None and j["roofline"]["gather"] is None
    got = np.load(os.path.join(out, "accumulator.npy"))

    import dogeray_amd as dr
    scene = dr.Scene.load(bench.ensure_scene(cache, 71, W, H), "")
    scene.build_bvh()
    s = scene.settings()
    ctx = dr.Context(0).upload(scene)
    ctx.accum_reset(W, H)
    ctx.render_accumulate(dr.pack_settings13(s, 1, spp=1), W, H, s.background, 1 + warmup * 1000003, 1000003, K)
    want = ctx.accum_read()
    ctx.close()
    assert got.dtype == np.float64 and got.shape == (W, H, 3) and np.array_equal(got, want) and want.sum() > 0
