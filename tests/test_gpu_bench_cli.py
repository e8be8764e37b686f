"""bench.py's command line on one GPU: a plain run carries only the headline line, `--full` adds the
roofline and the CPU baseline, and `--dump-outputs` writes the last timed step's frame exactly as the
timed path left it (compared bit for bit with a render of the same config through DeviceScene.render,
and with the line's own frame_md5). C1 (400x225, 50 spp) keeps each bench process to a few seconds;
`--cpu-threads` puts the `--full` oracle run on C1's 1/64 subsample, not its whole single-thread frame."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup")


def _bench(args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "C1", *args],
                       capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def plain(tmp_path_factory):
    d = tmp_path_factory.mktemp("dump")
    return _bench(["--steps", "2", "--warmup", "1", "--dump-outputs", str(d)]), d


@pytest.mark.gpu
def test_plain_run_prints_the_headline_line_only(plain):
    line, _ = plain
    for k in HEADLINE:
        assert k in line, k
    assert "roofline" not in line and "cpu_baseline" not in line
    assert line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "Msamples/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["ms_per_step"] > 0 and line["image_finite"]
    # value and ms_per_step are the same measurement: samples of one frame over one step's time
    c = line["config"]
    samples = c["width"] * c["height"] * c["spp"]
    assert line["value"] == pytest.approx(samples / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-9)


@pytest.mark.gpu
def test_dump_outputs_is_the_frame_the_timed_path_computed(plain, rt):
    line, d = plain
    assert sorted(os.listdir(d)) == ["frame.npy", "segments.npy"]
    frame, seg = np.load(d / "frame.npy"), np.load(d / "segments.npy")
    cfg = rt.CONFIGS["C1"]
    assert frame.dtype == np.float32 and frame.shape == (cfg.height, cfg.width, 3)
    assert seg.dtype == np.float64 and seg.shape == (1,)
    assert frame.nbytes + seg.nbytes <= 64 << 20
    assert hashlib.md5(frame.tobytes()).hexdigest() == line["frame_md5"]
    assert seg[0] * line["steps"] == line["segments"]
    # the same config rendered directly: the dump is the render's output, bit for bit
    scene = rt.Scene.generate(cfg.scene, cfg.scene_seed)
    params = rt.render_params(cfg.width, cfg.height, cfg.spp, cfg.depth, background=cfg.background(),
                              seed=cfg.render_seed)
    ds = rt.DeviceScene(scene, device=0)
    got, st = ds.render(cfg.camera(), params)
    ds.close()
    assert np.array_equal(np.asarray(got, dtype=np.float32).reshape(frame.shape), frame)
    assert st["segments"] == seg[0]


@pytest.mark.gpu
def test_full_adds_roofline_and_cpu_baseline_to_the_same_line(plain):
    line, _ = plain
    full = _bench(["--steps", "1", "--warmup", "0", "--full", "--cpu-threads", "4"])
    for k in HEADLINE:
        assert k in full, k
    assert full["steps"] == 1 and full["warmup"] == 0
    assert full["metric"] == line["metric"] and full["frame_md5"] == line["frame_md5"]
    roof, cpu = full["roofline"], full["cpu_baseline"]
    assert roof["kernel"] == "trace_samples" and roof["kernel_ms"] > 0 and roof["launches_per_step"] >= 1
    assert roof["bytes_per_sample"] > 0 and roof["achieved"] > 0
    assert cpu["value"] > 0 and cpu["cores"] == 4 and cpu["gpu_over_cpu"] > 0


def test_dump_outputs_writes_float32_frame_and_float64_segments(tmp_path):
    import torch

    import bench
    flat = torch.arange(5 * 7 * 3, dtype=torch.float32) * 0.25
    bench.dump_outputs(str(tmp_path / "new" / "dir"), flat, 7, 5, 123.0)
    frame = np.load(tmp_path / "new" / "dir" / "frame.npy")
    assert frame.dtype == np.float32 and frame.shape == (5, 7, 3)
    assert np.array_equal(frame.reshape(-1), flat.numpy())
    seg = np.load(tmp_path / "new" / "dir" / "segments.npy")
    assert seg.dtype == np.float64 and seg.tolist() == [123.0]
