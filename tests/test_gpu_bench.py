"""bench.py on the GPU: a plain run measures the headline figure only and --dump-outputs writes
what the timed path returned in its last step."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BATCH = 3


def test_plain_run_dumps_the_last_steps_outputs(cuda, tmp_path):
    """One plain run (ViT-B/16 @224, 3 images, 2 timed steps): the result line keeps the
    headline keys and drops what --full measures; logits.npy / detections.npy are float32
    (3, 17, 6) and equal what the same model returns here for the same seeded images, within
    the bf16 mode's tolerance against its oracle (tests/test_gpu_model.py TOL: 3e-2 of
    max|ref|) -- both sides run the same kernels on the same inputs."""
    import bench
    import vision_transformer_detector_amd as vtd
    out_dir = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
                        "--steps", "2", "--warmup", "1", "--batch", str(BATCH),
                        "--dump-outputs", str(out_dir)],
                       capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    line = json.loads(lines[0])
    assert line["steps"] == 2 and line["unit"] == "images/s" and line["dtype"] == "bf16"
    assert line["higher_is_better"] is True and line["metric"]
    assert line["ms_per_step"] > 0
    assert line["value"] == pytest.approx(1e3 * BATCH / line["ms_per_step"], rel=1e-2)
    for key in bench.FULL_KEYS + ("parity_mode", "cpu_baseline"):
        assert key not in line
    assert sorted(os.listdir(out_dir)) == ["detections.npy", "logits.npy"]
    logits = np.load(out_dir / "logits.npy")
    dets = np.load(out_dir / "detections.npy")

    model = vtd.create_vision_transformer_detector(
        **vtd.presets.PRESETS["vit_b16_224"], dtype="bfloat16", device=cuda, seed=0)
    gen = torch.Generator(device=cuda).manual_seed(1234)
    want_logits, want_dets = model.detect(
        bench.letterbox_images(BATCH, model.input_shape, gen, cuda))
    for got, want in ((logits, want_logits), (dets, want_dets)):
        want = want.float().cpu().numpy()
        assert got.dtype == np.float32 and got.shape == want.shape == (BATCH, 17, 6)
        assert np.isfinite(got).all()
        assert np.abs(got - want).max() <= 3e-2 * np.abs(want).max()
