"""bench.py as a process on the GPU: a plain run prints the headline record only and --dump-outputs
writes what its last timed step returned -- equal, bit for bit, to gen_feat_window + decoding on the
same seeded window."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_is_lean_and_dumps_its_outputs(stif, sd, tmp_path):
    r = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["steps"] == 2 and line["value"] > 0 and line["unit"] == "Mpix/s" and line["dtype"] == "f16x3"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    # value and ms_per_step state the same timed steps: 6 pairs x 512 x 512 pixels per step
    assert abs(line["value"] - 6 * 512 * 512 / (line["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * line["value"]
    for moved in ("roofline", "hot_path_kernels", "top_kernels", "extra_lines", "parity", "cpu_baseline"):
        assert moved not in line                         # these are --full's
    assert sorted(os.listdir(tmp_path)) == ["out_t0.npy"]
    out = np.load(tmp_path / "out_t0.npy")
    assert out.dtype == np.float32 and out.shape == (6, 3, 512, 512)
    m = stif.LunaTokis(64, 6, 8, 5, 40)
    m.load_state_dict(sd, strict=True)
    fr = torch.empty(7, 3, 128, 128)
    for i in range(7):
        fr[i] = torch.rand(3, 128, 128, generator=torch.Generator().manual_seed(1234 + i))
    with torch.no_grad():
        m.gen_feat_window(fr.cuda())
        ref = m.decoding([torch.tensor([[0.5]])])[0].cpu().numpy()
    assert np.array_equal(out, ref)
