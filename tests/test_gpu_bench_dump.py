"""GPU: a plain `bench.py --gpus 1 --steps K --warmup W` run prints only the headline line, and
`--dump-outputs DIR` writes the IQ its last timed step produced: bit for bit the chain's IQ of the frames
that step encodes (step s runs resident batch s % 2, bench.shard_plan)."""
import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import dvbt2ll
from dvbt2ll.configs import CONFIGS

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parents[1]


def test_plain_bench_headline_and_dump_of_last_step(gpu, tmp_path):
    B, K = 3, 2
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--config", "cfg1", "--frames", str(B),
                        "--steps", str(K), "--warmup", "1", "--dump-outputs", str(tmp_path / "d")],
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["unit"] == "Msamples/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert d["steps"] == K and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["metric"].endswith(CONFIGS["cfg1"].name)
    for k in ("stages", "roofline", "serial_1_stream", "cpu_baseline", "latency_1_frame", "iq_sc16_x0.2"):
        assert k not in d, k                                   # those run with --full only
    assert [p.name for p in (tmp_path / "d").iterdir()] == ["iq.npy"]
    iq = np.load(tmp_path / "d" / "iq.npy")
    ch = dvbt2ll.Chain(CONFIGS["cfg1"], max_frames=B)
    assert iq.dtype == np.float32 and iq.shape == (B * ch.iq_per_frame, 2)
    want = ch.run(((K - 1) % 2) * B, B)                        # the last step's batch: frames [B, 2B)
    np.testing.assert_array_equal(iq.reshape(-1).view(np.uint32), want.view(np.uint32))
