"""bench.py's plain run: K timed steps and the headline keys only (the rest behind --full), and --dump-outputs writing
rank 0's last timed step, the same from run to run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

_SMALL = ["--gpus", "1", "--warmup", "1", "--frames", "4", "--bank", "20000", "--encoder", "cnvnxt2ae_nano", "--settle-steps", "8"]


def _bench(args):
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    outs = []
    for i, steps in enumerate((3, 7)):
        d = tmp_path / f"run{i}"
        res = _bench([*_SMALL, "--steps", str(steps), "--dump-outputs", str(d)])
        for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
            assert key in res, key
        assert res["steps"] == steps and res["value"] > 0 and res["ms_per_step"] > 0
        assert abs(res["value"] - 4 * 8 * 1e3 / res["ms_per_step"]) <= 1e-2 * res["value"]
        # what --full adds is absent from a plain run
        assert "roofline" not in res and "cpu_baseline" not in res
        assert not {"unsettled_value", "sustained_value", "one_stream_value", "with_h2d_value"} & set(res["config"])
        files = sorted(os.listdir(d))
        assert sum(os.path.getsize(d / f) for f in files) <= 64_000_000
        arrs = {f[:-4]: np.load(d / f) for f in files}
        assert all(a.dtype in (np.float32, np.float64) for a in arrs.values())
        assert arrs["ids"].shape == (4, 8, 1) and arrs["z"].shape == (32, 768)
        assert ((arrs["ids"] >= 0) & (arrs["ids"] < 20000)).all()
        outs.append(arrs)
    # 3 and 7 steps both end on frame batch 2 of the 4 that rotate (seeded): the same last step
    a, b = outs
    assert a.keys() == b.keys()
    assert (a["ids"] == b["ids"]).all() and (a["crops"] == b["crops"]).all()
    assert np.abs(a["z"] - b["z"]).max() <= 1e-5
