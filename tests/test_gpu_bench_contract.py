"""-m gpu: bench.py prints ONE JSON line with the keys the driver reads (task contract), on a small workload so that it runs in
seconds; the default workload's line is produced by the driver itself at round end.  A plain run carries the headline keys only;
--full adds the auxiliary measurements (roofline, CPU baseline, ...)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conp_amd import neighbor, systems
from helpers import OracleRun

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE_KEYS = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config")
FULL_ONLY_KEYS = ("roofline", "roofline_hbm_member", "composite_roofline", "kernels_ms", "cpu_baseline", "configs",
                  "ms_per_step_host_buffers_pcie")


def run_bench(*extra):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "il_onelayer", *extra],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.strip()]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_prints_one_json_line_with_the_contract_keys():
    d = run_bench("--steps", "20", "--warmup", "3", "--full")
    for key in HEADLINE_KEYS + ("roofline", "cpu_baseline"):
        assert key in d, key
    assert d["n_gpus"] == 1 and d["steps"] == 20 and d["warmup"] == 3 and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert d["unit"] == "updates/s" and d["higher_is_better"] is True and d["vs_baseline"] is None
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-6)
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s") and 0.0 < r["frac"] < 1.0
    assert r["frac"] == pytest.approx(r["achieved"] / r["peak"], rel=1e-9)
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]


def test_plain_bench_times_the_steps_asked_for_and_dumps_the_charges_it_computed(tmp_path, oracle):
    d = run_bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(tmp_path / "out"))
    for key in HEADLINE_KEYS:
        assert key in d, key
    for key in FULL_ONLY_KEYS:
        assert key not in d, key
    assert d["steps"] == 7 and d["warmup"] == 2 and d["dtype"] == "f64" and d["unit"] == "updates/s"
    assert d["value"] == pytest.approx(1e3 / d["ms_per_step"], rel=1e-6)
    assert sorted(os.listdir(tmp_path / "out")) == ["q.npy"]
    q = np.load(tmp_path / "out" / "q.npy")
    # the same deck through the CPU oracle: the dumped array is the charge array of bench.py's atoms after an update
    s = systems.deck("il_onelayer", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    assert q.dtype == np.float64 and q.shape == at.q.shape and np.isfinite(q).all()
    o = OracleRun(oracle, s, at, alist, blist)
    o.setup()
    o.pre_force(s.potdiff)
    own = np.arange(len(q)) < at.nlocal
    ele = own & (at.echeck != 0)
    assert ele.sum() > 0
    err = np.abs(q[ele] - o.q[ele]).max() / np.abs(o.q[ele]).max()
    assert err < 1e-8, err
    assert np.array_equal(q[own & (at.echeck == 0)], at.q[own & (at.echeck == 0)])
