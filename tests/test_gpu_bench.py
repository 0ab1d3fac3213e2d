"""bench.py at N = 1 as the driver runs it: a plain run (headline only) with --dump-outputs, and a --full run with
every leg that a plain run leaves out."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

pytestmark = pytest.mark.gpu

N = 1_500_000   # per set: the union (2e6) is sampled, the intersection (1e6) is dumped whole


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--warmup", "1", "--set-size", str(N)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def _load(d, name):
    a = np.load(os.path.join(str(d), name + ".npy"))
    assert a.dtype == np.float64
    return a


def test_plain_run_dumps_the_last_steps_outputs(tmp_path):
    import bench
    res = _bench("--steps", "3", "--dump-outputs", str(tmp_path / "a"))
    assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["value"] > 0 and res["unit"] == "k-mers/s"
    assert res["higher_is_better"] is True and res["dtype"] == "u64" and res["full"] is False
    assert res["cpu_baseline"] is None and res["taxid_variant"] is None and res["parity_checked"] is None
    assert res["outputs_dumped_to"] == str(tmp_path / "a")
    A, B = bench.gen_sets_numpy((4 * N + 2) // 3, 32, 0, bench.SEED)
    U, I = np.union1d(A, B), np.intersect1d(A, B)
    xor = []
    for name, want in (("union", U), ("inter", I)):
        pos = _load(tmp_path / "a", name + "_index").astype(np.int64)
        codes = (_load(tmp_path / "a", name + "_hi").astype(np.uint64) << np.uint64(32)) | \
            _load(tmp_path / "a", name + "_lo").astype(np.uint64)
        assert len(pos) == min(len(want), bench.DUMP_SAMPLE) and np.all(np.diff(pos) > 0)
        assert np.array_equal(codes, want[pos])
        x = int(np.bitwise_xor.reduce(want))
        xor += [x >> 32, x & 0xFFFFFFFF]
    assert len(U) > bench.DUMP_SAMPLE >= len(I)          # one sampled output, one whole
    assert _load(tmp_path / "a", "counts").tolist() == [len(U), len(I)]
    assert _load(tmp_path / "a", "xor").tolist() == xor
    assert sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a"))) <= 64 << 20
    # the inputs are seeded: another run (of fewer steps) writes the same files
    _bench("--steps", "1", "--dump-outputs", str(tmp_path / "b"))
    for f in sorted(os.listdir(str(tmp_path / "a"))):
        assert np.array_equal(_load(tmp_path / "a", f[:-4]), _load(tmp_path / "b", f[:-4])), f


def test_full_run_keeps_every_leg():
    res = _bench("--steps", "2", "--full", "--cpu-sample", "1e5")
    assert res["full"] is True and res["steps"] == 2 and res["ms_per_step"] > 0
    assert res["parity_checked"] and res["cpu_baseline"]["value"] > 0 and res["speedup_vs_cpu_port"] > 0
    tax = res["taxid_variant"]
    assert "error" not in tax, tax
    assert tax["one_taxid_per_file"]["union_kernel_ms"] > 0 and tax["per_record_taxids"]["inter_kernel_ms"] > 0
    assert res["roofline"]["frac"] > 0 and res["outputs_dumped_to"] is None
