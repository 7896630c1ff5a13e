"""bench.py on the GPU box, short runs: the strong-scaling branch (BASELINE config 5's sharding: one global list, rank r
decodes shard_range(T, r, world)) exercised on ONE GPU before an 8-GPU node ever sees it, and the default (weak) line's
contract keys, and a plain run's outputs.  The driver's own timing runs use the defaults; these runs use few steps and skip the CPU
leg."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def run_bench(*flags, full=True, steps=3):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1"] +
                       (["--full", "--no-cpu", "--no-extras"] if full else []) + list(flags),
                       cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = [l for l in p.stdout.decode().splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout.decode()[-2000:]
    return json.loads(lines[0])


def test_strong_scaling_branch_on_one_gpu(built):
    d = run_bench("--scaling", "strong", "--total-units", "8192")
    assert d["scaling"] == "strong" and d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    c = d["config"]
    assert c["bit_exact"] is True and c["units_per_gpu"] == 8192 and c["units_on_frame_parallel_path"] == 1.0
    assert abs(d["value"] - 8192 * c["unit_bytes"] / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    assert d["roofline"]["frac"] < 1.0 and d["roofline"]["kernel_ms"] <= d["ms_per_step"] * 1.02


def test_weak_line_keys(built):
    d = run_bench("--units", "1024")
    assert d["scaling"] == "weak" and d["unit"] == "MB/s" and d["dtype"] == "u8" and d["vs_baseline"] is None
    assert d["config"]["bit_exact"] is True and "workload" in d["config"] and d["roofline"]["bound"] == "hbm"


def test_plain_run_and_dump_outputs(built, tmp_path):
    """a plain run times exactly --steps steps and carries only the headline; --dump-outputs writes what the last step decoded,
    here checked against the plaintext of the same seeds"""
    import numpy as np
    import libmspack_amd as M
    from libmspack_amd import dist as D
    d = run_bench("--units", "256", "--dump-outputs", str(tmp_path), full=False, steps=2)
    assert d["steps"] == 2 and d["warmup"] == 1 and d["unit"] == "MB/s" and d["dtype"] == "u8" and d["higher_is_better"] is True
    n, ub = d["config"]["units_per_gpu"], d["config"]["unit_bytes"]
    assert n == 256 and abs(d["value"] - n * ub / (d["ms_per_step"] * 1e-3) / 1e6) / d["value"] < 0.01
    assert "roofline" not in d and "secondary" not in d and "host_inclusive" not in d and d["cpu_baseline"] is None
    files = {f.name: np.load(f) for f in tmp_path.iterdir()}
    assert sum(f.stat().st_size for f in tmp_path.iterdir()) <= 64 << 20
    assert all(a.dtype in (np.float32, np.float64) for a in files.values())
    assert (files["result_err.npy"] == 0).all() and (files["result_out_len.npy"] == ub).all()
    plain = M.corpus_lzx_units(D.unit_seed_base(0xBA5E11, 0), 0, n, ub, 21, n_threads=4)[0].reshape(n, ub).astype(np.int64)
    assert np.array_equal(files["unit_checksums.npy"], np.stack([plain.sum(1), plain @ np.arange(1, ub + 1)], 1))
    # (bench.py's recipe: positions drawn from default_rng(0x5EED) after its per-unit draws -- none at n <= 65536 -- sorted; the
    # units' outputs lie back to back here)
    pos = np.sort(np.random.default_rng(0x5EED).integers(0, n * ub, min(n * ub, 1 << 22)))
    assert np.array_equal(files["output_sample.npy"], plain.ravel()[pos])
