"""bench.py's plain run on the GPU (no --full): one JSON line holding the headline alone, and
--dump-outputs writing the ciphertexts its last timed step computed -- compared word for word with the
same batch bootstrapped in this process from the same seed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

pytestmark = pytest.mark.gpu
B = 2500  # above DUMP_ROWS (a sampled dump) and above the throughput kernel's threshold; not a multiple of 256


def test_plain_run_line_and_dumped_outputs(tmp_path):
    assert B > bench.DUMP_ROWS
    dump = tmp_path / "dump"
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", str(B), "--dump-outputs", str(dump)], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.strip().splitlines()
    assert len(lines) == 1, lines
    line = json.loads(lines[0])
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
    assert line["metric"] == bench.METRIC and line["unit"] == "PBS/s" and line["dtype"] == "f64"
    assert line["higher_is_better"] is True and line["ms_per_step"] > 0
    # value = PBS per second of the timed steps (both rounded to 5 significant digits in the line)
    assert line["value"] == pytest.approx(B / (line["ms_per_step"] * 1e-3), rel=1e-3)
    for moved in ("roofline", "ops_s", "multibit", "cpu_baseline", "latency_level_ms", "pcie_inclusive_pbs_per_s"):
        assert moved not in line, moved

    assert sorted(os.listdir(dump)) == ["pbs_out.npy", "pbs_out_rows.npy"]
    got, rows = np.load(dump / "pbs_out.npy"), np.load(dump / "pbs_out_rows.npy")
    assert got.dtype == np.float64 and rows.dtype == np.float64
    assert got.shape == (bench.DUMP_ROWS, 2049) and rows.shape == (bench.DUMP_ROWS,)
    rows = rows.astype(np.int64)
    assert np.all(np.diff(rows) > 0) and rows[0] >= 0 and rows[-1] < B

    # the same keys, inputs and table as bench.pbs_leg at its default seed, rank 0
    from fhe_sign import Context, generate_keys
    seed = bench.parse([]).seed
    ck, sk = generate_keys(seed=seed)
    ctx = Context(0)
    try:
        ctx.set_server_key(sk)
        lid = ctx.lut([(m + 1) % 16 for m in range(16)])
        ck.seed_encryption(seed, 100)
        want = ctx.pbs(ck.encrypt_blocks(np.arange(B) % 16), lid)
    finally:
        ctx.close()
    assert want.dtype == np.uint64
    assert np.array_equal(got, want[rows].astype(np.float64))
    assert all(ck.decrypt_block(want[i]) == (i % 16 + 1) % 16 for i in rows[::64])
