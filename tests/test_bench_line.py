"""bench.py's stdout line (CPU, no GPU): the driver keeps only the last 8 KB of stdout, and round 5's
14.4 KB line lost the default-parameter mul / sign seconds to that cut.  compose_line is fed the full set
of legs bench.py runs (leg names read from bench.py itself) with realistic values; the line must stay under
LINE_MAX_BYTES with the classic headline keys in its last 2 KB, and everything else in the detail file."""
import argparse
import json
import os
import re
import sys

import pytest

from conftest import ROOT

sys.path.insert(0, ROOT)
import bench  # noqa: E402

LEGS = re.findall(r'leg\("(\w+)"', open(os.path.join(ROOT, "bench.py")).read())


def _ops(scale):
    ops = {name: {"seconds": 0.0123456789 * scale * (i + 1), "runs": [0.0123456789 * scale] * bench.OPS_REPS,
                  "pbs": 57564 + i, "levels": 44 + i} for i, name in enumerate(LEGS)}
    ops["sign_fhe_with_k0_batch8_compat"]["signs_per_s"] = 2.93456789
    return ops


def _pbs_part(kind):
    lat = {"before_throughput": {"B=1": 1.987654321, "B=256": 2.3987654321},
           "after_throughput": {"B=1": 1.998765432, "B=256": 2.4187654321}}
    hbm = {"bound": "hbm", "achieved": 3456.789012, "peak": 8000.0, "unit": "GB/s", "frac": 0.43209876}
    l2 = dict(hbm, bound="l2_to_cu", bytes_per_launch=1791500000000, peak=34500.0)
    roof = {"bound": "fp64_valu", "compute_pipe": "fp64 VALU (FFT butterflies; no dense contraction on the path)",
            "kernel": f"k_blind_rotate_qy<{1 if kind == 'classic' else 2}>", "achieved": 31.23456789, "peak": 78.6,
            "unit": "TFLOP/s", "frac": 0.397654321, "peak_measured": 65.0, "frac_measured": 0.48123456789,
            "flops_per_pbs": 218628096, "kernel_ms": 229.87654321, "keyswitch_ms": 2.987654321, "hbm": hbm, "l2": l2}
    return {"value": 138582.123456, "ms_per_step": 236.4567891234,
            "params": "n=834,N=2048,k=1,pbs=2^23x1,ks=2^3x5,msg=4,carry=4,grouping=1", "roofline": roof,
            "pcie_inclusive_pbs_per_s": 101234.56789, "latency_level_ms": lat,
            "clock": {"shader_ghz": 2.0312345678, "cu_cycles_per_pbs": 3754123.456789, "br_cu_cycles_per_pbs": 3654123.4,
                      "wg_cycles": 11234567.891, "workgroups": 655360, "source": "s_memtime / s_memrealtime ..."}}


def _cpu():
    ops = {n: {"seconds": 123.456789, "how": "projected", "pbs": 57564, "levels": 44, "projected_seconds": 120.1}
           for n in bench.CPU_REPLAY_OPS + bench.CPU_PROJECT_OPS}
    return {"value": 1236.123456, "unit": "PBS/s", "cores": 16, "kind": "port", "nproc": 256, "affinity": 16,
            "cgroup_cpu_quota": 16.0, "simd": "avx512",
            "sample": "19744 PBS (KS+BR+SE, same params/keys shape) with the C oracle (bit-exact restatement; its "
                      "blind rotation and keyswitch loops in AVX2 / AVX-512 ...), OpenMP 16 threads = ..., 12.3 s",
            "ops": ops, "ops_note": "x" * 400}


@pytest.mark.parametrize("world", [1, 8])
def test_line_short_with_headline_last(tmp_path, world):
    a = bench.parse(["--detail", str(tmp_path / "detail.json")])
    mb = dict(_pbs_part("multibit"), ops=_ops(0.8))
    fan = None
    if world > 1:
        fan = {"ranks": world, "min_level": 257}
        for n in ("warmup_add_fast", "biguint256_mul_fast", "biguint256_mul_compat", "sign_fhe_with_k0_v0_compat",
                  "sign_fhe_with_k0_v0_fast"):
            fan[n] = {"seconds": 0.1234567, "ok": True, "split_levels": 32}
    line, detail = bench.compose_line(a, world, _pbs_part("classic"), _ops(1.0), mb, fan,
                                      _cpu() if world == 1 else None)
    text = json.dumps(line, separators=(",", ":"))
    assert len(text.encode()) < bench.LINE_MAX_BYTES, len(text)
    tail = text[-2048:]
    for key in bench.HEADLINE_KEYS:
        assert f'"{key}":' in tail, key
    assert list(line)[-len(bench.HEADLINE_KEYS):] == list(bench.HEADLINE_KEYS)
    # the contract keys and the two required objects
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in line
    for key in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert key in line["roofline"]
    assert line["clock"]["shader_ghz"] > 0 and line["clock"]["cu_cycles_per_pbs"] > 0
    if world == 1:
        for key in ("value", "unit", "cores", "kind", "sample"):
            assert key in line["cpu_baseline"]
    # everything dropped from the line is in the detail file
    assert detail["ops"]["biguint256_mul_compat"]["runs"]
    assert "multibit_ops" in detail and "vs_reference_readme" in detail
    assert "sign_fhe_with_k0_v0_callsite" in LEGS and "sign_fhe_with_k0_v0_callsite" in line["ops_s"]
    json.dumps(detail)


def test_plain_line_is_the_head_of_the_full_line():
    """without --full the line is line_head alone: the contract keys, built from the timed steps only
    (no roofline, latency or host-buffer figure asked of the leg), with the values of the full line"""
    a = bench.parse([])
    assert not a.full and a.dump_outputs is None
    full = _pbs_part("classic")
    plain = {k: full[k] for k in ("value", "ms_per_step", "params", "clock")}
    head = bench._sig(bench.line_head(a, 1, plain))
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
                "vs_baseline", "dtype", "data", "config"):
        assert key in head
    assert "roofline" not in head and "latency_level_ms" not in head
    line, _ = bench.compose_line(a, 1, full, _ops(1.0), None, None, None)
    for key in head:
        assert line[key] == head[key], key
    assert head["unit"] == "PBS/s" and head["dtype"] == "f64" and head["higher_is_better"] is True
    assert head["steps"] == a.steps and head["ms_per_step"] == pytest.approx(236.46)


def test_dump_outputs_is_a_fixed_sample_in_float64(tmp_path):
    """--dump-outputs: every row of a small batch; of a large one the same seeded DUMP_ROWS rows on
    every call, which at the engine's 2049-word ciphertexts stay under 64 MB"""
    import numpy as np
    assert bench.DUMP_ROWS * 2049 * 8 + bench.DUMP_ROWS * 8 <= 64 << 20
    rng = np.random.default_rng(1)
    small = rng.integers(0, 1 << 63, (48, 9), dtype=np.uint64)
    bench.dump_outputs(str(tmp_path / "s"), small)
    got = np.load(tmp_path / "s" / "pbs_out.npy")
    assert got.dtype == np.float64 and np.array_equal(got, small.astype(np.float64))
    assert np.array_equal(np.load(tmp_path / "s" / "pbs_out_rows.npy"), np.arange(48))
    big = rng.integers(0, 1 << 63, (bench.DUMP_ROWS * 3 + 5, 3), dtype=np.uint64)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), big)
    rows = np.load(tmp_path / "a" / "pbs_out_rows.npy")
    assert rows.dtype == np.float64 and len(rows) == bench.DUMP_ROWS == len(set(rows.tolist()))
    assert np.array_equal(rows, np.load(tmp_path / "b" / "pbs_out_rows.npy"))
    assert np.array_equal(np.load(tmp_path / "a" / "pbs_out.npy"), big[rows.astype(np.int64)].astype(np.float64))
    assert sorted(os.listdir(tmp_path / "a")) == ["pbs_out.npy", "pbs_out_rows.npy"]
