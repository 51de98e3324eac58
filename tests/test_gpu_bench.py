"""bench.py end to end on the GPU box (small workloads): the contract line, the 24-bit configuration, and the N>1 flow
rehearsed with two ranks sharing the one GPU over gloo (the real 8-GPU RCCL run belongs to the driver)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from conftest import PARAMS, ROOT

pytestmark = pytest.mark.gpu


def run_bench(*args, env=None):
    e = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args], env=e, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_single_gpu_line_small_workload():
    j = run_bench("--full", "--steps", "3", "--warmup", "1", "--rows", "2048", "--no-cpu-baseline", "--latency")
    assert j["n_gpus"] == 1 and j["dtype"] == "u64" and j["unit"] == "poly-mults/s" and j["higher_is_better"] is True
    assert j["control_plane"] == "none" and j["scaling"] == "weak"
    p = j["parity"]
    assert p["bit_exact"] is True and p["first_row_checksum_device"] == p["reference_row0_checksum"] == 2710933653778106521
    r = j["roofline"]
    assert r["bound"] == "hbm" and r["algorithmic_bytes_per_launch"] == 2048 * 98304 and 0 < r["frac"] < 1
    # (kernel_ms is printed with four decimals: at 0.08 ms per launch that alone is 0.06 % of the quotient)
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["kernel_ms"] * 1e-3) / 1e9) < 0.002 * r["achieved"]
    assert j["config"]["lib_build_id"] not in ("", "unknown")
    assert j["per_rank"]["rows"] == [2048] and set(j["latency"]["device_resident_us"]) == {"1", "16", "256"} and j["latency"]["host_buffer_us"]["1"] > 0
    assert j["strong_scaling_n1_point"] is None          # only with --strong-point


def test_cfg2_line_with_reference_cpu_baseline(tmp_path, oracle):
    j = run_bench("--full", "--config", "cfg2", "--steps", "5", "--warmup", "2", "--dump-outputs", str(tmp_path))
    # a --full run dumps the timed steps' products too; 32-bit words: the upper halves are zero
    c = dumped_words(tmp_path)
    rows = bench.dump_rows(4096, 1)
    n, q, psi = PARAMS["P1024"]
    assert c.shape == (len(rows), n) == (512, 1024) and int(c.max()) < q
    r = int(rows[-1])
    assert np.array_equal(c[-1], oracle.poly_mult(oracle.make_poly(2 * r + 1, n, q), oracle.make_poly(2 * r + 2, n, q), q, psi))
    assert j["dtype"] == "u32" and j["config"]["n"] == 1024 and j["config"]["global_batch"] == 4096
    assert j["roofline"]["algorithmic_bytes_per_launch"] == 4096 * 12288
    assert j["parity"]["bit_exact"] is True and j["parity"]["first_row_checksum_device"] == 15308795525113097448
    assert j["parity"]["rows_compared_with_cpu_oracle"] == 64
    b = j["cpu_baseline"]
    assert b is not None and b["value"] > 0 and b["cores"] >= 1 and b["cpu_model"] not in ("", "unknown")
    if os.path.exists(os.path.join(ROOT, "oracle", "_ref", "benchmark_ntt_1024_avx512")):
        assert b["kind"] == "reference" and "benchmark_ntt_1024" in b["sample"]


def test_two_ranks_without_launcher_strong_split_over_gloo():
    j = run_bench("--full", "--gpus", "2", "--steps", "2", "--warmup", "1", "--global-batch", "3000", "--no-cpu-baseline",
                  env={"BENCH_BACKEND": "gloo"})
    assert j["n_gpus"] == 2 and j["scaling"] == "strong" and j["control_plane"] == "gloo" and j["control_plane_ranks"] == 2
    assert j["config"]["global_batch"] == 3000 and j["config"]["rows_per_gpu"] == 1500
    assert j["parity"]["bit_exact"] is True
    # a straggler would show in the per-rank lists; the N = 1 blocks stay off an N > 1 line
    assert j["per_rank"]["rows"] == [1500, 1500] and len(j["per_rank"]["kernel_ms"]) == 2 and min(j["per_rank"]["kernel_ms"]) > 0
    assert j["latency"] is None and j["strong_scaling_n1_point"] is None and j["spinup_launches"] >= 40          # at least 40 launches and 0.15 s of them (bench.py: SPINUP, SPINUP_SECONDS)


def dumped_words(d, suffix=""):
    hi, lo = np.load(os.path.join(d, f"c_hi{suffix}.npy")), np.load(os.path.join(d, f"c_lo{suffix}.npy"))
    assert hi.dtype == lo.dtype == np.float64 and hi.shape == lo.shape
    return hi.astype(np.uint64) << np.uint64(32) | lo.astype(np.uint64)


def test_plain_line_and_dumped_outputs(tmp_path, oracle):
    """A plain run (no --full): the contract fields, exactly K timed steps, none of the --full blocks; --dump-outputs writes the
    sampled rows of the last step's products, and they are the negacyclic products of global rows make_poly(2r+1) x make_poly(2r+2)."""
    j = run_bench("--steps", "4", "--warmup", "1", "--rows", "2048", "--dump-outputs", str(tmp_path))
    assert j["steps"] == 4 and j["warmup"] == 1 and j["full"] is False and j["ms_per_step"] > 0 and j["value"] > 0
    assert j["unit"] == "poly-mults/s" and j["higher_is_better"] is True and j["dtype"] == "u64"
    assert abs(j["value"] - 2048 / (j["ms_per_step"] * 1e-3)) < 1e-3 * j["value"]
    assert not {"parity", "roofline", "cpu_baseline", "latency", "strong_scaling_n1_point"} & set(j)
    assert sorted(os.listdir(tmp_path)) == ["c_hi.npy", "c_lo.npy"]
    c = dumped_words(tmp_path)
    rows = bench.dump_rows(2048, 1)
    n, q, psi = PARAMS["P4096_60"]
    assert c.shape == (len(rows), n) == (512, 4096)
    for i in (0, 100, len(rows) - 1):
        r = int(rows[i])
        assert np.array_equal(c[i], oracle.poly_mult(oracle.make_poly(2 * r + 1, n, q), oracle.make_poly(2 * r + 2, n, q), q, psi)), r
