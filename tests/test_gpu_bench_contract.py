"""bench.py contract on a GPU box: one JSON line with the driver's keys at N = 1, and the N > 1 control flow (head sharding,
chunk launches on two streams, per-chunk all-gather, max-over-ranks timing) as a 2-process smoke run — both ranks on cuda:0 over
gloo (SVG_BENCH_SMOKE), because a gpurun box has one GPU; RCCL itself is exercised by the driver's 8-GPU run."""
import json
import os
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu

KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype",
        "data", "config", "roofline", "cpu_baseline"}


def _last_json(out: str):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, out[-2000:]
    return json.loads(lines[-1])


@pytest.fixture(scope="module")
def one_rank_line():
    """the one-rank `bench.py --workload tiny` line, run once per module: the reference `output_checksum` of the N-rank runs (the inputs are
    seeded per global head, so every world size must leave the same bytes) — a fixture, so that any test of this module runs alone or in any order"""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup", "1", "--full", "--no-cpu"],
                       capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    return _last_json(r.stdout)


def test_bench_single_gpu_json_line(one_rank_line):
    d = one_rank_line
    assert KEYS <= set(d), sorted(KEYS - set(d))
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True and d["dtype"] == "bf16"
    assert d["value"] > 0 and d["ms_per_step"] > 0
    rf = d["roofline"]
    assert rf["bound"] == "mfma" and rf["peak"] == 2500.0 and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert "workload" in d["config"] and "model" not in d["config"]
    assert len(d["output_checksum"]) == 16


FULL_ONLY_KEYS = {"cpu_baseline", "dense_same_gpu", "same_box_ab", "fp8_hy720p", "svg1_other_models", "svg2_wan720p", "denoise_step_hy720p",
                  "denoise_step_wan720p_svg2", "hbm_kernels"}


def test_bench_plain_line_and_dump_outputs(one_rank_line, tmp_path):
    """a plain run (no --full) times the steps and nothing else; --dump-outputs writes the last step's output, and those bytes are the
    ones `output_checksum` digests — the same checksum as the --full run of the fixture (same seeded inputs).  A second plain run
    dumps the same arrays bit for bit."""
    import numpy as np

    for run in ("a", "b"):
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "tiny", "--steps", "3", "--warmup", "1", "--dump-outputs",
                            str(tmp_path / run)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert r.returncode == 0, r.stderr[-2000:]
    for name in ("attn_out.npy", "sample_mse.npy"):
        assert np.array_equal(np.load(tmp_path / "a" / name), np.load(tmp_path / "b" / name)), name
    d = _last_json(r.stdout)
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(d) and not FULL_ONLY_KEYS & set(d)
    assert d["metric"] == one_rank_line["metric"] and d["unit"] == "TFLOP/s" and d["dtype"] == "bf16" and d["steps"] == 3
    assert d["value"] > 0 and d["ms_per_step"] > 0 and d["clock"] is None
    assert d["output_checksum"] == one_rank_line["output_checksum"]
    o = np.load(tmp_path / "b" / "attn_out.npy")
    mse = np.load(tmp_path / "b" / "sample_mse.npy")
    assert o.dtype == np.float32 and o.shape == (4, 5 * 600 + 256, 128) and mse.dtype == np.float32 and mse.shape == (2, 4)
    assert np.isfinite(o).all() and np.isfinite(mse).all()
    bits = (o.view(np.uint32) >> 16).astype(np.uint16).view(np.int16).astype(np.int64)   # the bf16 output, exact in float32
    acc = 0
    for h in range(bits.shape[0]):
        acc = (acc * 1000003 + int((bits[h] * (np.arange(bits.shape[-1]) + 1)).sum()) + 31 * int(bits[h].sum())) % (1 << 64)
    assert f"{acc:016x}" == d["output_checksum"]


def test_bench_two_rank_control_flow_smoke(one_rank_line):
    env = dict(os.environ, SVG_BENCH_SMOKE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload", "tiny", "--full"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["config"]["parallelism"] == "heads/2"
    assert d["value"] > 0 and d["cpu_baseline"] is None
    ex = d["exchange"]
    assert ex["rccl_ranks_seen"] == 2 and ex["fallback_to_chunk_launches"] is False and ex["waiter_timeouts_in_timed_steps"] == 0
    assert ex["inbound_bytes_received_per_rank"] > 0 and ex["outbound_bytes_received_per_rank"] > 0
    # the gathered output of the two-rank run == the one-rank run's, bit for bit (inputs are seeded per global head)
    assert d["output_checksum"] == one_rank_line["output_checksum"], (d["output_checksum"], one_rank_line["output_checksum"])
    sd = d["denoise_step_hy720p"]     # the token-sharded denoise step at N = 2 (reduced stack on the tiny workload)
    assert sd["n_gpus"] == 2 and sd["sparse_step"]["ms"] > 0 and sd["sparse_step"]["rccl_bytes_received_per_step_this_rank"] > 0
    sw = d["denoise_step_wan720p_svg2"]   # the Wan SVG2 step, token- / head-sharded at N = 2
    assert sw["n_gpus"] == 2 and sw["sparse_step"]["ms"] > 0 and sw["sparse_step"]["rccl_bytes_received_per_step_this_rank"] > 0


def test_bench_two_rank_watchdog_falls_back(one_rank_line):
    """Waiters that never see their count (test hook) give up at their deadline during warm-up; the bench then switches to one
    launch per chunk of heads on every rank, says so, and still produces a checked result (the smoke run's poisoned-output test)."""
    env = dict(os.environ, SVG_BENCH_SMOKE="1", SVG_BENCH_TEST_STUCK_WAITER="1", SVG_BENCH_WAITER_TIMEOUT_MS="20")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29543", str(ROOT / "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--workload", "tiny"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    ex = d["exchange"]
    assert ex["fallback_to_chunk_launches"] is True and ex["waiter_timeouts_in_timed_steps"] == 0
    assert "per chunk" in ex["outbound"]
    # the fallback path (one launch + all-gather per chunk of heads) leaves the same bytes as the one-rank run (and so as the overlapped path)
    assert d["output_checksum"] == one_rank_line["output_checksum"], (d["output_checksum"], one_rank_line["output_checksum"])


def test_bench_fp8_line():
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup", "1", "--full", "--no-cpu",
                        "--dtype", "fp8"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _last_json(r.stdout)
    assert KEYS <= set(d) and d["dtype"] == "fp8" and d["value"] > 0
    rf = d["roofline"]
    assert rf["peak"] == 5000.0 and rf["kernel"].startswith("band_attn_f8_kernel") and abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-3
    assert 0 < d["fp8"]["prepass_ms"] < d["ms_per_step"] and 1e-3 < d["fp8"]["rel_l2_vs_bf16_kernel_this_workload"] < 0.1


def test_bench_step_small_stack():
    """bench_step.measure on a 1 + 1 block stack (the full 20 + 40 stack is what bench.py embeds): finite outputs, both kinds of
    step, attention share in (0, 1)."""
    sys.path.insert(0, str(ROOT))
    import bench_step

    d = bench_step.measure(steps=1, warmup=0, n_double=1, n_single=1)
    for kind in ("sparse_step", "dense_step"):
        assert d[kind]["ms"] > 0 and 0 < d[kind]["attention_share"] < 1 and d[kind]["gemm_tflop_this_rank"] > 0
    assert d["denoise_steps_per_s"] > 0 and d["speedup_sparse_vs_dense_step"] > 0 and d["n_gpus"] == 1


def test_bench_step_two_rank_smoke():
    """bench_step.py --gpus 2 (BASELINE.json configs[3] at N > 1): token-sharded stack, head-sharded attention, the exchanges and the
    final all-gather — both ranks on cuda:0 over gloo through host memory (SVG_BENCH_SMOKE): control flow and bookkeeping, not speed.
    The sharded step's hidden states are checked against the single-process step by tests/test_step_sharding_cpu.py."""
    env = dict(os.environ, SVG_BENCH_SMOKE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29547", str(ROOT / "bench_step.py"), "--gpus", "2", "--tiny", "--layers-double", "1", "--layers-single", "1",
           "--steps", "1", "--warmup", "1"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and "tokens/2" in d["parallelism"] and "gloo" in d["exchange_backend"]
    for kind in ("sparse_step", "dense_step"):
        assert d[kind]["ms"] > 0 and d[kind]["rccl_bytes_received_per_step_this_rank"] > 0
    assert d["denoise_steps_per_s"] > 0


def test_bench_step_wan_small_stack():
    """bench_step.measure_wan (what bench.py embeds as `denoise_step_wan720p_svg2`, BASELINE.json configs[2]) on a 3-block stack of a small
    geometry: layer 0 dense, layers 1-2 SVG2 with the k-means init in the first sparse step and the warm start after it; both kinds of step,
    the stage breakdown sums to the step."""
    sys.path.insert(0, str(ROOT))
    import bench_step

    geo = bench_step.WanGeo(F=5, P=600, hid=512, heads=4, hd=128, ffn=1024, text=64, layers=3, qc=20, kc=40)
    d = bench_step.measure_wan(steps=1, warmup=0, geo=geo)
    assert not _error_keys(d), _error_keys(d)
    for kind in ("sparse_step", "dense_step"):
        b = d[kind]["step_breakdown_ms"]
        assert d[kind]["ms"] > 0 and 0 < d[kind]["attention_share"] < 1 and d[kind]["gemm_tflops_this_rank"] > 0   # (the small stack's TFLOP round to 0.0)
        assert {"gemm", "glue", "prologue", "self_attention", "cross_attention"} <= set(b)
        assert abs(sum(b.values()) - d[kind]["ms"]) < 0.05 * d[kind]["ms"] + 0.1
    assert d["denoise_steps_per_s"] > 0 and d["first_sparse_step_ms_with_kmeans_init"] > 0 and d["n_gpus"] == 1


def test_bench_step_wan_two_rank_smoke():
    """bench_step.py --model wan720p --gpus 2: the Wan SVG2 step token-sharded / head-sharded over two ranks on cuda:0 (gloo through host memory):
    control flow — exchanges, the all-reduced k-means stopping rule, the final all-gather.  Equality with the one-process step:
    tests/test_step_sharding_cpu.py::test_wan_svg2_token_sharded_step_equals_single_process."""
    env = dict(os.environ, SVG_BENCH_SMOKE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29549", str(ROOT / "bench_step.py"), "--gpus", "2", "--tiny", "--model", "wan720p", "--steps", "1", "--warmup", "0"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    d = _last_json(r.stdout)
    assert d["n_gpus"] == 2 and "tokens/2" in d["parallelism"] and "gloo" in d["exchange_backend"]
    for kind in ("sparse_step", "dense_step"):
        assert d[kind]["ms"] > 0 and d[kind]["rccl_bytes_received_per_step_this_rank"] > 0
    assert d["denoise_steps_per_s"] > 0


def _error_keys(node, path=""):
    """every path in a bench line's JSON at which an "error"-like key sits (an extras block that raised)."""
    found = []
    if isinstance(node, dict):
        for k, v in node.items():
            if "error" in str(k).lower():
                found.append(f"{path}/{k}")
            found += _error_keys(v, f"{path}/{k}")
    elif isinstance(node, list):
        for i, v in enumerate(node):
            found += _error_keys(v, f"{path}[{i}]")
    return found


@pytest.mark.parametrize("fp8", [False, True])
def test_bench_svg2_measure_small(fp8):
    """bench_svg2.measure() is what bench.py embeds as svg2_wan720p / svg2_wan720p_fp8 (BASELINE.json configs[2] / [4]): called the way
    bench.py calls it, on the reduced geometry.  (Round 3's driver line lost both blocks to an AttributeError inside measure().)"""
    sys.path.insert(0, str(ROOT))
    import bench_svg2

    d = bench_svg2.measure("small", steps=1, warmup=0, fp8=fp8)
    assert not _error_keys(d), _error_keys(d)
    assert d["ms"]["total"] > 0 and d["ms"]["attention"] > 0 and 0 < d["density_mean"] <= 1
    assert d["spot_rows_rel_l2_vs_torch_fp32"] < (0.15 if fp8 else 4e-3)
    if fp8:
        assert "rel_l2_vs_16bit_kernel" in d


HBM_ROWS = ("placement_qkv", "inverse_placement_o", "qk_norm_rope_inplace", "qk_norm_rope_transpose", "label_sort", "svg2_gather",
            "svg2_scatter", "layernorm_modulate", "modulate_gate_residual", "wan_rmsnorm_rope_transpose_qkv", "wan_rmsnorm_rope_transpose_qk")


def _check_hbm_block(block):
    """the `hbm_kernels` block of the bench line (bench_hbm.measure): one roofline row per HBM-bound kernel of SURVEY §8(d)"""
    assert not _error_keys(block), _error_keys(block)
    assert block["peak_GBs"]["spec"] == 8000.0 and block["torch_copy_this_box"]["GBs"] > 0
    for name in HBM_ROWS:
        r = block["kernels"][name]
        assert r["ms"] > 0 and r["algorithmic_bytes"] > 0 and r["GBs"] > 0
        assert abs(r["GBs"] - r["algorithmic_bytes"] / r["ms"] / 1e6) <= 0.01 * r["GBs"] + 0.1      # (ms is rounded to 1e-4)
        assert abs(r["frac_of_8TBs"] - r["GBs"] / 8000.0) < 1e-3 and 0 < r["frac_of_8TBs"] < 1.0
        assert "svg/" in r["reference"]


def test_bench_hbm_measure_small():
    """bench_hbm.measure() is what bench.py embeds as `hbm_kernels`: called the way bench.py calls it, on the reduced geometry."""
    sys.path.insert(0, str(ROOT))
    import bench_hbm

    _check_hbm_block(bench_hbm.measure("small", reps=2))


def test_bench_line_with_extras_has_no_error_key():
    """bench.py with every extras block switched on (reduced geometries): exit code 0 and no "error" key anywhere in the line."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "tiny", "--steps", "2", "--warmup", "1", "--full", "--no-cpu",
                        "--extras", "small"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-1500:] + r.stderr[-1500:])
    d = _last_json(r.stdout)
    assert not _error_keys(d), _error_keys(d)
    for key in ("svg2_wan720p", "svg2_wan720p_fp8", "denoise_step_hy720p", "denoise_step_wan720p_svg2", "hbm_kernels"):
        assert key in d, sorted(d)
    assert d["svg2_wan720p_fp8"]["status"].startswith("closed") and d["denoise_step_hy720p"]["fp8_attention"]["status"].startswith("closed")
    assert "denoise_steps_per_s_fp8_attention" not in d["denoise_step_hy720p"] and "denoise_steps_per_s_video_average" not in d["denoise_step_hy720p"]
    assert d["denoise_step_wan720p_svg2"]["denoise_steps_per_s"] > 0 and d["denoise_step_wan720p_svg2"]["sparse_step"]["step_breakdown_ms"]["gemm"] > 0
    _check_hbm_block(d["hbm_kernels"])
    op = d["online_profiler"]     # the layer-call's HBM-bound kernel: K and V of every head once
    assert op["ms"] > 0 and op["bound"] == "hbm" and abs(op["GBs"] - op["algorithmic_bytes"] / op["ms"] / 1e6) <= 0.01 * op["GBs"] + 0.1
    assert abs(op["frac_of_8TBs"] - op["GBs"] / 8000.0) < 1e-3 and "svg/" in op["reference"]
    assert d["svg2_wan720p"]["ms"]["total"] > 0 and d["svg2_wan720p_fp8"]["ms"]["total"] > 0
    assert d["denoise_step_hy720p"]["denoise_steps_per_s"] > 0


def test_bench_exits_nonzero_when_an_extras_block_raises():
    """a failing extras block must not vanish silently: the line still carries the error string, and the exit code is 3."""
    env = dict(os.environ, SVG_BENCH_TEST_BREAK_EXTRAS="1")
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--workload", "tiny", "--steps", "1", "--warmup", "1", "--full", "--no-cpu",
                        "--extras", "small", "--no-step"], capture_output=True, text=True, timeout=900, cwd=ROOT, env=env)
    assert r.returncode == 3, (r.returncode, r.stderr[-1500:])
    d = _last_json(r.stdout)
    assert "error" in d["svg2_wan720p"] and d["value"] > 0
