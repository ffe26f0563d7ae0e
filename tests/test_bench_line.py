"""bench.py's last stdout line must survive the driver's capture: the driver keeps the last 8 KB of stdout (+ stderr) and
parses the final line.  Round 3's line was 25 KB (profiles/r03_z_bench_default.json is that record) and was lost."""
import importlib.util
import io
import json
import os
import subprocess
import sys
from contextlib import redirect_stdout

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("hfcl_bench", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _full_record():
    return json.load(open(os.path.join(ROOT, "profiles", "r03_z_bench_default.json")))


def test_compact_line_fits_and_carries_the_contract():
    b = _bench()
    full = _full_record()
    assert len(json.dumps(full)) > 20_000  # the record that was lost
    line = b.compact_line(full)
    assert "\n" not in line and len(line) < 4096
    d = json.loads(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["config"]["workload"] == full["config"]["workload"] and "model" not in d["config"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel", "kernel_ms", "bytes_per_query", "units_per_launch"):
        assert k in d["roofline"], k
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in d["cpu_baseline"], k
    # numbers are the full record's, to the printed digits
    assert abs(d["value"] - full["value"]) <= 1e-4 * full["value"]
    assert abs(d["roofline"]["frac"] - full["roofline"]["frac"]) <= 1e-4 * full["roofline"]["frac"]
    assert abs(d["roofline"]["achieved"] / d["roofline"]["peak"] - d["roofline"]["frac"]) < 1e-6
    assert len(d["secondary"]) == len(full["secondary"])
    for row, s in zip(d["secondary"], full["secondary"]):
        assert abs(row["value"] - s["value"]) <= 1e-3 * s["value"]


def test_last_8000_bytes_of_stdout_parse():
    """What the driver does: keep the tail of stdout, parse its last line."""
    b = _bench()
    full = _full_record()
    buf = io.StringIO()
    with redirect_stdout(buf):
        print("RCCL version banner and other library chatter " * 400)  # noise before the line
        print(b.compact_line(full), flush=True)
    tail = buf.getvalue()[-8000:]
    last = tail.rstrip("\n").rsplit("\n", 1)[-1]
    d = json.loads(last)
    assert d["metric"] and d["roofline"]["frac"] is not None and d["cpu_baseline"]["value"] > 0


def test_compact_line_drops_rows_before_it_overflows():
    b = _bench()
    full = _full_record()
    full["secondary"] = full["secondary"] * 8  # 80 rows
    line = b.compact_line(full)
    assert len(line) <= b.COMPACT_LIMIT
    d = json.loads(line)
    assert d["secondary_truncated"] and d["roofline"]["kernel"] and d["cpu_baseline"]["value"] > 0


def test_two_stream_rows_and_errors():
    b = _bench()
    full = _full_record()
    full["secondary"][0] = {"workload": "cfg2", "error": "RuntimeError('x' * 500)" + "y" * 500}
    full["secondary"][1]["batches_in_flight"] = 2
    full["secondary"][1]["roofline"] = {"frac": None, "kernel": None}
    d = json.loads(b.compact_line(full))
    assert len(d["secondary"][0]["error"]) <= 80
    assert d["secondary"][1]["l2_frac"] is None and d["secondary"][1]["hbm_frac"] is None and d["secondary"][1]["batches_in_flight"] == 2


def test_line_explains_itself():
    """The fields the round-5 review asked the line to carry: the dominant kernel under the name rocprofv3 lists it by (and the library's
    timer label beside it), the step's HBM bytes against the algorithmic bytes, useful flop against the fp32 vector peak, where the counter
    figures come from, the CPU figure of a -march=native build beside the reference's default arithmetic; N > 1: what the exchange did."""
    b = _bench()
    full = _full_record()
    full["roofline"].update({"kernel": "k_epa_loop<float, 8, 17>", "timer_label": "k_epa<fast>", "traffic_ratio": 5.2, "step_traffic": 8.6e8,
                             "step_traffic_ratio": 8.0, "useful_flop_per_query": 6400.0, "useful_flop_frac": 0.0241,
                             "traffic_source": "profiles/traffic_cfg3.json (PMC pass of this device code, source_sha 0123456789abcdef; replayed, not collected in this run)"})
    full["cpu_baseline"]["native"] = {"value": 612345.0, "cores": 1, "build": "g++ -O3 -march=native (FMA contraction on)"}
    full["config"]["exchange"] = {"ranks_seen": 8, "ms": 0.41, "bus_GBps": 730.0, "frac_of_link_budget": 0.68, "bytes_received_per_rank": 7 * 44_000_000,
                                  "bytes_sent_per_rank": 44_000_000, "link_budget_GBps": 1071.0}
    full["config"]["per_rank_ms_no_exchange"] = {"max": 1.71, "min": 1.69, "rank0": 1.70, "note": "x"}
    line = b.compact_line(full)
    assert len(line) <= b.COMPACT_LIMIT
    d = json.loads(line)
    rf = d["roofline"]
    assert rf["kernel"].startswith("k_epa_loop<") and rf["timer_label"] == "k_epa<fast>"
    for k in ("traffic_ratio", "step_traffic", "step_traffic_ratio", "useful_flop_per_query", "useful_flop_frac", "traffic_source"):
        assert rf[k] is not None, k
    assert "replayed" in rf["traffic_source"]
    assert d["cpu_baseline"]["native"]["value"] == 612350.0 or abs(d["cpu_baseline"]["native"]["value"] - 612345.0) < 10
    assert d["config"]["exchange"]["ranks_seen"] == 8 and d["config"]["exchange"]["frac_of_link_budget"] == 0.68
    assert d["config"]["per_rank_ms_no_exchange"] == {"max": 1.71, "min": 1.69}


def test_timer_labels_resolve_to_profiler_names():
    """bench.rocprof_names: the library's timer labels against the kernel names of the committed rocprofv3 traces."""
    b = _bench()
    assert any("k_epa_loop<float" in n for n in b.rocprof_names("cfg3", "k_epa<fast>"))
    assert any("k_gjk_cvx<2, 0" in n for n in b.rocprof_names("cfg3", "k_gjk_cvx<cc>"))
    names = b.rocprof_names("cfg4", "k_bvh_collide")
    assert names and all(("k_bvh_" in n or "k_tri_leaves" in n) and "true>" not in n for n in names)
    assert b._label_matches("k_bvh_collide", "void k_bvh_walk<double>(Work, ...)") and b._label_matches("k_bvh_collide", "void k_tri_leaves<double>(Work")
    assert not b._label_matches("k_bvh_collide", "void k_bvh_collide<double, false, false, true>(Work")


def test_plain_run_line():
    """A run without --full: the contract's fields as they are, `roofline` and `cpu_baseline` null, no secondary rows."""
    b = _bench()
    full = _full_record()
    full.update(roofline=None, cpu_baseline=None)
    for k in ("secondary", "host_buffers"):
        full.pop(k, None)
    d = json.loads(b.compact_line(full))
    for k in ("metric", "unit", "higher_is_better", "dtype", "steps", "warmup"):
        assert d[k] == full[k], k
    assert abs(d["value"] - full["value"]) <= 1e-4 * full["value"] and abs(d["ms_per_step"] - full["ms_per_step"]) <= 1e-4 * full["ms_per_step"]
    assert d["roofline"] is None and d["cpu_baseline"] is None and "secondary" not in d


def test_steps_must_be_positive():
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 2 and "--steps" in p.stderr


def test_dump_outputs(pkg, tmp_path, monkeypatch):
    """--dump-outputs: one float32 / float64 file per record field, integer fields exact; above DUMP_LIMIT the same seeded sample of
    records every time, its indices in index.npy, all files within the limit."""
    b = _bench()
    abi = pkg.abi
    rng = np.random.default_rng(7)
    rec = np.zeros(1000, dtype=abi.RESULT_DTYPE)
    rec.view(np.uint8)[:] = rng.integers(0, 256, rec.nbytes, dtype=np.uint8)
    b.dump_outputs(str(tmp_path / "all"), rec)
    assert sorted(os.listdir(tmp_path / "all")) == sorted(k + ".npy" for k in abi.RESULT_DTYPE.names)
    for k in abi.RESULT_DTYPE.names:
        got = np.load(tmp_path / "all" / (k + ".npy"))
        assert got.dtype == np.float64 and got.shape == rec[k].shape
        assert np.array_equal(got, rec[k].astype(np.float64), equal_nan=True)
    f32 = np.zeros(500, dtype=abi.RESULT_F32_DTYPE)
    f32["distance"], f32["status"] = rng.standard_normal(500), rng.integers(0, 2**32, 500, dtype=np.uint32)
    b.dump_outputs(str(tmp_path / "f32"), f32)
    assert np.load(tmp_path / "f32" / "distance.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "f32" / "status.npy"), f32["status"].astype(np.float64))
    # sampled: room for 100 fp64 records (112 B of fields + 8 B of index each) beside the 1 MB kept for headers
    monkeypatch.setattr(b, "DUMP_LIMIT", (1 << 20) + 100 * 120)
    for d in ("s1", "s2"):
        b.dump_outputs(str(tmp_path / d), rec)
        assert sum(os.path.getsize(tmp_path / d / f) for f in os.listdir(tmp_path / d)) <= b.DUMP_LIMIT
    idx = np.load(tmp_path / "s1" / "index.npy")
    assert len(idx) == 100 and np.all(np.diff(idx) > 0) and np.array_equal(idx, np.load(tmp_path / "s2" / "index.npy"))
    assert np.array_equal(np.load(tmp_path / "s1" / "p1.npy"), rec["p1"][idx.astype(np.int64)], equal_nan=True)


@pytest.mark.gpu
def test_plain_run_dumps_the_last_step(pkg, torch_cuda, tmp_path):
    """bench.py without --full: exactly --steps timed steps, no roofline or CPU baseline, and --dump-outputs holds the records the
    device entry point returns for the same seeded batch."""
    torch = torch_cuda
    env = dict(os.environ, HFCL_BENCH_FULL_DIR=str(tmp_path))
    for k in ("WORLD_SIZE", "RANK"):
        env.pop(k, None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--workload", "cfg3", "--pairs", "65537", "--steps", "2",
                        "--warmup", "1", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, env=env)
    assert p.returncode == 0, p.stderr[-3000:]
    d = json.loads(p.stdout.strip().splitlines()[-1])
    assert d["steps"] == 2 and d["ms_per_step"] > 0 and d["roofline"] is None and d["cpu_baseline"] is None
    abi, wl = pkg.abi, pkg.workloads
    bt = wl.cfg3_convex_convex(n=65537, seed=1)
    lib = wl.make_library(pkg, bt, device=0)
    dev = torch.device("cuda", 0)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    out = torch.zeros(len(bt) * 11, dtype=torch.int32, device=dev)
    lib.distance_device_f32(t(bt.s1.astype(np.int32)), t(bt.s2.astype(np.int32)), t(bt.pose1_f32), t(bt.pose2_f32), len(bt),
                            wl.make_request(bt, abi), out)
    torch.cuda.synchronize()
    want = out.cpu().numpy().view(abi.RESULT_F32_DTYPE)
    lib.close()
    for k in abi.RESULT_F32_DTYPE.names:
        got = np.load(tmp_path / "out" / (k + ".npy"))
        assert got.dtype == (np.float32 if k != "status" else np.float64)
        assert np.array_equal(got, want[k].astype(got.dtype), equal_nan=True), k
