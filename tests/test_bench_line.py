"""bench.py's output contract (CPU): the driver parses the LAST stdout line and keeps only an ~8 KB tail of
stdout, so the final line must be a compact JSON headline that carries the metric, roofline and cpu_baseline
(round 4's single 21 KB line did not parse). Built here from a recorded full bench result."""
import json
import os
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)

RECORD = os.path.join(ROOT, "profiles", "r04", "r04a5_bench.json")


def _record():
    if not os.path.exists(RECORD):
        pytest.skip("recorded bench result not present")
    return json.load(open(RECORD))


def test_headline_under_cap_and_round_trips():
    import bench
    line = _record()
    text = bench.headline_record(dict(line, full_record="gpurun_out/bench_full.json"))
    assert "\n" not in text
    assert len(text.encode()) < bench.HEADLINE_MAX_BYTES
    rec = json.loads(text)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "dtype", "config",
              "roofline", "cpu_baseline"):
        assert k in rec, k
    assert rec["value"] == pytest.approx(line["value"], rel=1e-4)
    for k in ("kernel_ms", "ops_per_unit", "units_per_launch", "frac", "traffic", "peak", "achieved"):
        assert k in rec["roofline"], k
    assert rec["roofline"]["frac"] == pytest.approx(rec["roofline"]["achieved"] / rec["roofline"]["peak"], rel=1e-3)
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in rec["cpu_baseline"], k
    legs = rec["secondary_summary"]
    assert len(legs) == len(line["secondary"])
    assert all("value" in s for s in legs)


def test_headline_drops_optional_parts_past_the_cap():
    import bench
    line = _record()
    # a pathological record: many large legs; the mandatory fields still fit and parse
    line = dict(line, secondary=line["secondary"] * 40)
    text = bench.headline_record(line)
    assert len(text.encode()) < bench.HEADLINE_MAX_BYTES
    rec = json.loads(text)
    assert "roofline" in rec and "cpu_baseline" in rec and "secondary_summary" not in rec


def test_dump_outputs_writes_float64_and_samples_past_the_cap(tmp_path, monkeypatch):
    import numpy as np

    import bench
    from namazu_amd import _lib
    st = np.zeros(1000, _lib.SCHED_STATS_DTYPE)
    st["sum_delay_ns"] = np.arange(1000, dtype=np.uint64) * np.uint64(1 << 30)
    st["first_fault"] = 0xFFFFFFFF
    tk = np.zeros(64, _lib.TOPK_DTYPE)
    tk["seed"] = np.arange(64)[::-1]
    bench.dump_outputs(str(tmp_path / "a"), {"last_step_stats": st, "job_topk": tk})
    a = np.load(tmp_path / "a" / "last_step_stats.npy")
    assert a.dtype == np.float64 and a.shape == (1000, 6)
    assert np.array_equal(a[:, 0].astype(np.uint64), st["sum_delay_ns"]) and (a[:, 4] == 0xFFFFFFFF).all()
    t = np.load(tmp_path / "a" / "job_topk.npy")
    assert t.dtype == np.float64 and t.shape == (64, 4) and t[:, 0].tolist() == tk["seed"].tolist()
    assert sorted(os.listdir(tmp_path / "a")) == ["job_topk.npy", "last_step_stats.npy"]
    # past the cap: the same fixed rows every time, everything together under the cap
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 20_000)
    for d in ("b", "c"):
        bench.dump_outputs(str(tmp_path / d), {"last_step_stats": st, "job_topk": tk})
    rows = np.load(tmp_path / "b" / "last_step_stats_rows.npy")
    b = np.load(tmp_path / "b" / "last_step_stats.npy")
    assert 100 < len(rows) < 1000 and (np.diff(rows) > 0).all()
    assert np.array_equal(b, a[rows.astype(np.int64)])
    assert np.array_equal(np.load(tmp_path / "b" / "job_topk.npy"), t)
    assert np.array_equal(rows, np.load(tmp_path / "c" / "last_step_stats_rows.npy"))
    assert sum(np.load(tmp_path / "b" / f).nbytes for f in os.listdir(tmp_path / "b")) <= 20_000


@pytest.mark.gpu
def test_plain_run_times_the_headline_only_and_dumps_its_last_step(tmp_path):
    """`bench.py --gpus 1 --steps K --warmup W` (no --full): the result line carries the headline fields and none
    of the --full parts, writes no full record, and --dump-outputs holds the last timed step's statistics and
    top-64 and the job's top-64, all equal to the oracle's on the same seeds (small shape: 3 steps of 4,096 seeds
    over 256 events)."""
    import subprocess

    import numpy as np

    import bench
    from namazu_amd.explorepolicy import to_csr
    from oracle import oracle as O
    S, E, K = 4096, 256, 3
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K),
                        "--warmup", "1", "--seeds", str(S), "--events", str(E), "--dump-outputs", "dump"],
                       capture_output=True, text=True, timeout=300, cwd=tmp_path)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1
    rec = json.loads(lines[0])
    assert rec["metric"] and rec["unit"] == "decisions/s" and rec["higher_is_better"] is True and rec["dtype"] == "u64"
    assert rec["steps"] == K and rec["warmup"] == 1 and rec["ms_per_step"] > 0
    assert rec["value"] == pytest.approx(S * E / (rec["ms_per_step"] * 1e-3), rel=1e-3)
    for k in ("roofline", "cpu_baseline", "end_to_end", "secondary_summary", "full_record"):
        assert k not in rec, k
    assert sorted(os.listdir(tmp_path)) == ["dump"]
    hoff, hb = to_csr(bench.zk_hints(E))
    soff, sb = bench.decimal_csr(0, K * S)
    st, _ = O.replayable_sweep(soff, sb, hoff, hb, bench.MAX_INTERVAL_NS)
    lo = (K - 1) * S
    got = np.load(tmp_path / "dump" / "last_step_stats.npy")
    assert got.dtype == np.float64 and got.shape == (S, 6)
    assert np.array_equal(got, bench.records_f64(st[lo:]))
    assert np.array_equal(np.load(tmp_path / "dump" / "last_step_topk.npy"),
                          bench.records_f64(O.topk_from_stats(st[lo:], lo, 64)))
    assert np.array_equal(np.load(tmp_path / "dump" / "job_topk.npy"), bench.records_f64(O.topk_from_stats(st, 0, 64)))


def test_write_final_last_line(tmp_path):
    import bench
    line = _record()
    r, w = os.pipe()
    bench.write_final(w, line, str(tmp_path / "full.json"))
    os.close(w)
    out = os.read(r, 1 << 20).decode()
    os.close(r)
    assert out.endswith("\n") and out.count("\n") == 1
    rec = json.loads(out.strip())
    assert rec["full_record"].endswith("full.json")
    full = json.load(open(tmp_path / "full.json"))
    assert full["secondary"] == line["secondary"]
