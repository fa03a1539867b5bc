"""bench.py's output contract: the LAST stdout line is one compact strict-JSON object of at most 4 KB that
carries the contract's keys, `roofline` and `cpu_baseline`; the long per-workload records go on earlier lines.  Checked on
recorded results of real runs (profiles/*_bench_default.json: the long form the bench produced on the MI355X)."""
import glob
import json
import os

import pytest

from benchmarks import report

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = [p for p in sorted(glob.glob(os.path.join(REPO, "profiles", "r*_bench_default.json")) +
                              glob.glob(os.path.join(REPO, "profiles", "r*_bench_2rank_same_device.json")))
            if os.path.basename(p) >= "r05"]            # (earlier rounds' records predate `exchange` / per-slice parity)
DEFAULT = [p for p in RECORDED if p.endswith("_bench_default.json")]


def _load(path):
    """A recorded run: either the old one-line form or the new detail lines ({"detail": name, "record": {...}} ... compact)."""
    rows = [json.loads(ln) for ln in open(path).read().splitlines() if ln.strip().startswith("{")]
    details = [r for r in rows if "detail" in r and "record" in r]
    if details:
        head = dict(next(r["record"] for r in details if r["detail"] == "headline"))
        head["workloads"] = {r["detail"]: r["record"] for r in details if r["detail"] != "headline"}
        return head
    return max(rows, key=lambda r: len(json.dumps(r)))


def _strict(s):
    def bad(c):
        raise ValueError("non-strict JSON constant " + c)
    return json.loads(s, parse_constant=bad)


@pytest.mark.parametrize("path", RECORDED, ids=[os.path.basename(p) for p in RECORDED])
def test_final_line_is_compact_strict_json(path):
    res = _load(path)
    line = report.compact_line(res)
    assert "\n" not in line and len(line.encode()) < report.LINE_LIMIT
    out = _strict(line)
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in out, k
    assert out["config"]["workload"] and "model" not in out["config"] and out["config"]["value_definition"]
    roof = out["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in roof, k
    assert roof["bound"] in ("hbm", "mfma") and abs(roof["frac"] - roof["achieved"] / roof["peak"]) < 1e-3
    if res.get("cpu_baseline"):
        cpu = out["cpu_baseline"]
        assert cpu["kind"] in ("port", "reference") and cpu["cores"] >= 1 and cpu["value"] > 0 and cpu["sample"]
    assert abs(out["value"] - res["value"]) <= 1e-5 * abs(res["value"])
    for name, rec in (out.get("workloads") or {}).items():
        assert len(json.dumps({name: rec}, separators=(",", ":"))) <= report.SLICE_LIMIT, name
        assert "err" in rec or {"kms", "frac"} <= set(rec), (name, rec)
        assert "err" in rec or out["n_gpus"] > 1 or rec.get("par") == "ok", (name, rec)
    if out["n_gpus"] > 1:
        assert out["ranks"]["ranks_seen"] == out["n_gpus"] and "cross_check" in out["ranks"]
        assert {"row_bytes", "exchange_ms", "hidden_ms"} <= set(out["exchange"])


def test_detail_lines_cannot_be_mistaken_for_the_line():
    res = _load(DEFAULT[-1])
    for ln in report.detail_lines(res):
        rec = _strict(ln)
        assert set(rec) == {"detail", "record"}


def test_non_finite_numbers_do_not_reach_the_line():
    res = _load(DEFAULT[-1])
    res["roofline"]["traffic_frac"] = float("nan")
    res["value_roots4096"] = float("inf")
    res["workloads"] = dict(res.get("workloads") or {}, broken=dict(error="RuntimeError: " + "x" * 500))
    out = _strict(report.compact_line(res))
    assert out["roofline"]["traffic_frac"] is None and "value_roots4096" not in out or out["value_roots4096"] is None
    assert len(out["workloads"]["broken"]["err"]) <= 80


def test_line_degrades_instead_of_growing():
    res = _load(DEFAULT[-1])
    base = dict(next(iter(res["workloads"].values())))
    res["workloads"] = dict(res["workloads"], **{"extra_slice_number_{}".format(i): base for i in range(12)})
    line = report.compact_line(res)
    assert len(line) <= report.LINE_LIMIT
    assert len(_strict(line)["workloads"]) == len(res["workloads"])


def test_plain_run_line_carries_the_headline_only():
    """A plain run (no --full) has no roofline, baseline or slices: its line still carries the contract's headline keys."""
    res = dict(metric="rollout env-steps/sec (UCT plan(), budget=1000)", unit="env-steps/s", value=1.5e11, ms_per_step=0.79,
               dtype="f64", n_gpus=1, steps=20, warmup=3, higher_is_better=True, scaling="weak", vs_baseline=None,
               config=dict(workload="uct_highway_shaped", value_definition_short="device-resident"), cpu_baseline=None)
    out = _strict(report.compact_line(res))
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup"):
        assert out[k] == res[k], k
    assert out["roofline"] is None and out["cpu_baseline"] is None and "workloads" not in out and "detail" not in out


def _bench_module():
    import importlib.util
    spec = importlib.util.spec_from_file_location("bench_driver", os.path.join(REPO, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_full_is_off_by_default(monkeypatch):
    bench = _bench_module()
    monkeypatch.setattr("sys.argv", ["bench.py", "--steps", "7", "--warmup", "2"])
    args = bench.parse()
    assert args.steps == 7 and args.warmup == 2 and not args.full and args.dump_outputs is None
    assert args.headline_only and args.no_cpu_baseline and args.no_parity_sample
    monkeypatch.setattr("sys.argv", ["bench.py", "--full", "--dump-outputs", "d"])
    args = bench.parse()
    assert args.full and args.dump_outputs == "d" and not (args.headline_only or args.no_cpu_baseline or args.no_parity_sample)


def test_dump_outputs_float_files_within_the_limit(tmp_path, monkeypatch):
    import numpy as np
    bench = _bench_module()
    monkeypatch.setattr(bench, "DUMP_LIMIT", 1 << 20)          # (the sampling path, on small arrays)
    plans = np.arange(40, dtype=np.int32).reshape(10, 4)
    bench.dump_outputs(str(tmp_path / "small"), dict(plans=plans, value=np.linspace(0, 1, 10), f=np.ones(3, np.float32)))
    got = {p.stem: np.load(p) for p in (tmp_path / "small").iterdir()}
    assert set(got) == {"plans", "value", "f"} and got["plans"].dtype == np.float64 and got["f"].dtype == np.float32
    assert np.array_equal(got["plans"], plans) and np.array_equal(got["value"], np.linspace(0, 1, 10))
    # beyond the limit: the same seeded rows of every array of the batch's length, and their indices
    n = 3 * bench.DUMP_LIMIT // 16
    big = dict(a=np.arange(n, dtype=np.int64), b=np.arange(n, dtype=np.float64) * 0.5, c=np.ones(5))
    for d in ("big1", "big2"):
        bench.dump_outputs(str(tmp_path / d), big)
    files = list((tmp_path / "big1").iterdir())
    assert sum(p.stat().st_size for p in files) <= bench.DUMP_LIMIT
    rows = np.load(tmp_path / "big1" / "sample_rows.npy").astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "big1" / "a.npy"), rows) and np.array_equal(np.load(tmp_path / "big1" / "b.npy"), rows * 0.5)
    assert np.array_equal(rows, np.load(tmp_path / "big2" / "sample_rows.npy").astype(np.int64))
    assert np.load(tmp_path / "big1" / "c.npy").shape == (5,)
