"""The bench line the driver parses (bench.py compact_line): bounded size, the contract's headline fields.

r03's line carried every sweep and reached 23.4 KB; the driver returned it unparsed.  These tests rebuild
the line from the full r03 record (profiles/r03/bench_default_final.json, the same shape bench.py now
writes to its detail file) and from a synthetic worst case, and hold it under the budget."""
import copy
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT))

import bench  # noqa: E402

R03 = ROOT / "profiles" / "r03" / "bench_default_final.json"
HEADLINE = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
            "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline", "recall_at_10")


def _full():
    return json.loads(R03.read_text().strip().splitlines()[-1])


def test_compact_line_from_r03_record_fits_and_keeps_headline():
    full = _full()
    assert len(json.dumps(full)) > 20000  # the record that did not parse
    line = bench.compact_line(full)
    s = json.dumps(line)
    assert len(s) < bench.LINE_BUDGET < 12000
    for k in HEADLINE:
        assert k in line, k
    assert line["value"] == full["value"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "kernel_ms", "frac_vs_survey_bytes"):
        assert k in line["roofline"], k
    for k in ("value", "unit", "cores", "kind"):
        assert k in line["cpu_baseline"], k
    cfg = line["configs"]
    assert cfg["C2_flat_l2_1m_768"]["value"] == full["configs"]["C2_flat_l2_1m_768"]["value"]
    assert cfg["C5_flat_ip_100m_768_sharded"]["frac"] == full["configs"]["C5_flat_ip_100m_768_sharded"]["roofline"]["frac"]
    assert cfg["C4_diskann_1m_1536_sq8"]["kernel_ms"] > 0
    json.loads(s)  # one parseable line


def test_compact_line_worst_case_stays_under_budget():
    """Twice as many configs, with long error strings: the fallback trims to the core fields."""
    full = _full()
    big = copy.deepcopy(full)
    for name, c in list(full["configs"].items()):
        c2 = copy.deepcopy(c)
        c2["error"] = "x" * 5000
        big["configs"][name + "_copy"] = c2
    s = json.dumps(bench.compact_line(big))
    assert len(s) < 12000


def test_emit_writes_detail_and_prints_one_line(tmp_path, capsys, monkeypatch):
    monkeypatch.setattr(bench, "DETAIL_PATH", tmp_path / "detail.json")
    full = _full()
    bench.emit(full, 0)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    assert json.loads(out[0])["value"] == full["value"]
    assert json.loads((tmp_path / "detail.json").read_text())["configs"].keys() == full["configs"].keys()
    bench.emit(full, 1)  # other ranks print nothing
    assert capsys.readouterr().out == ""


def test_plain_run_line_has_no_detail_file(tmp_path, capsys, monkeypatch):
    """A plain run (no --full) prints the line alone: nothing is written, the line names no detail file."""
    monkeypatch.setattr(bench, "DETAIL_PATH", tmp_path / "detail.json")
    full = _full()
    bench.emit(full, 0, detail=False)
    out = capsys.readouterr().out.strip().splitlines()
    assert len(out) == 1
    line = json.loads(out[0])
    assert "detail" not in line and not (tmp_path / "detail.json").exists()
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert line[k] == full[k], k


def test_plain_run_measures_only_the_headline(monkeypatch):
    """Without --full every extra measurement is off, whatever the other options say; --full keeps the defaults."""
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2", "--suite"])
    a = bench.parse()
    assert (a.full, a.suite, a.no_c5, a.no_cpu_baseline, a.no_alt_forms) == (False, False, True, True, True)
    assert (a.steps, a.warmup, a.dump_outputs) == (7, 2, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full"])
    a = bench.parse()
    assert (a.full, a.suite, a.no_c5, a.no_cpu_baseline, a.no_alt_forms) == (True, True, False, False, False)


def test_dump_outputs_writes_float_arrays(tmp_path, monkeypatch):
    import numpy as np

    monkeypatch.setattr(sys, "argv", ["bench.py", "--dump-outputs", str(tmp_path / "o")])
    a = bench.parse()
    D = np.arange(12, dtype=np.float32).reshape(4, 3)
    I = np.array([[2**40 + 1, -1, 5]] * 4, np.int64)
    bench.dump_outputs(a, 1, D, I)  # other ranks write nothing
    assert not (tmp_path / "o").exists()
    bench.dump_outputs(a, 0, D, I)
    d, i = np.load(tmp_path / "o" / "distances.npy"), np.load(tmp_path / "o" / "labels.npy")
    assert d.dtype == np.float32 and i.dtype == np.float64
    assert np.array_equal(d, D) and np.array_equal(i.astype(np.int64), I)
