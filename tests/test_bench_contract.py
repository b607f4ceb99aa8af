"""bench.py prints ONE JSON line with the fields the driver and the judge read; --dump-outputs writes what the timed
steps computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_json_contract(built):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "3", "--warmup", "1", "--systems", "4000",
                          "--cpu-sample", "2000", "--full"], capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config", "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["n_gpus"] == 1 and d["steps"] == 3 and d["warmup"] == 1
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None
    assert d["dtype"] == "f64" and d["data"] == "synthetic" and "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 1e5  # the north-star's floor: 1e5 converged 32-constraint systems per second
    r = d["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12 and "traffic" in r
    # the fraction is quoted on bytes that move: it cannot exceed what a streaming copy reaches on this part, and it agrees
    # with the counters' bytes over the same time
    assert r["frac_of_streaming_copy_rate"] <= 1.0
    assert r["algorithmic_bytes_per_system"] == 1920 and r["by_survey_8d_bytes"]["bytes_per_system"] == 2560
    if r["traffic"] is not None:
        assert abs(r["frac"] - r["frac_by_counter_bytes"]) <= 0.05 * r["frac_by_counter_bytes"]
    assert r["mixed_structure"]["algorithmic_bytes_per_system"] == 2560 and r["mixed_structure"]["frac"] <= 1.0
    c = d["cpu_baseline"]
    assert c["kind"] in ("port", "reference") and c["cores"] >= 1 and c["value"] > 0 and c["sample"]


def _plain_run(dump_dir, steps):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1",
                          "--systems", "4000", "--dump-outputs", str(dump_dir)], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_only_and_dumps_what_its_last_step_computed(built, tmp_path):
    d = _plain_run(tmp_path / "a", 3)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "solve_kernel"):
        assert k in d, k
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "f64"
    for k in ("roofline", "cpu_baseline", "host_path", "step_solvers", "other_workloads"):  # --full only
        assert k not in d, k
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")}
    assert {"vars", "systems", "result_sse_unscaled", "result_accepted", "result_trials"} <= set(a)
    assert all(v.dtype == np.float64 for v in a.values())
    assert sum(v.nbytes for v in a.values()) <= 64 << 20
    assert a["vars"].shape == (4000 * 32,) and np.array_equal(a["systems"], np.arange(4000))
    # the records are the timed steps' own: the line's counters come from the same Systems
    assert np.count_nonzero(a["result_sse_unscaled"] < 1e-4) / 4000 == d["converged_fraction"]
    # same arguments, same inputs: a second run (other step count) computes the same outputs bit for bit
    _plain_run(tmp_path / "b", 2)
    for name, v in a.items():
        assert np.array_equal(np.load(tmp_path / "b" / (name + ".npy")).view(np.uint64), v.view(np.uint64)), name


def test_dump_outputs_samples_a_batch_past_the_budget(fiksi, tmp_path):
    import bench

    rng = np.random.default_rng(7)
    lens = rng.integers(1, 40, size=3000)
    var_off = np.concatenate([[0], np.cumsum(lens)])
    vars_ = rng.standard_normal(int(var_off[-1]))
    res = np.zeros(3000, dtype=fiksi.abi.RESULT_DTYPE)
    res["trials"] = np.arange(3000)
    res["sse"] = rng.random(3000)
    bench.dump_outputs(str(tmp_path / "all"), vars_, var_off, res)
    assert np.array_equal(np.load(tmp_path / "all" / "vars.npy"), vars_)
    assert np.array_equal(np.load(tmp_path / "all" / "result_trials.npy"), np.arange(3000))
    budget = 100_000
    for run in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / run), vars_, var_off, res, budget=budget)
    files = sorted(os.listdir(tmp_path / "s1"))
    assert files == sorted(os.listdir(tmp_path / "all"))
    a = {f: np.load(tmp_path / "s1" / f) for f in files}
    assert all(v.dtype == np.float64 for v in a.values())
    assert budget - 8 * 50 < sum(v.nbytes for v in a.values()) <= budget
    idx = a["systems.npy"].astype(np.int64)
    assert np.all(np.diff(idx) > 0) and 0 < len(idx) < 3000
    assert np.array_equal(a["vars.npy"], np.concatenate([vars_[var_off[i]:var_off[i + 1]] for i in idx]))
    assert np.array_equal(a["result_trials.npy"], idx) and np.array_equal(a["result_sse.npy"], res["sse"][idx])
    for f in files:  # a fixed sample: the same Systems every time
        assert np.array_equal(np.load(tmp_path / "s2" / f), a[f])


def test_bench_runs_on_a_built_tree_it_cannot_write_in(capsys):
    """build() opens a lock file in the tree; a tree built beforehand may be read-only to the user who benchmarks it."""
    import bench

    class ReadOnlyTree:
        @staticmethod
        def build():
            raise PermissionError(13, "Permission denied", ".build.lock")

    class NoCompiler:
        @staticmethod
        def build():
            raise RuntimeError("fiksi_amd/libfiksi_amd.so is missing and there is no hipcc to build it with")

    bench.build_or_use_built(ReadOnlyTree)
    assert "using the native code already built" in capsys.readouterr().err
    with pytest.raises(RuntimeError):  # any other failure of the build still ends the run
        bench.build_or_use_built(NoCompiler)
