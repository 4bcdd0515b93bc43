"""bench.py's plain and --full runs and --dump-outputs, on the CPU (gloo)
rehearsal path of the harness: what a plain run leaves out, that the extras
refuse to run without --full, and that two runs with the same arguments dump
the same arrays."""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_modes_mod", os.path.join(REPO, "bench.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    return b


def test_plain_run_leaves_the_extras_out(bench):
    a = bench.parse_args(["--gpus", "1", "--steps", "7", "--warmup", "2"])
    assert (a.steps, a.warmup, a.full) == (7, 2, False)
    assert a.skip_baseline and a.no_agent_baseline == "off" and a.host_pmu == "off" and a.comm_trace == "off"
    # switching an extra off by name is not asking for it
    a = bench.parse_args(["--host-pmu", "off", "--no-agent-baseline", "off", "--comm-trace", "off"])
    assert a.skip_baseline and a.host_pmu == "off"


def test_full_run_keeps_todays_defaults(bench):
    a = bench.parse_args(["--full"])
    assert not a.skip_baseline and a.no_agent_baseline == "auto" and a.host_pmu == "auto" and a.comm_trace == "auto"
    a = bench.parse_args(["--full", "--host-pmu", "off", "--no-agent-baseline", "off", "--kernel-breakdown"])
    assert a.host_pmu == "off" and a.no_agent_baseline == "off" and a.kernel_breakdown


@pytest.mark.parametrize("extra", [["--kernel-breakdown"], ["--sweep-hz", "100,0"], ["--overhead-matrix", "core,lite"],
                                   ["--child-probe", "1"], ["--no-agent-baseline", "on"], ["--host-pmu", "auto"],
                                   ["--comm-trace", "on"]])
def test_extras_need_full(bench, extra, capsys):
    with pytest.raises(SystemExit) as e:
        bench.parse_args(extra)
    assert e.value.code == 2
    assert extra[0] in capsys.readouterr().err
    assert bench.parse_args(["--full"] + extra).full


def test_overhead_matrix_runs_its_entries_with_full(bench, monkeypatch):
    """Each matrix entry is a headline run with its A/B windows and no-agent
    children: it is started with --full."""
    seen = []

    def fake_run(cmd, **kw):
        seen.append(cmd)
        return subprocess.CompletedProcess(cmd, 1)
    monkeypatch.setattr(subprocess, "run", fake_run)
    monkeypatch.setattr(bench, "run_baseline_child", lambda *a, **k: {"tag": "countable"})
    args = bench.parse_args(["--full", "--overhead-matrix", "core,lite@kb", "--steps", "2"])
    assert bench.run_overhead_matrix(args) == 0
    assert len(seen) == 2 and all("--full" in c for c in seen)
    bench.parse_args(seen[1][2:])  # the entry's own command line parses (--kernel-breakdown with --full)


def _run(tmp_path, name, *more):
    out = tmp_path / name
    cmd = [sys.executable, os.path.join(REPO, "bench.py"), "--device", "cpu", "--model", "tiny", "--micro-batch", "2",
           "--seq-len", "64", "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(out), *more]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=120, env=dict(os.environ, OMP_NUM_THREADS="1"),
                       cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f: np.load(out / f) for f in sorted(os.listdir(out))}


def test_dump_outputs_repeat_exactly(bench, tmp_path):
    """Same arguments, same inputs: on the CPU path (no atomics, one thread)
    two runs dump identical arrays.  The dump is float32, holds the last
    timed step's loss, a fixed sample of its logits and of every parameter,
    and stays far below 64 MB."""
    res1, d1 = _run(tmp_path, "a")
    res2, d2 = _run(tmp_path, "b")
    assert sorted(d1) == ["logits_sample.npy", "loss.npy", "params_sample.npy"] == sorted(d2)
    for f in d1:
        assert d1[f].dtype == np.float32 and np.isfinite(d1[f]).all(), f
        assert d1[f].shape == d2[f].shape and (d1[f] == d2[f]).all(), f
    assert sum(a.nbytes for a in d1.values()) < 64 * 2 ** 20
    # tiny at batch 2 x 64: the whole logits tensor fits the sample, in order
    from dynolog_amd.models.llama import CONFIGS
    assert d1["logits_sample.npy"].shape == (min(2 * 64 * CONFIGS["tiny"].vocab_size, bench.DUMP_LOGITS_SAMPLE),)
    assert d1["loss.npy"].shape == (1,) and abs(float(d1["loss.npy"][0]) - res1["loss"]) < 1e-3
    for res in (res1, res2):
        assert res["steps"] == 3 and res["ms_per_step"] > 0 and res["config"]["full"] is False
        for key in ("metric", "value", "unit", "higher_is_better", "dtype"):
            assert key in res
    assert np.std(d1["params_sample.npy"]) > 0 and np.std(d1["logits_sample.npy"]) > 0
