"""bench.py's command line: a plain run measures the DDPG headline only, --full adds the CPU baseline and the sub-records,
--dump-outputs writes what the last timed step computed (seeded inputs: two runs give the same arrays)."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAPS = ("q", "y", "a_out", "dqda")


class _StubDDPG(object):
    """what bench.dump_outputs() reads from a population: taps, parameter blobs, beta powers"""
    def __init__(self, n_agents, B=100, A=1, P=81802):
        self.n_agents, self.B, self.A, self.P = n_agents, B, A, P

    def last_tap(self, agent, which):
        n = self.B * self.A if which in ("a_out", "dqda") else self.B
        return np.full(n, 1000 * agent + TAPS.index(which), np.float32)

    def get_blob(self, agent, which):
        return np.full(self.P, agent + (0.5 if which == "theta_target" else 0.0), np.float32)

    def get_beta_powers(self, agent):
        return np.full(4, agent, np.float32)


def test_dump_outputs_names_shapes_sample_and_budget(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    shapes = bench.dump_outputs(_StubDDPG(256), str(tmp_path))
    assert shapes["q"] == shapes["y"] == (256, 100) and shapes["a_out"] == shapes["dqda"] == (256, 100, 1)
    k = bench.DUMP_PARAM_AGENTS
    assert shapes["theta"] == shapes["theta_target"] == (k, 81802) and shapes["beta_powers"] == (256, 4)
    total = 0
    for name in shapes:
        v = np.load(str(tmp_path / (name + ".npy")))
        assert v.dtype == np.float32 and v.shape == shapes[name], name
        total += v.nbytes
    assert total <= 64 * 2 ** 20
    # every agent's taps, in agent order; the parameter sample is sorted, fixed and matches its rows
    q = np.load(str(tmp_path / "q.npy"))
    assert np.array_equal(q[:, 0], 1000.0 * np.arange(256))
    sample = np.load(str(tmp_path / "sample_agents.npy"))
    assert np.all(np.diff(sample) > 0) and len(set(sample.tolist())) == k
    assert np.array_equal(np.load(str(tmp_path / "theta.npy"))[:, 0], sample)
    assert np.array_equal(np.load(str(tmp_path / "theta_target.npy"))[:, 0], sample + 0.5)
    again = tmp_path / "again"
    bench.dump_outputs(_StubDDPG(256), str(again))
    assert np.array_equal(np.load(str(again / "sample_agents.npy")), sample)
    # fewer agents than the sample size: all of them
    small = tmp_path / "small"
    assert bench.dump_outputs(_StubDDPG(5), str(small))["theta"] == (5, 81802)


def test_dump_outputs_refuses_more_than_64_mb(tmp_path):
    sys.path.insert(0, ROOT)
    import bench
    with pytest.raises(ValueError, match="budget"):
        bench.dump_outputs(_StubDDPG(8, P=2 ** 20), str(tmp_path))


def _run_bench(clean_launcher, args, timeout=600):
    rep = clean_launcher([sys.executable, os.path.join(ROOT, "bench.py")] + args, timeout=timeout)
    assert rep["rc"] == 0, rep["stderr"][-3000:]
    return json.loads([l for l in rep["stdout"].splitlines() if l.startswith("{")][-1])


SMALL = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--agents", "8", "--updates-per-step", "4"]


@pytest.mark.gpu
def test_plain_bench_is_lean_and_its_outputs_repeat(clean_launcher, tmp_path):
    outs = []
    for run in ("a", "b"):
        d = tmp_path / run
        res = _run_bench(clean_launcher, SMALL + ["--dump-outputs", str(d)])
        assert res["steps"] == 3 and res["warmup"] == 1 and res["ms_per_step"] > 0
        assert res["config"]["updates_timed_per_agent"] == 4 * 3
        assert abs(res["value"] - 8 * 4 * 3 / (res["ms_per_step"] * 3e-3)) < 1e-6 * res["value"]
        assert res["unit"] == "gradient updates/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
        assert res["full"] is False and res["cpu_baseline"] is None
        assert not set(res) & {"sac", "naf", "kl", "ddpg_separate"}
        outs.append({n: np.load(str(d / (n + ".npy"))) for n in TAPS + ("theta", "theta_target", "beta_powers")})
    a, b = outs
    assert a["q"].shape == (8, 100) and a["theta"].shape[0] == 8
    for name in a:
        assert a[name].dtype == np.float32 and np.all(np.isfinite(a[name])), name
        assert np.array_equal(a[name], b[name]), name                 # same arguments, same inputs, same results


@pytest.mark.gpu
def test_full_bench_keeps_the_baseline_and_the_sub_records(clean_launcher):
    res = _run_bench(clean_launcher, SMALL + ["--full", "--cpu-seconds", "1", "--cpu-records", "2000"], timeout=900)
    assert res["full"] is True and res["cpu_baseline"]["value"] > 0
    for algo in ("sac", "naf", "kl", "ddpg_separate"):
        assert res[algo]["value"] > 0 and res[algo]["steps"] == 3, algo
