"""The Bimodal toy environments on the host (CPU only) against what the reference itself recorded
(tests/golden/bimodal_envs.json, written by tests/golden/make_bimodal_golden.py from the reference's
environments/environments.py:158-912).

The host classes use the reference's scalar functions in the reference's expression order on float64, so every
recorded reset and step is compared for BIT equality -- no tolerance.
"""
import json
import os
import struct

import numpy as np
import pytest

from rlcontrol_amd.environments import bimodal
from rlcontrol_amd.environments.environments import create_environment
from rlcontrol_amd.experiment import Experiment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "bimodal_envs.json")) as _f:
    GOLD = json.load(_f)["envs"]
NAMES_1D = [n for n in GOLD if n != "Bimodal2DEnv"]
ATTRS = ["name", "eval_interval", "eval_episodes", "TOTAL_STEPS_LIMIT", "EPISODE_STEPS_LIMIT", "state_dim", "state_min",
         "state_max", "state_range", "state_bounded", "action_dim", "action_min", "action_max", "action_range"]


def bits(x):
    return [struct.pack("<d", float(v)) for v in np.asarray(x, np.float64).reshape(-1)]


def ulps(a, b):
    ia, ib = struct.unpack("<q", struct.pack("<d", float(a)))[0], struct.unpack("<q", struct.pack("<d", float(b)))[0]
    return abs(ia - ib)


def plain(v):
    return v.tolist() if isinstance(v, np.ndarray) else v


def test_fixture_covers_the_eight_environments():
    assert sorted(GOLD) == sorted(bimodal.NAMES) and len(NAMES_1D) == 7
    for name in NAMES_1D:
        acts = np.array([s[0] for s in GOLD[name]["steps"]])
        assert len(acts) >= 190 and np.array_equal(acts, acts.astype(np.float32).astype(np.float64))
        m1, m2 = bimodal.BIMODAL_1D[name][:2]
        for must in (-2.0, 2.0, 0.0, np.float32(m1), np.float32(m2)):
            assert float(must) in acts, (name, must)
        assert acts.min() < -2.0 and acts.max() > 2.0
    traj = GOLD["Bimodal2DEnv"]["trajectories"]
    ends = {k: v[-1] for k, v in traj.items()}
    assert ends["into_upper_goal"][3] and ends["into_lower_goal"][3] and ends["oblique_into_lower_goal"][3]
    assert not any(s[3] for s in traj["never_terminates"]) and not any(s[3] for s in traj["into_the_wall"])
    assert ends["into_the_wall"][1] == [6.0, -6.0]                     # the clip was active


@pytest.mark.parametrize("name", sorted(GOLD))
def test_dispatch_and_attributes(name):
    rec = GOLD[name]
    env = create_environment(rec["env_json"])
    assert type(env) is (bimodal.Bimodal2DEnvironment if name == "Bimodal2DEnv" else bimodal.Bimodal1DEnvironment)
    for k in ATTRS:
        got, want = plain(getattr(env, k)), rec["attrs"][k]
        assert got == want and type(got) is type(want), (k, got, want)
    assert create_environment(dict(rec["env_json"], EpisodeSteps=-1)).EPISODE_STEPS_LIMIT == rec["episode_steps_limit_default"]
    assert bits(env.reset()) == bits(rec["reset"])
    env.set_random_seed(5)
    env.close()


@pytest.mark.parametrize("name", NAMES_1D)
def test_1d_steps_are_bit_equal(name):
    env = create_environment(GOLD[name]["env_json"])
    worst = 0
    for a, s2, r, done in GOLD[name]["steps"]:
        env.reset()
        gs2, gr, gdone, info = env.step(np.array([a]))
        worst = max(worst, ulps(gr, r))
        assert bits(gs2) == bits(s2) and gdone is True and done is True and info == {}
        assert isinstance(gr, float)
    print("worst reward distance for %s: %d ulp" % (name, worst))
    assert worst == 0


def test_2d_trajectories_are_bit_equal():
    env = create_environment(GOLD["Bimodal2DEnv"]["env_json"])
    worst = 0
    for tname, steps in GOLD["Bimodal2DEnv"]["trajectories"].items():
        assert bits(env.reset()) == bits([0.0, 0.0])
        for a, s2, r, done in steps:
            gs2, gr, gdone, _ = env.step(np.array(a))
            worst = max(worst, ulps(gr, r))
            assert bits(gs2) == bits(s2) and bool(gdone) is done, tname
    print("worst 2-D reward distance: %d ulp" % worst)
    assert worst == 0


def test_unknown_name_still_needs_gym():
    with pytest.raises(RuntimeError, match="needs gym"):
        create_environment({"environment": "Bimodal3DEnv", "TotalMilSteps": 1, "EpisodeSteps": -1,
                            "EvalIntervalMilSteps": 1, "EvalEpisodes": 1})


def test_shipped_json_files_match_the_recorded_settings():
    """the seven 1-D files carry the reference's step budgets; Bimodal2DEnv.json is the project's own (the fixture was
    generated from it, so this also catches an edit that forgot to regenerate)"""
    for name, rec in GOLD.items():
        with open(os.path.join(ROOT, "jsonfiles", "environment", name + ".json")) as fh:
            shipped = json.load(fh)
        assert shipped == rec["env_json"], name


def test_device_names_cover_the_host_names():
    from rlcontrol_amd import _lib
    assert set(bimodal.NAMES) <= set(_lib.ENV_IDS) and len(set(_lib.ENV_IDS.values())) == len(_lib.ENV_IDS)
    assert all(_lib.ENV_DEFAULT_EPISODE_STEPS[n] == GOLD[n]["episode_steps_limit_default"] for n in bimodal.NAMES)
    assert _lib.ENV_IDS["Pendulum-v0"] == 1 and _lib.ENV_DEFAULT_EPISODE_STEPS["Pendulum-v0"] == 200


def test_helper_environments_equal_the_fixture():
    """tests/helpers/bimodal_rollout.py (the CPU restatement the GPU tests compare with) on the same fixture"""
    from helpers.bimodal_rollout import VARIANTS_1D, make_env
    assert [n for n, _ in VARIANTS_1D] == NAMES_1D == list(bimodal.BIMODAL_1D)
    assert all(tuple(c) == tuple(bimodal.BIMODAL_1D[n]) for n, c in VARIANTS_1D)
    for name in NAMES_1D:
        env = make_env(name)
        for a, s2, r, done in GOLD[name]["steps"]:
            assert bits(env.reset()) == bits([0.0])
            gs2, gr, gdone = env.step(np.array([a], np.float32))
            assert bits(gs2) == bits(s2) and bits(gr) == bits(r) and gdone is True
    env = make_env("Bimodal2DEnv")
    for steps in GOLD["Bimodal2DEnv"]["trajectories"].values():
        env.reset()
        for a, s2, r, done in steps:
            gs2, gr, gdone = env.step(np.array(a, np.float32))
            assert bits(gs2) == bits(s2) and bits(gr) == bits(r) and gdone is done


class StubAgent(object):
    def __init__(self):
        self.updates, self.evals_at, self.n_updates = [], [], 0

    def start(self, s, is_train):
        if not is_train:
            self.evals_at.append(self.n_updates)
        return np.array([0.75])

    def step(self, s, is_train):
        raise AssertionError("a one-step episode never asks for a second action")

    def update(self, s, s2, r, a, done, truncated):
        self.n_updates += 1
        self.updates.append((float(s[0]), float(s2[0]), r, done, truncated))

    def reset(self):
        pass


def test_experiment_on_bimodal1d_stores_every_transition():
    """experiment.py:122-125: the 1-D family is exempt from the truncation rule although done coincides with the limit"""
    rec = GOLD["Bimodal1DEnv"]
    agent = StubAgent()
    out = Experiment(agent, create_environment(rec["env_json"]), create_environment(rec["env_json"]), seed=0,
                     verbose=False).run()
    total, interval, episodes = int(rec["attrs"]["TOTAL_STEPS_LIMIT"]), int(rec["attrs"]["eval_interval"]), rec["attrs"]["eval_episodes"]
    assert len(agent.updates) == total
    want_r = [s[2] for s in rec["steps"] if s[0] == 0.75][0]
    assert all(u == (0.0, 0.75, want_r, True, False) for u in agent.updates)
    train_rewards, eval_rewards, train_steps, eval_steps, ts_at_eval = out[:5]
    assert train_steps == [1] * total and out[7] == total and out[8] == list(range(1, total + 1))
    assert ts_at_eval == list(range(0, total + 1, interval))
    assert np.array(eval_rewards).shape == (total // interval + 1, episodes) and np.all(np.array(eval_steps) == 1)
    # each evaluation (eval_episodes greedy starts) happens after exactly `interval` more updates
    assert agent.evals_at == [i * interval for i in range(total // interval + 1) for _ in range(episodes)]


def test_rule_4_truncation_in_the_cpu_restatement():
    """Bimodal2DEnv: `done` exactly at the step limit is truncated (not stored), before it is stored with gamma 0, the
    limit without `done` is stored with gamma and one more action is drawn -- on a scripted agent, so that the device
    loop's bookkeeping (rlc_env_advance_store) has a CPU statement of each rule that does not depend on a policy"""
    from helpers.bimodal_rollout import _BimodalLoop

    class Scripted(_BimodalLoop):
        def __init__(self, limit, total, step_size):
            self.limit, self.total_limit, self.eval_interval, self.eval_episodes = limit, total, 10 ** 9, 0
            self.total = self.evals = 0
            self.train_ret, self.train_len, self.train_cum = [], [], []
            self.eval_ret, self.eval_len, self.timesteps_at_eval = [], [], []
            self.stored, self.draws, self.step_size = [], 0, np.float32(step_size)

        def agent_reset(self):
            pass

        def act(self, obs, is_train):
            self.draws += 1
            return np.array([self.step_size, self.step_size], np.float32)

        def update(self, obs, obs_n, r, action, done, truncated):
            if not truncated:
                self.stored.append(0.0 if done else 0.99)

    # unit steps reach (4, 4) at step 4
    at = Scripted(limit=4, total=8, step_size=1.0).use_env("Bimodal2DEnv").run()
    assert at.rule_counts == {1: 0, 2: 0, 3: 0, 4: 2} and at.stored == [0.99] * 6 and at.train_len == [4, 4]
    assert at.draws == 2 * 4                                   # start + 3 steps; none after `done`
    before = Scripted(limit=6, total=8, step_size=1.0).use_env("Bimodal2DEnv").run()
    assert before.rule_counts == {1: 0, 2: 2, 3: 0, 4: 0} and before.stored == [0.99, 0.99, 0.99, 0.0] * 2
    never = Scripted(limit=3, total=6, step_size=1.0).use_env("Bimodal2DEnv").run()
    assert never.rule_counts == {1: 0, 2: 0, 3: 2, 4: 0} and never.stored == [0.99] * 6 and never.train_len == [3, 3]
    assert never.draws == 2 * 4                                # start + 3 steps: the last one is discarded
