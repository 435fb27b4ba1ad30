"""TEST INFRASTRUCTURE -- CPU restatement of the on-device experiment loop on the Bimodal toy environments.

oracle/rollout.py restates the loop for Pendulum-v0 only (``done = step >= limit`` is written into its ``run`` and
``eval``).  The classes here keep its agents -- ``act``, ``update``, ``_learn`` and the Philox streams are inherited
unchanged -- and replace the environments and the two loops, so that the environment's own ``done`` drives the
episode.  The episode rules are those of the reference's experiment.py:102-160,196-215:

  1. Bimodal1DEnv family: ``is_truncated`` is always False; the single transition is stored with gamma 0 although
     ``done`` coincides with the step limit of 1 (experiment.py:122-125).
  2. ``done`` before the limit: stored with gamma 0, the episode ends.
  3. the limit without ``done``: stored with gamma, the episode ends -- and ``agent.step(obs_n)`` is still called
     once (``if not done``), its action discarded: the draw consumes the agent's exploration stream.
  4. ``done`` exactly at the limit (outside the 1-D family): truncated, not stored.

``rule_counts`` records how often each occurred in the training loop, so a test can assert that a run met them.

The environments are written a second time here (plain Python floats, no numpy arrays) and compared with
rlcontrol_amd/environments/bimodal.py on the reference's recorded fixture by tests/test_bimodal_host.py.
"""
import math

import numpy as np

from oracle.rollout import KlRolloutOracle, NafRolloutOracle, RolloutOracle, SacRolloutOracle

# name -> (maxima1, maxima2, stddev1, stddev2, height1, height2); the index is the device's variant number
VARIANTS_1D = [
    ("Bimodal1DEnv", (-1.0, 1.0, 0.2, 0.2, 1.0, 1.5)),
    ("Bimodal1DEnv_uneq_var1", (-1.0, 1.0, 0.4, 0.2, 1.0, 1.5)),
    ("Bimodal1DEnv_uneq_var2", (-1.0, 1.0, 0.3, 0.1, 1.0, 1.5)),
    ("Bimodal1DEnv_uneq_var3", (-1.0, 1.0, 0.3, 0.1, 1.0, 1.0)),
    ("Bimodal1DEnv_eq_var1", (-0.6, 0.6, 0.2, 0.2, 1.0, 1.0)),
    ("Bimodal1DEnv_eq_var2", (-0.8, 0.8, 0.2, 0.2, 1.0, 1.0)),
    ("Bimodal1DEnv_eq_var3", (-1.0, 1.0, 0.2, 0.2, 1.0, 1.0)),
]


def reward_1d(name, a):
    m1, m2, s1, s2, h1, h2 = dict(VARIANTS_1D)[name]
    z1, z2 = (a - m1) / s1, (a - m2) / s2
    return h1 * math.exp(-0.5 * (z1 * z1)) + h2 * math.exp(-0.5 * (z2 * z2))


class Bimodal1D(object):
    """step() -> (observation, reward, done); the action is a float32 vector, widened as the device widens it"""

    def __init__(self, name):
        self.name = name
        self.resets = 0
        self.state = 0.0

    def reset_at(self, ctr):
        self.state = 0.0
        return np.array([self.state])

    def reset(self):
        self.resets += 1
        return self.reset_at(self.resets - 1)

    def step(self, action):
        a = float(np.asarray(action).reshape(-1)[0])
        self.state = self.state + a
        return np.array([self.state]), reward_1d(self.name, a), True


class Bimodal2D(object):
    name = "Bimodal2DEnv"

    def __init__(self, name="Bimodal2DEnv"):
        self.resets = 0
        self.x = self.y = 0.0

    def reset_at(self, ctr):
        self.x = self.y = 0.0
        return np.array([self.x, self.y])

    def reset(self):
        self.resets += 1
        return self.reset_at(self.resets - 1)

    def step(self, action):
        a = np.asarray(action).reshape(-1)
        x = min(max(self.x + float(a[0]), -6.0), 6.0)
        y = min(max(self.y + float(a[1]), -6.0), 6.0)
        self.x, self.y = x, y
        stddev = 2.25
        norm = 2 * math.pi * (stddev * stddev)
        # np.exp is the reference's function here (math.exp in 1-D)
        m1 = 0.5 * 1.0 / norm * float(np.exp(-0.5 * (((x - -4.0) / stddev) ** 2 + ((y - -4.0) / stddev) ** 2)))
        m2 = 0.5 * 1.0 / norm * float(np.exp(-0.5 * (((x - 4.0) / stddev) ** 2 + ((y - 4.0) / stddev) ** 2)))
        reward = 125 * (m1 + m2) - 2
        done = ((-4.0 - x) ** 2 + (-4.0 - y) ** 2 <= 0.5) or ((4.0 - x) ** 2 + (4.0 - y) ** 2 <= 0.5)
        return np.array([x, y]), reward, bool(done)


def make_env(name):
    return Bimodal2D() if name == "Bimodal2DEnv" else Bimodal1D(name)


class _BimodalLoop(object):
    """run / eval of oracle/rollout.py with the environment's own `done` (the four rules of the module docstring)"""

    def use_env(self, name):
        self.env_name = name
        self.train_env, self.test_env = make_env(name), make_env(name)
        self.exempt = name.startswith("Bimodal1DEnv")
        self.rule_counts = {1: 0, 2: 0, 3: 0, 4: 0}
        return self

    def eval(self):
        rets, lens = [], []
        for e in range(self.eval_episodes):
            obs = self.test_env.reset_at(self.evals * self.eval_episodes + e)
            self.agent_reset()
            ret, steps, done = 0.0, 0, False
            action = self.act(obs, False)
            while not (done or steps == self.limit):
                obs, r, done = self.test_env.step(action)
                ret += r
                if not done:
                    action = self.act(obs, False)
                steps += 1
            rets.append(ret)
            lens.append(steps)
        self.eval_ret.append(rets)
        self.eval_len.append(lens)
        self.evals += 1

    def run(self, max_steps=None):
        stop = self.total_limit if max_steps is None else min(self.total_limit, max_steps)
        self.eval()
        self.timesteps_at_eval.append(self.total)
        self.n_started = 0
        while self.total < stop:
            self.n_started += 1
            obs = self.train_env.reset()
            self.agent_reset()
            ret, done, step = 0.0, False, 0
            action = self.act(obs, True)
            while not (done or step == self.limit or self.total == stop):
                step += 1
                self.total += 1
                obs_n, r, done = self.train_env.step(action)
                ret += r
                at_limit = step == self.limit
                truncated = (not self.exempt) and bool(done and at_limit)
                rule = 1 if self.exempt else 4 if truncated else 2 if done else 3 if at_limit else 0
                if rule:
                    self.rule_counts[rule] += 1
                self.update(obs, obs_n, r, action, done, truncated)
                if not done:
                    action = self.act(obs_n, True)         # rule 3: drawn and discarded
                obs = obs_n
                if self.total % self.eval_interval == 0:
                    self.timesteps_at_eval.append(self.total)
                    self.eval()
            if done or step == self.limit:
                self.train_ret.append(ret)
                self.train_len.append(step)
                self.train_cum.append(self.total)
        self.last_obs, self.last_step = obs, step
        return self


class BimodalRolloutOracle(_BimodalLoop, RolloutOracle):
    pass


class BimodalSacRolloutOracle(_BimodalLoop, SacRolloutOracle):
    pass


class BimodalKlRolloutOracle(_BimodalLoop, KlRolloutOracle):
    pass


class BimodalNafRolloutOracle(_BimodalLoop, NafRolloutOracle):
    pass
