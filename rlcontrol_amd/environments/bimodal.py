"""The reference's toy environments that need no gym (environments/environments.py:158-912 of the reference).

``Bimodal1DEnv`` and its six variants are one-step bandits: the state starts at 0, the action is added to it,
the reward is a sum of two Gaussians of the ACTION and the episode is over.  The reference writes seven
near-identical classes; here it is one class and a table of (peak positions, standard deviations, heights).
``Bimodal2DEnv`` walks on [-6, 6]^2 towards one of two goals under a two-Gaussian mixture reward.

The arithmetic is float64 with the reference's scalar functions and expression order (``math.exp`` in 1-D,
``np.exp`` / ``np.square`` in 2-D), so tests/test_bimodal_host.py asks for bit equality with what the reference
itself recorded (tests/golden/bimodal_envs.json).  The reference's constructor print and its plotting are left out.
The same arithmetic runs on the device (csrc/rollout_env.h).
"""
import math

import numpy as np

# name -> (maxima1, maxima2, stddev1, stddev2, height1, height2); environments.py:227-238 and the six copies of it
BIMODAL_1D = {
    'Bimodal1DEnv':           (-1.0, 1.0, 0.2, 0.2, 1., 1.5),
    'Bimodal1DEnv_uneq_var1': (-1.0, 1.0, 0.4, 0.2, 1., 1.5),
    'Bimodal1DEnv_uneq_var2': (-1.0, 1.0, 0.3, 0.1, 1., 1.5),
    'Bimodal1DEnv_uneq_var3': (-1.0, 1.0, 0.3, 0.1, 1., 1.),
    'Bimodal1DEnv_eq_var1':   (-0.6, 0.6, 0.2, 0.2, 1., 1.),
    'Bimodal1DEnv_eq_var2':   (-0.8, 0.8, 0.2, 0.2, 1., 1.),
    'Bimodal1DEnv_eq_var3':   (-1., 1., 0.2, 0.2, 1., 1.),
}
BIMODAL_2D = 'Bimodal2DEnv'
NAMES = tuple(BIMODAL_1D) + (BIMODAL_2D,)


def _scalar(x):
    """the one element of a size-1 array as a Python float (what math.exp makes of it in the reference)"""
    return float(np.asarray(x).reshape(-1)[0])


def create(env_params):
    name = env_params['environment']
    if name in BIMODAL_1D:
        return Bimodal1DEnvironment(env_params)
    if name == BIMODAL_2D:
        return Bimodal2DEnvironment(env_params)
    raise KeyError(name)


class _ToyEnvironment(object):
    """what Experiment and main.py read of an environment (the attribute set of ContinuousEnvironment)"""

    def __init__(self, env_params, low_state, high_state, low_action, high_action):
        self.name = env_params['environment']
        self.eval_interval = env_params['EvalIntervalMilSteps'] * 1000000
        self.eval_episodes = env_params['EvalEpisodes']
        self.TOTAL_STEPS_LIMIT = env_params['TotalMilSteps'] * 1000000
        # -1 means "the environment's own": 1 in the reference, for both families
        self.EPISODE_STEPS_LIMIT = env_params['EpisodeSteps'] if env_params['EpisodeSteps'] != -1 else 1
        self.state_min, self.state_max = np.array(low_state), np.array(high_state)
        self.state_range = self.state_max - self.state_min
        self.state_dim = len(low_state)
        self.state_bounded = True
        self.action_min, self.action_max = np.array(low_action), np.array(high_action)
        self.action_range = self.action_max - self.action_min
        self.action_dim = len(low_action)
        self.state = None

    def set_random_seed(self, random_seed):
        pass                                # nothing is drawn

    def close(self):
        pass


class Bimodal1DEnvironment(_ToyEnvironment):
    def __init__(self, env_params):
        _ToyEnvironment.__init__(self, env_params, [-2.], [2.], [-2.], [2.])
        self.constants = BIMODAL_1D[self.name]

    def reset(self):
        self.state = np.array([0.])
        return self.state

    def step(self, action):
        self.state = self.state + action    # terminal, and not clipped
        return self.state, self.reward_func(action), True, {}

    def reward_func(self, action):
        maxima1, maxima2, stddev1, stddev2, height1, height2 = self.constants
        modal1 = height1 * math.exp(_scalar(-0.5 * ((action - maxima1) / stddev1) ** 2))
        modal2 = height2 * math.exp(_scalar(-0.5 * ((action - maxima2) / stddev2) ** 2))
        return modal1 + modal2


class Bimodal2DEnvironment(_ToyEnvironment):
    def __init__(self, env_params):
        _ToyEnvironment.__init__(self, env_params, [-6.0, -6.0], [6.0, 6.0], [-1.0, -1.0], [1.0, 1.0])
        self.goal_states = np.array([[-4.0, -4.0], [4.0, 4.0]])

    def seed(self, seed):
        pass

    def reset(self):
        self.state = np.array([0.0, 0.0])
        return self.state

    def step(self, action):
        self.state = np.clip(self.state + action, self.state_min, self.state_max)
        return self.state, self.reward_func(self.state), self.reached_goal(self.state), {}

    def reward_func(self, state):
        magnitude, stddev = 125, 2.25
        coeff1 = 0.5
        coeff2 = 1 - coeff1
        (ax, ay), (bx, by) = self.goal_states
        norm = 2 * np.pi * np.square(stddev)
        modal1 = coeff1 * 1.0 / norm * np.exp(-0.5 * (np.square((state[0] - ax) / stddev) + np.square((state[1] - ay) / stddev)))
        modal2 = coeff2 * 1.0 / norm * np.exp(-0.5 * (np.square((state[0] - bx) / stddev) + np.square((state[1] - by) / stddev)))
        return magnitude * (modal1 + modal2) - 2

    def reached_goal(self, state):
        for goal in self.goal_states:
            if np.sum(np.square(np.abs(goal - state))) <= 0.5:
                return True
        return False
