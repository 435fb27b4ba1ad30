"""Python face of an OptimalQ population handle (rlc_optq_* in include/rlcontrol_hip.h): the Q-learner without an actor
whose greedy action and TD target come from an exhaustive search over a discretised action grid (agents/OptimalQ.py,
agents/network/optimal_q_network.py of the reference)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import RlcError, check, dptr, f64, fptr
from .hip_pop import Population, broadcast as bc, layout_of

# what rlc_optq_config.norm_type carries: the library runs 0 and refuses the others by name
NORM_CODES = {"none": 0, "input_norm": 0, "layer": 1, "batch": 2}
MAX_NODES = 1 << 24


def param_layout(S, A, L1, L2):
    """name -> (offset, shape), variable creation order of optimal_q_network.py:82-108; the action rows are the last A
    rows of W2 (tf.concat([net, action], 1), :94)"""
    return layout_of([("W1", (S, L1)), ("b1", (L1,)), ("W2", (L1 + A, L2)), ("b2", (L2,)), ("W3", (L2, 1)), ("b3", (1,))])


def init_params(S, A, L1, L2, seed):
    """The reference's initialiser families (optimal_q_network.py:84-106), drawn as hip_ddpg.init_params draws the
    critic's: hidden W and b ~ U(+-sqrt(3/fan_in)) (for a 1-D bias [n] TF takes fan_in = n), output W, b ~ U(+-3e-3).
    numpy RandomState(seed) stands in for TF's stream (distribution parity only)."""
    rng = np.random.RandomState(seed)
    lay, P = param_layout(S, A, L1, L2)
    theta = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        lim = 3e-3 if name in ("W3", "b3") else np.sqrt(3.0 / shp[0])
        theta[off:off + n] = rng.uniform(-lim, lim, n).astype(np.float32)
    return theta


def action_grid(action_min, action_max, discretization, action_dim):
    """discretized_action_pairs of the reference (optimal_q_network.py:163-179), float64 [n_nodes][action_dim]:
    np.arange over the FIRST dimension's bounds (plus 1e-10), the same axis for every action dimension, np.meshgrid in
    its default 'xy' order, flattened and zipped."""
    lo = float(np.asarray(action_min, np.float64).reshape(-1)[0])
    hi = float(np.asarray(action_max, np.float64).reshape(-1)[0])
    axis = np.arange(lo, hi + 1e-10, discretization)
    mesh = np.meshgrid(*np.tile(axis, (int(action_dim), 1)))
    return np.stack([m.flatten() for m in mesh], axis=1).astype(np.float64)


class OptQPopulation(Population):
    """One kernel: the any-shape one.  set_kernel("auto") and set_kernel("generic") mean the same, set_kernel("mfma")
    and set_split(n > 1) raise RlcError."""
    PREFIX = "rlc_optq"
    BETA_POWERS = 2
    BLOB = {"theta": 0, "theta_target": 1, "adam_m": 2, "adam_v": 3}
    TAP = {"q": 0, "y": 1, "max_q": 2, "a_star": 3, "grads": 4}

    def __init__(self, n_agents, state_dim, action_dim, l1_dim, l2_dim, batch_size, buffer_size, tau, state_min,
                 state_max, learning_rate, seeds, node_actions, clip_state=True, device=0, norm_type="input_norm"):
        self._init_base(n_agents, state_dim, action_dim, batch_size)
        if norm_type not in NORM_CODES:
            raise ValueError("norm_type %r: expected one of %s" % (norm_type, ", ".join(sorted(NORM_CODES))))
        self.dims = (self.S, self.A, int(l1_dim), int(l2_dim))
        self.norm_type = norm_type
        self.layout, self.P = param_layout(*self.dims)
        grid = np.ascontiguousarray(node_actions, np.float32).reshape(-1, max(self.A, 1))   # the upload is fp32
        self.n_nodes = int(grid.shape[0])
        self._keep = dict(smin=bc(state_min, self.S), smax=bc(state_max, self.S), lr=bc(learning_rate, self.n_agents),
                          grid=grid)
        self._keep["seed"], seed_ptr = self._seeds(seeds)
        cfg = _lib.rlc_optq_config()
        cfg.device, cfg.n_agents, cfg.state_dim, cfg.action_dim = int(device), self.n_agents, self.S, self.A
        cfg.l1_dim, cfg.l2_dim = self.dims[2:]
        cfg.batch_size, cfg.clip_state, cfg.buffer_size, cfg.tau = self.B, 1 if clip_state else 0, int(buffer_size), float(tau)
        cfg.norm_type = NORM_CODES[norm_type]
        cfg.state_min, cfg.state_max = fptr(self._keep["smin"]), fptr(self._keep["smax"])
        cfg.learning_rate = fptr(self._keep["lr"])
        cfg.seed = seed_ptr
        cfg.n_nodes = self.n_nodes
        cfg.node_actions = fptr(grid)
        check(self._lib.rlc_optq_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    def act(self, states, first_agent=0, with_q=False):
        """greedy grid row [n][A] of the online network for one state per agent (and its Q [n])"""
        s = f64(states).reshape(-1, self.S)
        a = np.empty((s.shape[0], self.A), np.float32)
        q = np.empty(s.shape[0], np.float32) if with_q else None
        check(self._lib.rlc_optq_act(self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s), fptr(a),
                                     fptr(q) if q is not None else None))
        return (a, q) if with_q else a

    def act_fetch(self, n, first_agent=0, with_q=False):
        a = np.empty((int(n), self.A), np.float32)
        q = np.empty(int(n), np.float32) if with_q else None
        check(self._lib.rlc_optq_act_fetch(self._h, int(first_agent), ctypes.c_int32(int(n)), fptr(a),
                                           fptr(q) if q is not None else None))
        return (a, q) if with_q else a

    def qval(self, agent, states, actions):
        s = f64(states).reshape(-1, self.S)
        a = f64(actions).reshape(s.shape[0], self.A)
        out = np.empty(s.shape[0], np.float32)
        check(self._lib.rlc_optq_qval(self._h, int(agent), ctypes.c_int32(s.shape[0]), dptr(s), dptr(a), fptr(out)))
        return out

    def set_split(self, n_workgroups):
        if int(n_workgroups) != 1:
            raise RlcError("OptimalQ has no latency mode: one workgroup per agent (the any-shape kernel only)")

    def tap_lengths(self):
        return {"q": self.B, "y": self.B, "max_q": self.B, "a_star": self.B * self.A, "grads": self.P}
