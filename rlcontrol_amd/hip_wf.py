"""Python face of a WireFitting population handle (rlc_wf_* in include/rlcontrol_hip.h): the Q-learner whose one
network puts out app_points wires (an action and a value each) and whose Q(s, a) interpolates the wire values
(agents/WireFitting.py, agents/network/wf_network.py of the reference)."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, fptr
from .hip_pop import Population, broadcast as bc, layout_of

# what rlc_wf_config.norm_type carries: the library runs 0 and refuses the others by name
NORM_CODES = {"none": 0, "input_norm": 0, "layer": 1, "batch": 2}


def param_layout(S, A, L1, L2, N):
    """name -> (offset, shape), variable creation order of wf_network.py:76-92,116; wire i owns columns i*A .. i*A+A-1
    of Wa (the reshape to [-1, app_points, action_dim], :112)"""
    return layout_of([("W1", (S, L1)), ("b1", (L1,)), ("W2", (L1, L2)), ("b2", (L2,)), ("Wa", (L2, N * A)), ("ba", (N * A,)),
                      ("Wq", (L2, N)), ("bq", (N,)), ("kappa", (N,))])


def init_params(S, A, L1, L2, N, seed):
    """The reference's initialiser families: slim.fully_connected's defaults for the hidden layers (Xavier-uniform
    weights, U(+-sqrt(6 / (fan_in + fan_out))), zero biases; wf_network.py:76,78), U(-1, 1) weights and zero biases for
    both heads (:86-92), U(-0.003, 0.003) for smooth_c (:115-116).  numpy RandomState(seed) stands in for TF's stream
    (distribution parity only)."""
    rng = np.random.RandomState(seed)
    lay, P = param_layout(S, A, L1, L2, N)
    theta = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        if name in ("W1", "W2"):
            lim = np.sqrt(6.0 / (shp[0] + shp[1]))
        elif name in ("Wa", "Wq"):
            lim = 1.0
        elif name == "kappa":
            lim = 0.003
        else:
            continue                                   # biases: zero
        theta[off:off + n] = rng.uniform(-lim, lim, n).astype(np.float32)
    return theta


class WFPopulation(Population):
    """One kernel: the any-shape one.  set_kernel("auto") and set_kernel("generic") mean the same, set_kernel("mfma")
    and set_split(n > 1) raise RlcError."""
    PREFIX = "rlc_wf"
    BETA_POWERS = 2
    BLOB = {"theta": 0, "theta_target": 1, "adam_m": 2, "adam_v": 3}
    TAP = {"q": 0, "y": 1, "max_q": 2, "grads": 3}

    def __init__(self, n_agents, state_dim, action_dim, l1_dim, l2_dim, app_points, batch_size, buffer_size, tau,
                 state_min, state_max, action_max0, learning_rate, seeds, clip_state=True, device=0,
                 norm_type="input_norm"):
        self._init_base(n_agents, state_dim, action_dim, batch_size)
        if norm_type not in NORM_CODES:
            raise ValueError("norm_type %r: expected one of %s" % (norm_type, ", ".join(sorted(NORM_CODES))))
        self.dims = (self.S, self.A, int(l1_dim), int(l2_dim), int(app_points))
        self.N = self.dims[4]
        self.norm_type = norm_type
        self.layout, self.P = param_layout(*self.dims)
        self._keep = dict(smin=bc(state_min, self.S), smax=bc(state_max, self.S), lr=bc(learning_rate, self.n_agents))
        self._keep["seed"], seed_ptr = self._seeds(seeds)
        cfg = _lib.rlc_wf_config()
        cfg.device, cfg.n_agents, cfg.state_dim, cfg.action_dim = int(device), self.n_agents, self.S, self.A
        cfg.l1_dim, cfg.l2_dim = self.dims[2:4]
        cfg.batch_size, cfg.clip_state, cfg.buffer_size, cfg.tau = self.B, 1 if clip_state else 0, int(buffer_size), float(tau)
        cfg.norm_type = NORM_CODES[norm_type]
        cfg.state_min, cfg.state_max = fptr(self._keep["smin"]), fptr(self._keep["smax"])
        cfg.learning_rate = fptr(self._keep["lr"])
        cfg.seed = seed_ptr
        cfg.app_points = self.N
        cfg.action_max0 = float(action_max0)
        check(self._lib.rlc_wf_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    def _wires(self, n):
        return np.empty(int(n) * self.N * (self.A + 1), np.float32)

    def _split_wires(self, n, w):
        n = int(n)
        return w[:n * self.N * self.A].reshape(n, self.N, self.A), w[n * self.N * self.A:].reshape(n, self.N)

    def act(self, states, first_agent=0, with_wires=False):
        """the arg-max wire's action [n][A] of the online network for one state per agent (and every wire's action
        [n][N][A] and value [n][N])"""
        s = f64(states).reshape(-1, self.S)
        a = np.empty((s.shape[0], self.A), np.float32)
        w = self._wires(s.shape[0]) if with_wires else None
        check(self._lib.rlc_wf_act(self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s), fptr(a),
                                   fptr(w) if w is not None else None))
        return (a,) + self._split_wires(s.shape[0], w) if with_wires else a

    def act_fetch(self, n, first_agent=0, with_wires=False):
        a = np.empty((int(n), self.A), np.float32)
        w = self._wires(n) if with_wires else None
        check(self._lib.rlc_wf_act_fetch(self._h, int(first_agent), ctypes.c_int32(int(n)), fptr(a),
                                         fptr(w) if w is not None else None))
        return (a,) + self._split_wires(n, w) if with_wires else a

    def qval(self, agent, states, actions):
        s = f64(states).reshape(-1, self.S)
        a = f64(actions).reshape(s.shape[0], self.A)
        out = np.empty(s.shape[0], np.float32)
        check(self._lib.rlc_wf_qval(self._h, int(agent), ctypes.c_int32(s.shape[0]), dptr(s), dptr(a), fptr(out)))
        return out

    def tap_lengths(self):
        return {"q": self.B, "y": self.B, "max_q": self.B, "grads": self.P}
