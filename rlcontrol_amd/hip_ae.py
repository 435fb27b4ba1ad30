"""Python face of an ActorExpert population handle (rlc_ae_* in include/rlcontrol_hip.h): the hydra network with a
mixture-density actor and an expert Q, trained by Q-learning (expert) and by the likelihood of the top-k sampled actions
(actor) -- agents/ActorExpert.py, agents/network/ae_network.py of the reference."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, fptr, iptr
from .hip_pop import Population, broadcast as bc, layout_of

# what rlc_ae_config.norm_type carries: the library runs 0 and refuses the others by name
NORM_CODES = {"none": 0, "input_norm": 0, "layer": 1, "batch": 2}


def top_k(num_samples, rho):
    """int(num_samples * rho), formed in Python as the reference forms it (agents/ActorExpert.py:177)"""
    return int(num_samples * rho)


def param_layout(S, A, L1, La, Le, M):
    """name -> (offset, shape), variable creation order of ae_network.py:138-229; mode m, dimension d is column m*A + d of
    Wm and Ws (the reshape to [-1, num_modal, action_dim], :189-190); the action rows are last in Wq2 (:214)"""
    return layout_of([("W1", (S, L1)), ("b1", (L1,)), ("Wa2", (L1, La)), ("ba2", (La,)), ("Wm", (La, M * A)), ("bm", (M * A,)),
                      ("Ws", (La, M * A)), ("bs", (M * A,)), ("Wal", (La, M)), ("bal", (M,)),
                      ("Wq2", (L1 + A, Le)), ("bq2", (Le,)), ("Wq3", (Le, 1)), ("bq3", (1,))])


def init_params(S, A, L1, La, Le, M, seed):
    """The reference's initialiser families (ae_network.py:140-227): variance_scaling(1.0, FAN_IN, uniform) =
    U(+-sqrt(3 / fan_in)) for the weights AND the biases of the shared layer, the actor layer, the mean head and the
    expert layer (a bias's fan_in is its length); the sigma head's weights U(0, 1), the alpha head's and Wq3 U(+-3e-3);
    the sigma, alpha and Wq3 biases U(+-3e-3).  numpy RandomState(seed) stands in for TF's stream (SURVEY.md a11:
    distribution parity only)."""
    rng = np.random.RandomState(seed)
    lay, P = param_layout(S, A, L1, La, Le, M)
    theta = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        if name == "Ws":
            lo, hi = 0.0, 1.0
        elif name in ("bs", "Wal", "bal", "Wq3", "bq3"):
            lo, hi = -0.003, 0.003
        else:
            lim = np.sqrt(3.0 / shp[0])
            lo, hi = -lim, lim
        theta[off:off + n] = rng.uniform(lo, hi, n).astype(np.float32)
    return theta


class AEPopulation(Population):
    """One kernel: the any-shape one.  set_kernel("auto") and set_kernel("generic") mean the same, set_kernel("mfma")
    and set_split(n > 1) raise RlcError.  Draws: pass (u, eps) or neither (the device's Philox stream)."""
    PREFIX = "rlc_ae"
    BETA_POWERS = 4
    BLOB = {"theta": 0, "theta_target": 1, "actor_m": 2, "actor_v": 3, "expert_m": 4, "expert_v": 5}
    TAP = {"q": 0, "y": 1, "a_next": 2, "samples": 3, "sample_q": 4, "selected": 5, "actor_loss": 6, "grads_a": 7,
           "grads_e": 8}

    def __init__(self, n_agents, state_dim, action_dim, shared_l1_dim, actor_l2_dim, expert_l2_dim, num_modal, num_samples,
                 top_k, batch_size, buffer_size, tau, state_min, state_max, action_min, action_max, actor_lr, expert_lr,
                 seeds, clip_state=True, device=0, norm_type="input_norm"):
        self._init_base(n_agents, state_dim, action_dim, batch_size)
        if norm_type not in NORM_CODES:
            raise ValueError("norm_type %r: expected one of %s" % (norm_type, ", ".join(sorted(NORM_CODES))))
        self.dims = (self.S, self.A, int(shared_l1_dim), int(actor_l2_dim), int(expert_l2_dim), int(num_modal))
        self.M, self.n, self.k = int(num_modal), int(num_samples), int(top_k)
        self.norm_type = norm_type
        self.layout, self.P = param_layout(*self.dims)
        self._keep = dict(smin=bc(state_min, self.S), smax=bc(state_max, self.S), amin=bc(action_min, self.A),
                          amax=bc(action_max, self.A), alr=bc(actor_lr, self.n_agents), elr=bc(expert_lr, self.n_agents))
        self._keep["seed"], seed_ptr = self._seeds(seeds)
        cfg = _lib.rlc_ae_config()
        cfg.device, cfg.n_agents, cfg.state_dim, cfg.action_dim = int(device), self.n_agents, self.S, self.A
        cfg.shared_l1_dim, cfg.actor_l2_dim, cfg.expert_l2_dim = self.dims[2:5]
        cfg.num_modal, cfg.num_samples, cfg.top_k = self.M, self.n, self.k
        cfg.batch_size, cfg.clip_state, cfg.buffer_size, cfg.tau = self.B, 1 if clip_state else 0, int(buffer_size), float(tau)
        cfg.norm_type = NORM_CODES[norm_type]
        cfg.state_min, cfg.state_max = fptr(self._keep["smin"]), fptr(self._keep["smax"])
        cfg.action_min, cfg.action_max = fptr(self._keep["amin"]), fptr(self._keep["amax"])
        cfg.actor_lr, cfg.expert_lr = fptr(self._keep["alr"]), fptr(self._keep["elr"])
        cfg.seed = seed_ptr
        check(self._lib.rlc_ae_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    # ---- draws ------------------------------------------------------------------------------
    @staticmethod
    def _draws(u, eps, rows, A):
        """(u, eps) as contiguous float32 of rows and rows * A entries, or (None, None)"""
        if (u is None) != (eps is None):
            raise ValueError("u and eps: pass both, or neither for the device's Philox stream")
        if u is None:
            return None, None
        u, eps = np.ascontiguousarray(u, np.float32), np.ascontiguousarray(eps, np.float32)
        if u.size != rows or eps.size != rows * A:
            raise ValueError("u must hold %d entries and eps %d (got %d and %d)" % (rows, rows * A, u.size, eps.size))
        return u, eps

    # ---- acting -----------------------------------------------------------------------------
    def _act_args(self, states, first_agent, sample, u, eps):
        s = f64(states).reshape(-1, self.S)
        u, eps = self._draws(u, eps, s.shape[0], self.A)
        keep = (s, u, eps)
        return keep, (self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s), ctypes.c_int32(1 if sample else 0),
                      fptr(u) if u is not None else None, fptr(eps) if eps is not None else None)

    def act(self, states, first_agent=0, sample=False, u=None, eps=None):
        """sample False: the mean of the largest-alpha mode [n][A]; True: one draw, clipped to the action bounds"""
        keep, args = self._act_args(states, first_agent, sample, u, eps)
        out = np.empty((keep[0].shape[0], self.A), np.float32)
        check(self._lib.rlc_ae_act(*(args + (fptr(out),))))
        return out

    def act_queue(self, states, first_agent=0, sample=False, u=None, eps=None):
        """queue the acting forward for `states` behind the work already on the handle's stream (no synchronisation)"""
        keep, args = self._act_args(states, first_agent, sample, u, eps)
        check(self._lib.rlc_ae_act_queue(*args))
        return keep[0].shape[0]

    def qval(self, agent, states, actions):
        s = f64(states).reshape(-1, self.S)
        a = f64(actions).reshape(s.shape[0], self.A)
        out = np.empty(s.shape[0], np.float32)
        check(self._lib.rlc_ae_qval(self._h, int(agent), ctypes.c_int32(s.shape[0]), dptr(s), dptr(a), fptr(out)))
        return out

    # ---- learning ---------------------------------------------------------------------------
    def update(self, n_updates=1, host_indices=None, u=None, eps=None):
        """u [n_agents][n_updates][B][n] uniform in [0, 1), eps [..][n][A] standard normal, or neither"""
        idx = None
        if host_indices is not None:
            idx = np.ascontiguousarray(host_indices, np.int64)
            if idx.size != self.n_agents * int(n_updates) * self.B:
                raise ValueError("host_indices must hold n_agents*n_updates*batch_size entries")
        u, eps = self._draws(u, eps, self.n_agents * int(n_updates) * self.B * self.n, self.A)
        check(self._lib.rlc_ae_update(self._h, ctypes.c_int32(int(n_updates)), iptr(idx) if idx is not None else None,
                                      fptr(u) if u is not None else None, fptr(eps) if eps is not None else None))

    def update_batch(self, agent, states, actions, next_states, rewards, gammas, u=None, eps=None):
        r = f64(rewards).reshape(-1)
        n = r.size
        s, s2 = f64(states).reshape(n, self.S), f64(next_states).reshape(n, self.S)
        a, g = f64(actions).reshape(n, self.A), f64(gammas).reshape(n)
        u, eps = self._draws(u, eps, n * self.n, self.A)
        check(self._lib.rlc_ae_update_batch(self._h, int(agent), ctypes.c_int32(n), dptr(s), dptr(a), dptr(s2), dptr(r),
                                            dptr(g), fptr(u) if u is not None else None,
                                            fptr(eps) if eps is not None else None))

    def tap_lengths(self):
        B = self.B
        return {"q": B, "y": B, "a_next": B * self.A, "samples": B * self.n * self.A, "sample_q": B * self.n,
                "selected": B * self.k, "actor_loss": 1, "grads_a": self.P, "grads_e": self.P}
