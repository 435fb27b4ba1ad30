"""Python face of an ActorCritic population handle (rlc_ac_* in include/rlcontrol_hip.h): the hydra network with a
one-mode Gaussian actor in pre-tanh space and a critic Q, trained by a TD step (critic) and by a likelihood-ratio or
cross-entropy step on sampled actions (actor) -- agents/ActorCritic.py, agents/network/ac_network.py of the reference."""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, fptr, iptr
from .hip_pop import Population, broadcast as bc, layout_of

# what rlc_ac_config.norm_type carries: the library runs 0 and refuses the others by name
NORM_CODES = {"none": 0, "input_norm": 0, "layer": 1, "batch": 2}
CRITIC_UPDATES = {"mean": 0, "sampled": 1, "expected": 2}           # 'random_q' is not implemented
ACTOR_UPDATES = {"ll": 0, "ll_update_all": 1, "cem": 2}             # 'reparam' is not implemented


def top_k(num_samples, rho):
    """int(num_samples * rho), formed in Python as the reference forms it (agents/ActorCritic.py:248)"""
    return int(num_samples * rho)


def next_draws(critic_update, num_samples):
    """draws per row for the next action of the TD target: 0 (mean), 1 (sampled), num_samples (expected)"""
    return {"mean": 0, "sampled": 1, "expected": int(num_samples)}[critic_update]


def param_layout(S, A, L1, La, Lc):
    """name -> (offset, shape), variable creation order of ac_network.py:124-288 with num_modal = 1; the action rows are
    last in Wq2 (:271).  The alpha head (Wal, bal) is carried and never trained."""
    return layout_of([("W1", (S, L1)), ("b1", (L1,)), ("Wp2", (L1, La)), ("bp2", (La,)), ("Wmu", (La, A)), ("bmu", (A,)),
                      ("Wls", (La, A)), ("bls", (A,)), ("Wal", (La, 1)), ("bal", (1,)),
                      ("Wq2", (L1 + A, Lc)), ("bq2", (Lc,)), ("Wq3", (Lc, 1)), ("bq3", (1,))])


def init_params(S, A, L1, La, Lc, seed):
    """The reference's initialiser families (ac_network.py:127-172, 271-287): variance_scaling(1.0, FAN_IN, uniform) =
    U(+-sqrt(3 / fan_in)) for the weights AND the biases of the shared layer, the actor layer, the mu head and the
    critic layer (a bias's fan_in is its length); the sigma head's weights U(0, 1), the alpha head's and Wq3 U(+-3e-3);
    the sigma, alpha and Wq3 biases U(+-3e-3).  numpy RandomState(seed) stands in for TF's stream (SURVEY.md a11:
    distribution parity only)."""
    rng = np.random.RandomState(seed)
    lay, P = param_layout(S, A, L1, La, Lc)
    theta = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        if name == "Wls":
            lo, hi = 0.0, 1.0
        elif name in ("bls", "Wal", "bal", "Wq3", "bq3"):
            lo, hi = -0.003, 0.003
        else:
            lim = np.sqrt(3.0 / shp[0])
            lo, hi = -lim, lim
        theta[off:off + n] = rng.uniform(lo, hi, n).astype(np.float32)
    return theta


class ACPopulation(Population):
    """One kernel: the any-shape one.  set_kernel("auto") and set_kernel("generic") mean the same, set_kernel("mfma")
    and set_split(n > 1) raise RlcError.  Draws: pass the standard normals (eps, and eps_next when critic_update draws)
    or none of them (the device's Philox stream)."""
    PREFIX = "rlc_ac"
    BETA_POWERS = 4
    BLOB = {"theta": 0, "theta_target": 1, "actor_m": 2, "actor_v": 3, "critic_m": 4, "critic_v": 5}
    TAP = {"q": 0, "y": 1, "a_next": 2, "raw_samples": 3, "samples": 4, "sample_q": 5, "weights": 6, "grads_a": 7,
           "grads_c": 8}

    def __init__(self, n_agents, state_dim, action_dim, shared_l1_dim, actor_l2_dim, critic_l2_dim, num_samples, top_k,
                 batch_size, buffer_size, tau, state_min, state_max, action_max, actor_lr, critic_lr, seeds,
                 critic_update="sampled", actor_update="ll", clip_state=True, device=0, norm_type="input_norm"):
        self._init_base(n_agents, state_dim, action_dim, batch_size)
        if norm_type not in NORM_CODES:
            raise ValueError("norm_type %r: expected one of %s" % (norm_type, ", ".join(sorted(NORM_CODES))))
        if critic_update not in CRITIC_UPDATES:
            raise ValueError("critic_update %r: expected one of %s" % (critic_update, ", ".join(sorted(CRITIC_UPDATES))))
        if actor_update not in ACTOR_UPDATES:
            raise ValueError("actor_update %r: expected one of %s" % (actor_update, ", ".join(sorted(ACTOR_UPDATES))))
        self.dims = (self.S, self.A, int(shared_l1_dim), int(actor_l2_dim), int(critic_l2_dim))
        self.n, self.k = int(num_samples), int(top_k)
        self.critic_update, self.actor_update = critic_update, actor_update
        self.n_next = next_draws(critic_update, self.n)
        self.norm_type = norm_type
        self.layout, self.P = param_layout(*self.dims)
        self._keep = dict(smin=bc(state_min, self.S), smax=bc(state_max, self.S), amax=bc(action_max, self.A),
                          alr=bc(actor_lr, self.n_agents), clr=bc(critic_lr, self.n_agents))
        self._keep["seed"], seed_ptr = self._seeds(seeds)
        cfg = _lib.rlc_ac_config()
        cfg.device, cfg.n_agents, cfg.state_dim, cfg.action_dim = int(device), self.n_agents, self.S, self.A
        cfg.shared_l1_dim, cfg.actor_l2_dim, cfg.critic_l2_dim = self.dims[2:5]
        cfg.num_samples, cfg.top_k = self.n, self.k
        cfg.critic_update, cfg.actor_update = CRITIC_UPDATES[critic_update], ACTOR_UPDATES[actor_update]
        cfg.batch_size, cfg.clip_state, cfg.buffer_size, cfg.tau = self.B, 1 if clip_state else 0, int(buffer_size), float(tau)
        cfg.norm_type = NORM_CODES[norm_type]
        cfg.state_min, cfg.state_max = fptr(self._keep["smin"]), fptr(self._keep["smax"])
        cfg.action_max = fptr(self._keep["amax"])
        cfg.actor_lr, cfg.critic_lr = fptr(self._keep["alr"]), fptr(self._keep["clr"])
        cfg.seed = seed_ptr
        check(self._lib.rlc_ac_create(ctypes.byref(cfg), ctypes.byref(self._h)))

    # ---- draws ------------------------------------------------------------------------------
    def _draws(self, eps_next, eps, rows):
        """(eps_next, eps) as contiguous float32 of rows * n_next * A and rows * n * A entries; eps_next None when
        critic_update is 'mean'; (None, None): the device's stream"""
        if eps is None:
            if eps_next is not None:
                raise ValueError("eps_next without eps: pass the draws of the whole update, or none")
            return None, None
        if (eps_next is not None) != (self.n_next > 0):
            raise ValueError("critic_update %r takes %d next draws per row: eps_next must be %s" % (
                self.critic_update, self.n_next, "given" if self.n_next else "None"))
        eps = np.ascontiguousarray(eps, np.float32)
        if eps.size != rows * self.n * self.A:
            raise ValueError("eps must hold %d entries (got %d)" % (rows * self.n * self.A, eps.size))
        if eps_next is not None:
            eps_next = np.ascontiguousarray(eps_next, np.float32)
            if eps_next.size != rows * self.n_next * self.A:
                raise ValueError("eps_next must hold %d entries (got %d)" % (rows * self.n_next * self.A, eps_next.size))
        return eps_next, eps

    # ---- acting -----------------------------------------------------------------------------
    def _act_args(self, states, first_agent, sample, eps):
        s = f64(states).reshape(-1, self.S)
        if eps is not None:
            eps = np.ascontiguousarray(eps, np.float32)
            if eps.size != s.shape[0] * self.A:
                raise ValueError("eps must hold %d entries (got %d)" % (s.shape[0] * self.A, eps.size))
        keep = (s, eps)
        return keep, (self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s), ctypes.c_int32(1 if sample else 0),
                      fptr(eps) if eps is not None else None)

    def act(self, states, first_agent=0, sample=False, eps=None):
        """sample False: tanh(mu) * action_max [n][A]; True: tanh(mu + sigma * eps) * action_max (eps [n][A] standard
        normal, or None: the device's stream)"""
        keep, args = self._act_args(states, first_agent, sample, eps)
        out = np.empty((keep[0].shape[0], self.A), np.float32)
        check(self._lib.rlc_ac_act(*(args + (fptr(out),))))
        return out

    def act_queue(self, states, first_agent=0, sample=False, eps=None):
        """queue the acting forward for `states` behind the work already on the handle's stream (no synchronisation)"""
        keep, args = self._act_args(states, first_agent, sample, eps)
        check(self._lib.rlc_ac_act_queue(*args))
        return keep[0].shape[0]

    def qval(self, agent, states, actions):
        s = f64(states).reshape(-1, self.S)
        a = f64(actions).reshape(s.shape[0], self.A)
        out = np.empty(s.shape[0], np.float32)
        check(self._lib.rlc_ac_qval(self._h, int(agent), ctypes.c_int32(s.shape[0]), dptr(s), dptr(a), fptr(out)))
        return out

    # ---- learning ---------------------------------------------------------------------------
    def update(self, n_updates=1, host_indices=None, eps_next=None, eps=None):
        """eps_next [n_agents][n_updates][B][n_next][A], eps [n_agents][n_updates][B][n][A] standard normal, or neither"""
        idx = None
        if host_indices is not None:
            idx = np.ascontiguousarray(host_indices, np.int64)
            if idx.size != self.n_agents * int(n_updates) * self.B:
                raise ValueError("host_indices must hold n_agents*n_updates*batch_size entries")
        eps_next, eps = self._draws(eps_next, eps, self.n_agents * int(n_updates) * self.B)
        check(self._lib.rlc_ac_update(self._h, ctypes.c_int32(int(n_updates)), iptr(idx) if idx is not None else None,
                                      fptr(eps_next) if eps_next is not None else None,
                                      fptr(eps) if eps is not None else None))

    def update_batch(self, agent, states, actions, next_states, rewards, gammas, eps_next=None, eps=None):
        r = f64(rewards).reshape(-1)
        n = r.size
        s, s2 = f64(states).reshape(n, self.S), f64(next_states).reshape(n, self.S)
        a, g = f64(actions).reshape(n, self.A), f64(gammas).reshape(n)
        eps_next, eps = self._draws(eps_next, eps, n)
        check(self._lib.rlc_ac_update_batch(self._h, int(agent), ctypes.c_int32(n), dptr(s), dptr(a), dptr(s2), dptr(r),
                                            dptr(g), fptr(eps_next) if eps_next is not None else None,
                                            fptr(eps) if eps is not None else None))

    def tap_lengths(self):
        B, SN = self.B, self.B * self.n
        return {"q": B, "y": B, "a_next": B * max(self.n_next, 1) * self.A, "raw_samples": SN * self.A,
                "samples": SN * self.A, "sample_q": SN, "weights": SN, "grads_a": self.P, "grads_c": self.P}
