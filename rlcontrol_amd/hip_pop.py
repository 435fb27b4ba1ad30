"""Common part of every population handle (rlc_handle): lifetime, replay ring, timing, and the plumbing every algorithm
has under its own symbol prefix (blobs, taps, update, queued acting, kernel choice).

One handle = a population of independent agents of ONE algorithm on one MI355X (include/rlcontrol_hip.h).
The per-algorithm classes (hip_ddpg.DDPGPopulation, hip_sac.SACPopulation, hip_naf.NAFPopulation, hip_kl.KLPopulation,
hip_optq.OptQPopulation, hip_wf.WFPopulation, hip_ae.AEPopulation, hip_ac.ACPopulation) add the constructor, the tables (PREFIX, BLOB, TAP, BETA_POWERS, tap_lengths) and what only they have."""
import ctypes
from collections import OrderedDict

import numpy as np

from . import _lib
from ._lib import check, dptr, f64, fptr, iptr

NORM_TYPES = {"none": 0, "input_norm": 0, "layer": 1}


def broadcast(v, n, dtype=np.float32):
    """per-agent / per-dimension constructor argument (a scalar or n values) -> contiguous [n] array"""
    return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype).reshape(-1), (n,)))


def layout_of(items):
    """[(name, shape)] in variable creation order -> (name -> (offset, shape), parameter count)"""
    out, p = OrderedDict(), 0
    for name, shp in items:
        out[name] = (p, shp)
        p += int(np.prod(shp))
    return out, p


def _opt(ptr, a):
    return ptr(a) if a is not None else None


class Population(object):
    PREFIX = None                        # "rlc_ddpg", "rlc_sac", "rlc_naf", "rlc_kl"
    KERNEL = {"auto": 0, "generic": 1, "mfma": 2}
    BETA_POWERS = 4
    EPS = False                          # update / update_batch take injected N(0,1) draws

    def _init_base(self, n_agents, state_dim, action_dim, batch_size):
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        self.n_agents = int(n_agents)
        self.S, self.A, self.B = int(state_dim), int(action_dim), int(batch_size)

    # ---- lifetime -------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self._lib.rlc_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        check(self._lib.rlc_sync(self._h))

    def _fn(self, name):
        return getattr(self._lib, self.PREFIX + name)

    def _seeds(self, seeds):
        s = broadcast(seeds, self.n_agents, np.uint64)
        return s, s.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))

    # ---- parameters -----------------------------------------------------------------------
    def set_blob(self, agent, which, values):
        v = np.ascontiguousarray(values, np.float32).reshape(-1)
        check(self._fn("_set_blob")(self._h, int(agent), self.BLOB[which], fptr(v), ctypes.c_int64(v.size)))

    def get_blob(self, agent, which):
        out = np.empty(self.P, np.float32)
        check(self._fn("_get_blob")(self._h, int(agent), self.BLOB[which], fptr(out), ctypes.c_int64(self.P)))
        return out

    def set_params(self, agent, theta, init_target=True):
        self.set_blob(agent, "theta", theta)
        if init_target:
            check(self._fn("_init_target")(self._h, int(agent)))

    def get_beta_powers(self, agent):
        out = np.empty(self.BETA_POWERS, np.float32)
        check(self._fn("_get_beta_powers")(self._h, int(agent), fptr(out)))
        return out

    def set_beta_powers(self, agent, pw4):
        v = np.ascontiguousarray(pw4, np.float32).reshape(self.BETA_POWERS)
        check(self._fn("_set_beta_powers")(self._h, int(agent), fptr(v)))

    def named(self, blob):
        return OrderedDict((k, blob[o:o + int(np.prod(s))].reshape(s)) for k, (o, s) in self.layout.items())

    # ---- acting ---------------------------------------------------------------------------
    def act_queue(self, states, first_agent=0):
        """queue the greedy forward for `states` behind the work already on the handle's stream (no synchronisation)"""
        s = f64(states).reshape(-1, self.S)
        check(self._fn("_act_queue")(self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s)))
        return s.shape[0]

    def act_fetch(self, n, first_agent=0):
        out = np.empty((int(n), self.A), np.float32)
        check(self._fn("_act_fetch")(self._h, int(first_agent), ctypes.c_int32(int(n)), fptr(out)))
        return out

    # ---- learning -------------------------------------------------------------------------
    def update(self, n_updates=1, host_indices=None, eps=None):
        idx = None
        if host_indices is not None:
            idx = np.ascontiguousarray(host_indices, np.int64)
            if idx.size != self.n_agents * int(n_updates) * self.B:
                raise ValueError("host_indices must hold n_agents*n_updates*batch_size entries")
        args = (self._h, ctypes.c_int32(int(n_updates)), _opt(iptr, idx))
        if self.EPS:
            e = None
            if eps is not None:
                e = np.ascontiguousarray(eps, np.float32)
                if e.size != self.n_agents * int(n_updates) * self.B * self.A:
                    raise ValueError("eps must hold n_agents*n_updates*batch_size*action_dim entries")
            args += (_opt(fptr, e),)
        elif eps is not None:
            raise TypeError("update() of this algorithm takes no eps")
        check(self._fn("_update")(*args))

    def update_batch(self, agent, states, actions, next_states, rewards, gammas, eps=None):
        r = f64(rewards).reshape(-1)
        n = r.size
        s, s2 = f64(states).reshape(n, self.S), f64(next_states).reshape(n, self.S)
        a, g = f64(actions).reshape(n, self.A), f64(gammas).reshape(n)
        args = (self._h, int(agent), ctypes.c_int32(n), dptr(s), dptr(a), dptr(s2), dptr(r), dptr(g))
        if self.EPS:
            args += (_opt(fptr, None if eps is None else np.ascontiguousarray(eps, np.float32).reshape(n, self.A)),)
        elif eps is not None:
            raise TypeError("update_batch() of this algorithm takes no eps")
        check(self._fn("_update_batch")(*args))

    def set_kernel(self, name):
        check(self._fn("_set_kernel")(self._h, self.KERNEL[name]))

    def kernel_in_use(self):
        out = ctypes.c_int32(0)
        check(self._fn("_get_kernel")(self._h, ctypes.byref(out)))
        return {v: k for k, v in self.KERNEL.items()}[out.value]

    def set_split(self, n_workgroups):
        """latency mode: every agent's update over n_workgroups CUs (1 = off); MFMA shapes of DDPG and the KL agents"""
        check(self._fn("_set_split")(self._h, ctypes.c_int32(int(n_workgroups))))

    def debug_fail_next_split(self):
        """test hook: the next latency-mode launch finds its barrier error word set (include/rlcontrol_hip.h)"""
        check(self._lib.rlc_debug_fail_next_split(self._h))

    def enable_grad_taps(self, on=True):
        check(self._fn("_enable_grad_taps")(self._h, 1 if on else 0))

    def last_tap(self, agent, which):
        n = self.tap_lengths()[which]
        out = np.empty(n, np.float32)
        check(self._fn("_last_tap")(self._h, int(agent), self.TAP[which], fptr(out), ctypes.c_int64(n)))
        return out

    # ---- replay ---------------------------------------------------------------------------
    def replay_add(self, agent, state, action, reward, next_state, transition_gamma):
        s, a, s2 = f64(state).reshape(-1), f64(action).reshape(-1), f64(next_state).reshape(-1)
        if s.size != self.S or s2.size != self.S or a.size != self.A:
            raise ValueError("transition shapes do not match state_dim/action_dim")
        check(self._lib.rlc_replay_add(self._h, int(agent), dptr(s), dptr(a), ctypes.c_double(float(reward)),
                                       dptr(s2), ctypes.c_double(float(transition_gamma))))

    def replay_add_batch(self, agent, states, actions, rewards, next_states, gammas):
        r = f64(rewards).reshape(-1)
        n = r.size
        s, s2 = f64(states).reshape(n, self.S), f64(next_states).reshape(n, self.S)
        a, g = f64(actions).reshape(n, self.A), f64(gammas).reshape(n)
        check(self._lib.rlc_replay_add_batch(self._h, int(agent), ctypes.c_int64(n), dptr(s), dptr(a), dptr(r),
                                             dptr(s2), dptr(g)))

    def replay_fill_all_dev(self, n, s_ptr, a_ptr, r_ptr, s2_ptr, g_ptr):
        """device pointers (ints), e.g. torch tensor .data_ptr(): fp32 s/a/s2, fp64 r/gamma"""
        vp = ctypes.c_void_p
        check(self._lib.rlc_replay_fill_all_dev(self._h, ctypes.c_int64(int(n)), vp(s_ptr), vp(a_ptr), vp(r_ptr),
                                                vp(s2_ptr), vp(g_ptr)))

    def replay_size(self, agent):
        out = ctypes.c_int64(0)
        check(self._lib.rlc_replay_size(self._h, int(agent), ctypes.byref(out)))
        return int(out.value)

    def replay_gather(self, agent, logical_idx):
        idx = np.ascontiguousarray(logical_idx, np.int64).reshape(-1)
        k = idx.size
        s, s2 = np.empty((k, self.S)), np.empty((k, self.S))
        a, r, g = np.empty((k, self.A)), np.empty(k), np.empty(k)
        check(self._lib.rlc_replay_gather(self._h, int(agent), iptr(idx), ctypes.c_int32(k), dptr(s), dptr(a),
                                          dptr(r), dptr(s2), dptr(g)))
        return s, a, r, s2, g

    def replay_sample_indices(self, agent, k):
        out = np.empty(int(k), np.int64)
        check(self._lib.rlc_replay_sample_indices(self._h, int(agent), ctypes.c_int32(int(k)), iptr(out)))
        return out

    # ---- timing ---------------------------------------------------------------------------
    def timer_begin(self):
        check(self._lib.rlc_timer_begin(self._h))

    def timer_end(self):
        ms = ctypes.c_float(0.0)
        check(self._lib.rlc_timer_end(self._h, ctypes.byref(ms)))
        return float(ms.value)


class SampledPolicyPopulation(Population):
    """SoftActorCritic and the KL agents: a Gaussian policy that acts with an optional sample (eps injected or drawn on
    the device) and whose updates take injected draws too"""
    EPS = True
    BLOB = {"theta": 0, "theta_target": 1, "adam_m": 2, "adam_v": 3}

    def _act_args(self, states, first_agent, sample, eps):
        s = f64(states).reshape(-1, self.S)
        e = None if eps is None else np.ascontiguousarray(eps, np.float32).reshape(s.shape[0], self.A)
        return s, (self._h, int(first_agent), ctypes.c_int32(s.shape[0]), dptr(s), ctypes.c_int32(1 if sample else 0),
                   _opt(fptr, e))

    def act(self, states, first_agent=0, sample=False, eps=None):
        s, args = self._act_args(states, first_agent, sample, eps)
        out = np.empty((s.shape[0], self.A), np.float32)
        check(self._fn("_act")(*(args + (fptr(out),))))
        return out

    def act_queue(self, states, first_agent=0, sample=False, eps=None):
        """queue the acting forward for `states` behind the work already on the handle's stream (no synchronisation)"""
        s, args = self._act_args(states, first_agent, sample, eps)
        check(self._fn("_act_queue")(*args))
        return s.shape[0]
