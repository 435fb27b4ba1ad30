"""Restatement of the reference's ActorCritic agent in torch (test infrastructure): agents/ActorCritic.py:116-263 and
agents/network/ac_network.py:124-288, 322-334, built the way the reference runs it -- B*n stacked rows through the Q
network, B, B*n or B*k stacked rows through the actor, the loss mean(-logp * w) with logp = the diagonal normal's
log-density of the raw action minus the tanh-correction term -- with autograd for the gradients.  fp32 by default (what
the kernel is compared with), float64 on request (the twin both are held to).

Parity status: parity unpinned -- no reference fixture exercises this agent.  The TF-1.15 Adam arithmetic, the loss
scaling and the Polyak average are those of tests/torch_ref_ae.py (tests/torch_ref_optq.py, which tests/test_optq.py
ties to the C oracle).  The draws are the caller's standard normals (they stand for TF's random ops).

Deliberate difference: among bit-equal Q values the lower sample index ranks first (a stable sort of -q); the
reference's argsort()[::-1] orders exact ties the other way round, which only matters between different actions.
"""
from collections import OrderedDict

import numpy as np
import torch

from torch_ref_ae import select

NAMES = ("W1", "b1", "Wp2", "bp2", "Wmu", "bmu", "Wls", "bls", "Wal", "bal", "Wq2", "bq2", "Wq3", "bq3")
ALPHA_HEAD = ("Wal", "bal")                        # in the blob and in Polyak; no gradient, no moments
ACTOR_ONLY = ("Wp2", "bp2", "Wmu", "bmu", "Wls", "bls")
CRITIC_ONLY = ("Wq2", "bq2", "Wq3", "bq3")
CRITIC_UPDATES = ("mean", "sampled", "expected")
ACTOR_UPDATES = ("ll", "ll_update_all", "cem")


def layout(dims):
    """name -> (offset, shape): variable creation order (ac_network.py:124-288)"""
    S, A, L1, La, Lc = dims
    out, p = OrderedDict(), 0
    for name, shp in (("W1", (S, L1)), ("b1", (L1,)), ("Wp2", (L1, La)), ("bp2", (La,)), ("Wmu", (La, A)), ("bmu", (A,)),
                      ("Wls", (La, A)), ("bls", (A,)), ("Wal", (La, 1)), ("bal", (1,)), ("Wq2", (L1 + A, Lc)),
                      ("bq2", (Lc,)), ("Wq3", (Lc, 1)), ("bq3", (1,))):
        out[name] = (p, shp)
        p += int(np.prod(shp))
    return out, p


def init_params(dims, seed):
    """U(+-sqrt(3 / fan_in)) weights and biases; Wls U(0, 1); bls, Wal, bal, Wq3, bq3 U(+-3e-3) (ac_network.py:127-287)"""
    rng = np.random.RandomState(seed)
    lay, P = layout(dims)
    th = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        if name == "Wls":
            lo, hi = 0.0, 1.0
        elif name in ("bls", "Wal", "bal", "Wq3", "bq3"):
            lo, hi = -0.003, 0.003
        else:
            lo, hi = -np.sqrt(3.0 / shp[0]), np.sqrt(3.0 / shp[0])
        th[off:off + n] = rng.uniform(lo, hi, n).astype(np.float32)
    return th


def next_draws(critic_update, n):
    return {"mean": 0, "sampled": 1, "expected": n}[critic_update]


def logprob(mu, sigma, raw):
    """pi_actions_logprob (ac_network.py:240-242): MultivariateNormalDiag(mu, sigma).log_prob(raw) minus the
    tanh-correction term, which depends on the fed raw action alone"""
    z = (raw - mu) / sigma
    lp = torch.sum(-0.5 * z * z - torch.log(sigma) - 0.5 * np.log(2.0 * np.pi), dim=1)
    return lp - torch.sum(torch.log(torch.clamp(1.0 - torch.tanh(raw) ** 2, 0.0, 1.0) + 1e-6), dim=1)


class TorchActorCritic(object):
    """theta, theta_t, m_a, v_a (actor Adam), m_c, v_c (critic Adam): flat [P] tensors; pw: float32 [4] running beta
    powers {actor b1^t, b2^t, critic b1^t, b2^t}"""

    def __init__(self, dims, num_samples, top_k, critic_update, actor_update, theta, actor_lr, critic_lr, tau, state_min,
                 state_max, action_max, clip_state=True, dtype=torch.float32):
        assert critic_update in CRITIC_UPDATES and actor_update in ACTOR_UPDATES
        self.dims, self.dt = tuple(int(v) for v in dims), dtype
        self.n, self.k = int(num_samples), int(top_k)
        self.critic_update, self.actor_update = critic_update, actor_update
        self.layout, self.P = layout(self.dims)
        self.theta = torch.as_tensor(np.asarray(theta, np.float32).copy()).to(dtype)
        self.theta_t = self.theta.clone()
        for name in ("m_a", "v_a", "m_c", "v_c"):
            setattr(self, name, torch.zeros(self.P, dtype=dtype))
        self.pw = np.array([0.9, 0.999, 0.9, 0.999], np.float32)
        self.actor_lr, self.critic_lr, self.tau = float(actor_lr), float(critic_lr), float(tau)
        S, A = self.dims[:2]
        as_t = lambda v, n: torch.as_tensor(np.broadcast_to(np.asarray(v, np.float32), (n,)).copy()).to(dtype)
        self.smin, self.smax, self.amax = as_t(state_min, S), as_t(state_max, S), as_t(action_max, A)
        self.clip = bool(clip_state)
        self.mask_a, self.mask_c = torch.zeros(self.P, dtype=torch.bool), torch.zeros(self.P, dtype=torch.bool)
        for name, (off, shp) in self.layout.items():
            n = int(np.prod(shp))
            # TF's minimize skips variables whose gradient is None: the alpha head belongs to neither optimizer
            self.mask_a[off:off + n] = name not in CRITIC_ONLY and name not in ALPHA_HEAD
            self.mask_c[off:off + n] = name not in ACTOR_ONLY and name not in ALPHA_HEAD

    # ---- network --------------------------------------------------------------------------
    def _views(self, flat):
        return {k: flat[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in self.layout.items()}

    def _t(self, x, shape):
        return torch.as_tensor(np.asarray(x, np.float64)).to(self.dt).reshape(shape)

    def _x(self, s):
        x = torch.as_tensor(np.asarray(s, np.float32)).to(self.dt).reshape(-1, self.dims[0])
        return torch.max(torch.min(x, self.smax), self.smin) if self.clip else x

    def _h1(self, P, x):
        return torch.relu(x @ P["W1"] + P["b1"])

    def _actor(self, P, h1):
        """(mu [R][A], linear; sigma [R][A])"""
        hp = torch.relu(h1 @ P["Wp2"] + P["bp2"])
        return hp @ P["Wmu"] + P["bmu"], torch.exp(-20.0 + 11.0 * (torch.tanh(hp @ P["Wls"] + P["bls"]) + 1.0))

    def _q(self, P, h1, a):
        return (torch.relu(torch.cat([h1, a], dim=1) @ P["Wq2"] + P["bq2"]) @ P["Wq3"] + P["bq3"]).reshape(-1)

    def _np(self, t):
        return t.detach().to(torch.float64).numpy().copy()

    def _down(self, v):
        """a value the reference holds as a float32 numpy array between two session runs"""
        return np.asarray(v, np.float32).astype(np.float64) if self.dt == torch.float32 else np.asarray(v, np.float64)

    def _sample(self, mu, sigma, eps):
        """mvn.sample then tanh and the scale (ac_network.py:221-237): mu, sigma [R][A] tensors, eps [R][j][A] ->
        (raw, squashed) [R][j][A] tensors of the network's dtype"""
        e = torch.as_tensor(np.asarray(eps, np.float32)).to(self.dt)
        raw = mu.unsqueeze(1) + sigma.unsqueeze(1) * e
        return raw, torch.tanh(raw) * self.amax

    def modal(self, states):
        with torch.no_grad():
            P = self._views(self.theta)
            return tuple(self._np(v) for v in self._actor(P, self._h1(P, self._x(states))))

    def act(self, states):
        """predict_action (ac_network.py:449-472): tanh(mu) * action_max"""
        with torch.no_grad():
            P = self._views(self.theta)
            mu, _ = self._actor(P, self._h1(P, self._x(states)))
            return self._np(torch.tanh(mu) * self.amax)

    def sample(self, states, eps):
        """one draw per state: eps [R][A]"""
        with torch.no_grad():
            P = self._views(self.theta)
            mu, sigma = self._actor(P, self._h1(P, self._x(states)))
            return self._np(self._sample(mu, sigma, np.reshape(eps, (mu.shape[0], 1, -1)))[1])[:, 0]

    def qval(self, states, actions):
        with torch.no_grad():
            P = self._views(self.theta)
            x = self._x(states)
            return self._np(self._q(P, self._h1(P, x), self._t(actions, (x.shape[0], self.dims[1]))))

    # ---- one update -----------------------------------------------------------------------
    def _adam(self, g, m, v, lr, pw, mask):
        b1p, b2p = np.float32(pw[0]), np.float32(pw[1])                             # TF-1.15 ApplyAdam
        lr_t = float(np.float32(lr) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p))
        m[mask] += ((g - m) * float(np.float32(1) - np.float32(0.9)))[mask]
        v[mask] += ((g * g - v) * float(np.float32(1) - np.float32(0.999)))[mask]
        self.theta[mask] -= ((m * lr_t) / (torch.sqrt(v) + 1e-8))[mask]

    def weights(self, sq):
        """the constants of the actor loss from the samples' Q [B][n] (as the reference holds them: numpy of the
        network's precision): (w [B][n], R)"""
        B, n = sq.shape
        if self.actor_update == "cem":
            w = np.zeros((B, n))
            w[np.arange(B)[:, None], select(sq, self.k)] = 1.0
            return w, B * self.k
        dt = np.float32 if self.dt == torch.float32 else np.float64
        q = sq.astype(dt)
        w = (q - np.mean(q, axis=1, keepdims=True)).astype(np.float64)              # ActorCritic.py:210, :223
        if self.actor_update == "ll":
            w[:, 1:] = 0.0
            return w, B
        return w, B * n

    def update(self, s, a, s2, r, gam, eps_next, eps, taps=False, stop_after_critic=False):
        S, A, L1, La, Lc = self.dims
        n = self.n
        B = len(np.reshape(r, -1))
        x, x2 = self._x(s), self._x(s2)
        nd = next_draws(self.critic_update, n)
        # 1: a' from the ONLINE actor on s', y from the TARGET Q (ActorCritic.py:123-167)
        with torch.no_grad():
            P, Pt = self._views(self.theta), self._views(self.theta_t)
            mu2, sig2 = self._actor(P, self._h1(P, x2))
            if nd == 0:
                a_next = (torch.tanh(mu2) * self.amax).unsqueeze(1)
            else:
                a_next = self._sample(mu2, sig2, np.reshape(eps_next, (B, nd, A)))[1]
            nn = a_next.shape[1]
            a_next = self._down(self._np(a_next))                                    # [B][nn][A]
            q_next = self._np(self._q(Pt, self._h1(Pt, x2).repeat_interleave(nn, dim=0), self._t(a_next, (B * nn, A))))
            dt = np.float32 if self.dt == torch.float32 else np.float64
            q_next = np.mean(q_next.reshape(B, nn).astype(dt), axis=1).astype(np.float64)
        y64 = np.asarray(r, np.float64).reshape(B) + np.asarray(gam, np.float64).reshape(B) * q_next
        y = torch.as_tensor(self._down(y64)).to(self.dt)                            # the placeholder is float32 (:56)
        # 2: critic step
        theta = self.theta.clone().requires_grad_(True)
        P = self._views(theta)
        q = self._q(P, self._h1(P, x), self._t(a, (B, A)))
        g_c = torch.autograd.grad(torch.mean((y - q) ** 2), theta)[0]
        with torch.no_grad():
            self._adam(g_c, self.m_c, self.v_c, self.critic_lr, self.pw[2:4], self.mask_c)
            if stop_after_critic:
                return None
            # 3: the sampling pass on the weights after the critic step, Q of every sample (B*n stacked rows)
            P = self._views(self.theta)
            h1 = self._h1(P, x)
            mu, sigma = self._actor(P, h1)
            raw, sa = self._sample(mu, sigma, np.reshape(eps, (B, n, A)))
            raw, sa = self._down(self._np(raw)), self._down(self._np(sa))            # [B][n][A]
            sq = self._down(self._np(self._q(P, h1.repeat_interleave(n, dim=0), self._t(sa, (B * n, A)))).reshape(B, n))
            w, R = self.weights(sq)
        # 4: actor step on the stacked rows that carry weight (ActorCritic.py:203-254)
        rows_b, rows_j = np.nonzero(np.ones_like(w)) if self.actor_update == "ll_update_all" else (
            (np.arange(B), np.zeros(B, int)) if self.actor_update == "ll" else np.nonzero(w))
        assert len(rows_b) == R
        theta = self.theta.clone().requires_grad_(True)
        P = self._views(theta)
        mu_t, sig_t = self._actor(P, self._h1(P, x[rows_b]))
        lp = logprob(mu_t, sig_t, self._t(raw[rows_b, rows_j], (R, A)))
        loss = torch.mean(-lp * self._t(w[rows_b, rows_j], (R,)))
        g_a = torch.autograd.grad(loss, theta)[0]
        with torch.no_grad():
            self._adam(g_a, self.m_a, self.v_a, self.actor_lr, self.pw[0:2], self.mask_a)
            self.pw *= np.array([0.9, 0.999, 0.9, 0.999], np.float32)
            self.theta_t += self.tau * (self.theta - self.theta_t)                  # assign_add (:69-71)
        if not taps:
            return None
        return {"q": self._np(q), "y": self._np(y), "a_next": a_next.reshape(-1), "raw_samples": raw.reshape(-1),
                "samples": sa.reshape(-1), "sample_q": sq.reshape(-1), "weights": w.reshape(-1),
                "grads_a": self._np(g_a), "grads_c": self._np(g_c), "mu": self._np(mu), "sigma": self._np(sigma),
                "sigma_next": self._np(sig2)}
