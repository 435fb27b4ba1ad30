"""Restatement of the reference's ActorExpert agent in torch (test infrastructure): agents/ActorExpert.py:116-185 and
agents/network/ae_network.py:138-229, 262-278, 409-496, built the way the reference runs it -- B*n stacked rows through
the Q network, B*k stacked rows through the actor, the density as a linear-space product, clip_by_value before the log --
with autograd for the gradients.  fp32 by default (what the kernel is compared with), float64 on request (the twin both
are held to).

Parity status: parity unpinned -- no reference fixture exercises this agent.  The TF-1.15 Adam arithmetic, the loss
scaling and the Polyak average are those of tests/torch_ref_optq.py, which tests/test_optq.py ties to the C oracle.

Deliberate difference: among bit-equal Q values the lower sample index ranks first (a stable sort of -q); the
reference's argsort()[::-1] orders exact ties the other way round, which only matters between different actions.
"""
from collections import OrderedDict

import numpy as np
import torch

NAMES = ("W1", "b1", "Wa2", "ba2", "Wm", "bm", "Ws", "bs", "Wal", "bal", "Wq2", "bq2", "Wq3", "bq3")
ACTOR_ONLY = ("Wa2", "ba2", "Wm", "bm", "Ws", "bs", "Wal", "bal")
EXPERT_ONLY = ("Wq2", "bq2", "Wq3", "bq3")


def layout(dims):
    """name -> (offset, shape): variable creation order (ae_network.py:138-229)"""
    S, A, L1, La, Le, M = dims
    out, p = OrderedDict(), 0
    for name, shp in (("W1", (S, L1)), ("b1", (L1,)), ("Wa2", (L1, La)), ("ba2", (La,)), ("Wm", (La, M * A)), ("bm", (M * A,)),
                      ("Ws", (La, M * A)), ("bs", (M * A,)), ("Wal", (La, M)), ("bal", (M,)), ("Wq2", (L1 + A, Le)),
                      ("bq2", (Le,)), ("Wq3", (Le, 1)), ("bq3", (1,))):
        out[name] = (p, shp)
        p += int(np.prod(shp))
    return out, p


def init_params(dims, seed):
    """U(+-sqrt(3 / fan_in)) weights and biases; Ws U(0, 1); bs, Wal, bal, Wq3, bq3 U(+-3e-3) (ae_network.py:140-227)"""
    rng = np.random.RandomState(seed)
    lay, P = layout(dims)
    th = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        n = int(np.prod(shp))
        if name == "Ws":
            lo, hi = 0.0, 1.0
        elif name in ("bs", "Wal", "bal", "Wq3", "bq3"):
            lo, hi = -0.003, 0.003
        else:
            lo, hi = -np.sqrt(3.0 / shp[0]), np.sqrt(3.0 / shp[0])
        th[off:off + n] = rng.uniform(lo, hi, n).astype(np.float32)
    return th


def modes_of(alpha, u):
    """RandomState.choice(M, n, p=alpha) for the uniforms u: searchsorted(cdf, u, side='right'), cdf = cumsum(alpha) /
    its last element, float64.  alpha [M], u [n] -> [n]"""
    cdf = np.cumsum(np.asarray(alpha, np.float64))
    cdf /= cdf[-1]
    return np.minimum(np.searchsorted(cdf, np.asarray(u, np.float64), side="right"), len(cdf) - 1)


def cdf_of(alpha):
    cdf = np.cumsum(np.asarray(alpha, np.float64), axis=-1)
    return cdf / cdf[..., -1:]


def select(q, k):
    """the k largest of every row of q [B][n], the lower index first among equal values; ascending indices [B][k]"""
    order = np.argsort(-np.asarray(q), axis=1, kind="stable")[:, :k]
    return np.sort(order, axis=1)


def tf_normal(y, mu, sigma):
    """ae_network.py:231-243: y [R][A], mu / sigma [R][M][A] -> [R][M]"""
    yy = y.unsqueeze(1).repeat(1, mu.shape[1], 1)
    return torch.prod(torch.sqrt(1.0 / (2 * np.pi * sigma ** 2)) * torch.exp(-(yy - mu) ** 2 / (2 * sigma ** 2)), dim=2)


def mixture_density(alpha, sigma, mean, action):
    return torch.sum(tf_normal(action, mean, sigma) * alpha, dim=1, keepdim=True)


def lossfunc(alpha, sigma, mean, action):
    """get_lossfunc (ae_network.py:262-278)"""
    return torch.mean(-torch.log(torch.clamp(mixture_density(alpha, sigma, mean, action), 1e-30, 1e30)))


class TorchActorExpert(object):
    """theta, theta_t, m_a, v_a (actor Adam), m_c, v_c (expert Adam): flat [P] tensors; pw: float32 [4] running beta
    powers {actor b1^t, b2^t, expert b1^t, b2^t}"""

    def __init__(self, dims, num_samples, top_k, theta, actor_lr, expert_lr, tau, state_min, state_max, action_min,
                 action_max, clip_state=True, dtype=torch.float32):
        self.dims, self.dt = tuple(int(v) for v in dims), dtype
        self.n, self.k = int(num_samples), int(top_k)
        self.layout, self.P = layout(self.dims)
        self.theta = torch.as_tensor(np.asarray(theta, np.float32).copy()).to(dtype)
        self.theta_t = self.theta.clone()
        for name in ("m_a", "v_a", "m_c", "v_c"):
            setattr(self, name, torch.zeros(self.P, dtype=dtype))
        self.pw = np.array([0.9, 0.999, 0.9, 0.999], np.float32)
        self.actor_lr, self.expert_lr, self.tau = float(actor_lr), float(expert_lr), float(tau)
        S, A = self.dims[:2]
        as_t = lambda v, n: torch.as_tensor(np.broadcast_to(np.asarray(v, np.float32), (n,)).copy()).to(dtype)
        self.smin, self.smax = as_t(state_min, S), as_t(state_max, S)
        self.amin, self.amax = as_t(action_min, A), as_t(action_max, A)
        self.clip = bool(clip_state)
        self.mask_a, self.mask_e = torch.zeros(self.P, dtype=torch.bool), torch.zeros(self.P, dtype=torch.bool)
        for name, (off, shp) in self.layout.items():
            n = int(np.prod(shp))
            self.mask_a[off:off + n] = name not in EXPERT_ONLY
            self.mask_e[off:off + n] = name not in ACTOR_ONLY

    # ---- network --------------------------------------------------------------------------
    def _views(self, flat):
        return {k: flat[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in self.layout.items()}

    def _t(self, x, shape):
        return torch.as_tensor(np.asarray(x, np.float64)).to(self.dt).reshape(shape)

    def _x(self, s):
        x = torch.as_tensor(np.asarray(s, np.float32)).to(self.dt).reshape(-1, self.dims[0])
        return torch.max(torch.min(x, self.smax), self.smin) if self.clip else x       # ae_network.py:130-131

    def _h1(self, P, x):
        return torch.relu(x @ P["W1"] + P["b1"])

    def _actor(self, P, h1):
        """(alpha [R][M], mean [R][M][A], sigma [R][M][A])"""
        A, M = self.dims[1], self.dims[5]
        ha = torch.relu(h1 @ P["Wa2"] + P["ba2"])
        mean = torch.tanh(ha @ P["Wm"] + P["bm"]).reshape(-1, M, A) * self.amax
        sigma = torch.exp(-20.0 + 11.0 * (torch.tanh(ha @ P["Ws"] + P["bs"]).reshape(-1, M, A) + 1.0))
        t = torch.tanh(ha @ P["Wal"] + P["bal"])
        e = torch.exp(t - torch.max(t, dim=1, keepdim=True).values)
        return e * (1.0 / torch.sum(e, dim=1, keepdim=True)), mean, sigma

    def _q(self, P, h1, a):
        return (torch.relu(torch.cat([h1, a], dim=1) @ P["Wq2"] + P["bq2"]) @ P["Wq3"] + P["bq3"]).reshape(-1)

    def _np(self, t):
        return t.detach().to(torch.float64).numpy().copy()

    def modal(self, states, target=False):
        """(alpha, mean, sigma) as float64 numpy"""
        with torch.no_grad():
            P = self._views(self.theta_t if target else self.theta)
            return tuple(self._np(v) for v in self._actor(P, self._h1(P, self._x(states))))

    def act(self, states):
        """predict_action (ae_network.py:409-435): the mean of the largest-alpha mode, np.argmax = lowest index"""
        alpha, mean, _ = self.modal(states)
        idx = np.argmax(alpha, axis=1)
        return mean[np.arange(len(idx)), idx]

    def draw(self, alpha, mean, sigma, u, eps):
        """sample_action (ae_network.py:485-488) of one row: alpha [M], mean / sigma [M][A] as the network's dtype put
        them out, u [n], eps [n][A] -> clipped actions [n][A] (float64 arithmetic, as numpy's)"""
        idx = modes_of(alpha, u)
        a = mean[idx] + sigma[idx] * np.asarray(eps, np.float64)
        return np.clip(a, self._np(self.amin), self._np(self.amax))

    def sample(self, states, u, eps):
        """one draw per state: u [R], eps [R][A]"""
        alpha, mean, sigma = self.modal(states)
        return np.stack([self.draw(alpha[i], mean[i], sigma[i], np.reshape(u, -1)[i:i + 1], np.reshape(eps, (len(alpha), 1, -1))[i])[0]
                         for i in range(len(alpha))])

    def qval(self, states, actions):
        with torch.no_grad():
            P = self._views(self.theta)
            x = self._x(states)
            return self._np(self._q(P, self._h1(P, x), self._t(actions, (x.shape[0], self.dims[1]))))

    # ---- one update -----------------------------------------------------------------------
    def _adam(self, g, m, v, lr, pw, mask):
        b1p, b2p = np.float32(pw[0]), np.float32(pw[1])                             # TF-1.15 ApplyAdam
        lr_t = float(np.float32(lr) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p))
        # (1 - beta) is formed in float32, as ApplyAdam forms T(1) - beta
        m[mask] += ((g - m) * float(np.float32(1) - np.float32(0.9)))[mask]
        v[mask] += ((g * g - v) * float(np.float32(1) - np.float32(0.999)))[mask]
        self.theta[mask] -= ((m * lr_t) / (torch.sqrt(v) + 1e-8))[mask]

    def update(self, s, a, s2, r, gam, u, eps, taps=False, stop_after_expert=False):
        S, A, L1, La, Le, M = self.dims
        n, k = self.n, self.k
        B = len(np.reshape(r, -1))
        f32 = self.dt == torch.float32
        down = (lambda v: np.asarray(v, np.float32).astype(np.float64)) if f32 else (lambda v: np.asarray(v, np.float64))
        x, x2 = self._x(s), self._x(s2)
        # 1-2: a' from the ONLINE actor on s', y from the TARGET Q (ActorExpert.py:138-154)
        with torch.no_grad():
            P, Pt = self._views(self.theta), self._views(self.theta_t)
            alpha2, mean2, _ = self._actor(P, self._h1(P, x2))
            best = torch.argmax(alpha2, dim=1)                                      # ties: the lowest index
            a_next = mean2[torch.arange(B), best]
            q_next = self._np(self._q(Pt, self._h1(Pt, x2), a_next))
        y64 = np.asarray(r, np.float64).reshape(B) + np.asarray(gam, np.float64).reshape(B) * down(q_next)
        y = torch.as_tensor(down(y64)).to(self.dt)                                  # the placeholder is float32 (:101)
        # 3: expert step
        theta = self.theta.clone().requires_grad_(True)
        P = self._views(theta)
        q = self._q(P, self._h1(P, x), self._t(a, (B, A)))
        g_e = torch.autograd.grad(torch.mean((y - q) ** 2), theta)[0]
        with torch.no_grad():
            self._adam(g_e, self.m_c, self.v_c, self.expert_lr, self.pw[2:4], self.mask_e)
            # 4: the sampling pass on the weights after the expert step
            P = self._views(self.theta)
            h1 = self._h1(P, x)
            alpha, mean, sigma = (self._np(v) for v in self._actor(P, h1))
            if stop_after_expert:
                return {"alpha": alpha}
            u, eps = np.asarray(u, np.float32).reshape(B, n), np.asarray(eps, np.float32).reshape(B, n, A)
            samples = down(np.stack([self.draw(alpha[b], mean[b], sigma[b], u[b], eps[b]) for b in range(B)]))
            # 5: Q of every sample (B*n stacked rows), the k largest per row
            sq = self._np(self._q(P, h1.repeat_interleave(n, dim=0), self._t(samples, (B * n, A)))).reshape(B, n)
            sel = select(down(sq), k)
        # 6: actor step on B*k stacked rows (ActorExpert.py:178-182)
        chosen = samples[np.arange(B)[:, None], sel].reshape(B * k, A)
        theta = self.theta.clone().requires_grad_(True)
        P = self._views(theta)
        al_t, mean_t, sig_t = self._actor(P, self._h1(P, x.repeat_interleave(k, dim=0)))
        act_t = self._t(chosen, (B * k, A))
        loss = lossfunc(al_t, sig_t, mean_t, act_t)
        g_a = torch.autograd.grad(loss, theta)[0]
        with torch.no_grad():
            logp = torch.log(mixture_density(al_t, sig_t, mean_t, act_t)).reshape(B, k)
            self._adam(g_a, self.m_a, self.v_a, self.actor_lr, self.pw[0:2], self.mask_a)
            self.pw *= np.array([0.9, 0.999, 0.9, 0.999], np.float32)
            self.theta_t += self.tau * (self.theta - self.theta_t)                  # assign_add (:84-86)
        if not taps:
            return None
        return {"q": self._np(q), "y": self._np(y), "a_next": self._np(a_next).reshape(-1), "samples": samples.reshape(-1),
                "sample_q": sq.reshape(-1), "selected": sel.reshape(-1).astype(np.float64), "actor_loss": self._np(loss).reshape(1),
                "grads_a": self._np(g_a), "grads_e": self._np(g_e),
                "alpha_next": self._np(alpha2), "alpha": alpha, "mean": mean, "sigma": sigma, "logp_selected": self._np(logp)}
