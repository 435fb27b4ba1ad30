"""Restatement of the reference's WireFitting agent in torch (test infrastructure): agents/WireFitting.py:23-77 and
agents/network/wf_network.py:60-125, built the way the reference's graph is built (the action tiled against the wires,
the weights normalised before they multiply the wire values) with autograd for the gradients.  fp32 by default (what the
kernel is compared with), float64 on request (the twin both are held to).

Parity status: parity unpinned -- no reference fixture exercises this agent.  The TF-1.15 Adam arithmetic, the loss
scaling and the Polyak average are those of tests/torch_ref_optq.py, which tests/test_optq.py ties to the C oracle.
"""
from collections import OrderedDict

import numpy as np
import torch

SMOOTH_EPS = 0.00001                                  # wf_network.py:27


def layout(dims):
    """name -> (offset, shape): variable creation order (wf_network.py:76-92,116)"""
    S, A, L1, L2, N = dims
    out, p = OrderedDict(), 0
    for name, shp in (("W1", (S, L1)), ("b1", (L1,)), ("W2", (L1, L2)), ("b2", (L2,)), ("Wa", (L2, N * A)), ("ba", (N * A,)),
                      ("Wq", (L2, N)), ("bq", (N,)), ("kappa", (N,))):
        out[name] = (p, shp)
        p += int(np.prod(shp))
    return out, p


def init_params(dims, seed):
    """Xavier-uniform hidden weights, U(-1, 1) head weights, zero biases, U(+-3e-3) smooth_c (wf_network.py:76-92,115)"""
    rng = np.random.RandomState(seed)
    lay, P = layout(dims)
    th = np.zeros(P, np.float32)
    for name, (off, shp) in lay.items():
        lim = {"W1": np.sqrt(6.0 / sum(shp)), "W2": np.sqrt(6.0 / sum(shp)), "Wa": 1.0, "Wq": 1.0, "kappa": 0.003}.get(name)
        if lim is not None:
            n = int(np.prod(shp))
            th[off:off + n] = rng.uniform(-lim, lim, n).astype(np.float32)
    return th


def interpolate(ahat, qhat, a, kappa):
    """create_interpolation (wf_network.py:106-125): ahat [n][N][A], qhat [n][N], a [n][A], kappa [N] -> Q [n]"""
    N = qhat.shape[1]
    tiled = a.repeat(1, N).reshape(-1, N, a.shape[1])                           # tf.tile + reshape (:109-110)
    act_distance = torch.sum((tiled - ahat) ** 2, dim=2)
    max_q = torch.max(qhat, dim=1).values                                       # gradient to the arg-max wire
    q_distance = torch.sigmoid(kappa).reshape(1, N) * (max_q.reshape(-1, 1) - qhat)
    distance = act_distance + q_distance + SMOOTH_EPS
    weight = 1.0 / distance
    weight_final = weight / torch.sum(weight, dim=1, keepdim=True)
    return torch.sum(weight_final * qhat, dim=1)


class TorchWireFitting(object):
    """theta, theta_t, m, v: flat [P] tensors; pw: float32 [2] running beta powers"""

    def __init__(self, dims, theta, learning_rate, tau, state_min, state_max, action_max0, clip_state=True,
                 dtype=torch.float32):
        self.dims, self.dt = tuple(int(v) for v in dims), dtype
        self.layout, self.P = layout(self.dims)
        self.theta = torch.as_tensor(np.asarray(theta, np.float32).copy()).to(dtype)
        self.theta_t = self.theta.clone()
        self.m, self.v = torch.zeros(self.P, dtype=dtype), torch.zeros(self.P, dtype=dtype)
        self.pw = np.array([0.9, 0.999], np.float32)
        self.lr, self.tau = float(learning_rate), float(tau)
        S = self.dims[0]
        self.smin = torch.as_tensor(np.broadcast_to(np.asarray(state_min, np.float32), (S,)).copy()).to(dtype)
        self.smax = torch.as_tensor(np.broadcast_to(np.asarray(state_max, np.float32), (S,)).copy()).to(dtype)
        self.amax0 = float(np.float32(action_max0))
        self.clip = bool(clip_state)

    def _views(self, flat):
        return {k: flat[o:o + int(np.prod(s))].reshape(s) for k, (o, s) in self.layout.items()}

    def _t(self, x, shape):
        return torch.as_tensor(np.asarray(x, np.float32)).to(self.dt).reshape(shape)

    def _x(self, s):
        x = self._t(s, (-1, self.dims[0]))
        return torch.max(torch.min(x, self.smax), self.smin) if self.clip else x      # wf_network.py:73-74

    def _wires(self, P, x):
        """build_network (wf_network.py:76-92): wire actions [n][N][A], wire values [n][N]"""
        A, N = self.dims[1], self.dims[4]
        h1 = torch.relu(x @ P["W1"] + P["b1"])
        h2 = torch.relu(h1 @ P["W2"] + P["b2"])
        ahat = torch.tanh(h2 @ P["Wa"] + P["ba"]) * self.amax0
        return ahat.reshape(-1, N, A), h2 @ P["Wq"] + P["bq"]

    def _np(self, t):
        return t.detach().to(torch.float64).numpy().copy()

    def wires(self, states, target=False):
        """(wire actions [n][N][A], wire values [n][N]) as float64 numpy"""
        with torch.no_grad():
            ahat, qhat = self._wires(self._views(self.theta_t if target else self.theta), self._x(states))
            return self._np(ahat), self._np(qhat)

    def act(self, states):
        """the arg-max wire's action [n][A] (predict_action, wf_network.py:97-102,136-143): np.argmax = lowest index"""
        ahat, qhat = self.wires(states)
        idx = np.argmax(qhat, axis=1)
        return ahat[np.arange(len(idx)), idx], idx

    def qval(self, states, actions):
        with torch.no_grad():
            P = self._views(self.theta)
            x = self._x(states)
            ahat, qhat = self._wires(P, x)
            return self._np(interpolate(ahat, qhat, self._t(actions, (x.shape[0], self.dims[1])), P["kappa"]))

    def update(self, s, a, s2, r, gam, taps=False):
        A = self.dims[1]
        B = len(np.reshape(r, -1))
        with torch.no_grad():                                                   # WireFitting.py:69
            max_q = torch.max(self._wires(self._views(self.theta_t), self._x(s2))[1], dim=1).values
        max_q = self._np(max_q) if self.dt == torch.float64 else max_q.numpy().copy()
        y64 = np.asarray(r, np.float64).reshape(B) + np.asarray(gam, np.float64).reshape(B) * np.asarray(max_q, np.float64)
        # the placeholder is float32 (wf_network.py:62); the twin keeps float64
        y = torch.as_tensor(y64 if self.dt == torch.float64 else y64.astype(np.float32)).to(self.dt)
        theta = self.theta.clone().requires_grad_(True)
        P = self._views(theta)
        ahat, qhat = self._wires(P, self._x(s))
        q = interpolate(ahat, qhat, self._t(a, (B, A)), P["kappa"])
        loss = torch.mean((y - q) ** 2)                                         # tf.losses.mean_squared_error (:63)
        g = torch.autograd.grad(loss, theta)[0]
        with torch.no_grad():
            b1p, b2p = np.float32(self.pw[0]), np.float32(self.pw[1])           # TF-1.15 ApplyAdam
            lr_t = float(np.float32(self.lr) * np.sqrt(np.float32(1) - b2p) / (np.float32(1) - b1p))
            # (1 - beta) is formed in float32, as ApplyAdam forms T(1) - beta: 1 - 0.999f is 0.99998712e-3, not 1e-3
            self.m += (g - self.m) * float(np.float32(1) - np.float32(0.9))
            self.v += (g * g - self.v) * float(np.float32(1) - np.float32(0.999))
            self.theta -= (self.m * lr_t) / (torch.sqrt(self.v) + 1e-8)
            self.pw *= np.array([0.9, 0.999], np.float32)
            self.theta_t += self.tau * (self.theta - self.theta_t)              # assign_add (:56-58)
        if not taps:
            return None
        return {"q": self._np(q).reshape(-1), "y": self._np(y).reshape(-1), "max_q": np.asarray(max_q, np.float64).copy(),
                "grads": self._np(g).reshape(-1)}
