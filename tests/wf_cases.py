"""Inputs shared by tests/test_wf.py (CPU) and tests/test_gpu_wf.py: the shapes, the weights, the minibatches, the
tie-free condition and the float64 form of the kernel's backward seeds."""
import numpy as np
import torch

import torch_ref_wf as R

LR, TAU, AMAX0 = 1e-3, 0.01, 2.0

# (S, A, L1, L2, N), batch
SHAPES = [((1, 1, 16, 16, 1), 2),          # N = 1
          ((3, 1, 32, 24, 7), 17),         # ragged everything
          ((2, 2, 16, 20, 65), 5),         # N one past a wave
          ((4, 6, 32, 32, 10), 9),         # largest A
          ((5, 2, 48, 64, 33), 32),
          ((3, 1, 200, 200, 100), 32),     # shipped shape
          ((3, 1, 200, 200, 100), 100)]


def shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def bounds(S):
    return -np.ones(S) * 0.8, np.ones(S) * 0.8              # inside the states' range: the clip is active


def oracle(dims, theta, dtype=torch.float32, lr=LR):
    smin, smax = bounds(dims[0])
    return R.TorchWireFitting(dims, theta, lr, TAU, smin, smax, AMAX0, dtype=dtype)


def batch(rng, dims, B):
    """states in [-1, 1], actions in [-2, 2], rewards in [-16, 0]; update()'s order (s, a, s2, r, gamma)"""
    S, A = dims[:2]
    return (rng.uniform(-1, 1, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-1, 1, (B, S)), rng.uniform(-16, 0, B),
            np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def target_apart(theta, rng):
    return (theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32)


def on_a_wire(o32, b):
    """the minibatch with its actions placed on a wire of the fp32 restatement's online network: even rows on wire
    min(3, N - 1), odd rows on the arg-max wire (the 1e-5 floor of the distance, off and on the wire that carries M)"""
    ahat, qhat = o32.wires(b[0])
    n, N = qhat.shape
    wire = np.where(np.arange(n) % 2 == 0, min(3, N - 1), np.argmax(qhat, axis=1))
    return (b[0], ahat[np.arange(n), wire].astype(np.float32).astype(np.float64)) + tuple(b[2:])


def assert_tie_free(o, b, label=""):
    """a condition on the inputs, not a measurement: the top two wire values of every row, online on s and target on
    s', differ by more than 1e-4 max|qhat| (the gradient through the maximum goes to ONE wire on the device; TF splits
    it among exact ties)"""
    for states, target in ((b[0], False), (b[2], True)):
        q = o.wires(states, target)[1]
        if q.shape[1] < 2:
            continue
        top = np.sort(q, axis=1)[:, -2:]
        gap = float(np.min(top[:, 1] - top[:, 0])) / float(np.max(np.abs(q)))
        assert gap > 1e-4, (label, "target" if target else "online", gap)


def seeds_float64(ahat, qhat, a, kappa, y):
    """The kernel's backward seeds (rlcontrol_amd/csrc/wf_generic.hip) in numpy float64:
    (Q [n], dL/dqhat [n][N], dL/dahat [n][N][A], dL/dkappa [N]) of L = mean (y - Q)^2"""
    n, N = qhat.shape
    c = 1.0 / (1.0 + np.exp(-kappa))
    M = qhat.max(1)
    istar = qhat.argmax(1)
    diff = a[:, None, :] - ahat
    w = 1.0 / ((diff ** 2).sum(2) + c[None] * (M[:, None] - qhat) + R.SMOOTH_EPS)
    W = w.sum(1)
    Q = ((w / W[:, None]) * qhat).sum(1)
    g = 2.0 * (Q - y) / n
    e = -w ** 2 * (qhat - Q[:, None]) / W[:, None]
    dq = g[:, None] * (w / W[:, None] - c[None] * e)
    dq[np.arange(n), istar] += g * (c[None] * e).sum(1)
    da = -2.0 * g[:, None, None] * e[:, :, None] * diff
    dk = (g[:, None] * e * (c * (1.0 - c))[None] * (M[:, None] - qhat)).sum(0)
    return Q, dq, da, dk
