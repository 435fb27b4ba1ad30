"""Inputs shared by tests/test_ae.py (CPU) and tests/test_gpu_ae.py: the shapes, the weights, the minibatches and draws,
the conditions on the inputs and the float64 form of the kernel's summed backward seeds."""
import copy

import numpy as np
import torch

import torch_ref_ae as R

ALR, ELR, TAU = 1e-3, 1e-2, 0.01
ASCALE = 100.0       # test weights: the factor on the action rows of Wq2 (theta_for_tests)

# (S, A, L1, La, Le, M, n, k), batch
SHAPES = [((1, 1, 16, 16, 16, 1, 1, 1), 2),              # one sample, all selected (ae_plus's n and rho)
          ((3, 1, 32, 24, 20, 2, 30, 6), 17),            # ragged; ae_separate's n and rho
          ((2, 2, 16, 20, 16, 3, 65, 5), 5),             # n one past a wave; three modes
          ((4, 6, 32, 32, 32, 2, 10, 10), 9),            # largest A; k = n
          ((3, 1, 200, 200, 200, 1, 120, 6), 32),        # shipped
          ((3, 1, 200, 200, 200, 2, 120, 6), 100)]       # shipped widths, two modes


# For every case the first seed of range(200) whose three updates (weights theta_for_tests(dims, 3), a target apart, then
# batch / draws / nudge per update from RandomState(seed)) satisfy conditions (a) to (d) below on the fp32 restatement:
# what find_seed(dims, B, 3, range(200)) returns.  At the widest case most seeds fail condition (a) in one of its 300 rows.
CASE_SEEDS = dict(zip(SHAPES, (0, 0, 0, 0, 4, 47)))


def shape_id(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def bounds(S, A):
    """state bounds inside the states' range (the clip is active), action bounds that differ per dimension"""
    amax = np.linspace(1.0, 2.0, A) if A > 1 else np.array([2.0])
    return -np.ones(S) * 0.8, np.ones(S) * 0.8, -amax, amax


def theta_for_tests(dims, seed):
    """The reference's initialisers put every sigma at e^2, every alpha within 1e-3 of 1 / M and make Q nearly flat in the
    action.  For the tests: the sigma head scaled and shifted so that sigma lies between 0.2 and 0.9 (condition d:
    |log density| <= 40, and samples spread over the action range), the alpha head scaled so that the modes' weights
    differ (condition c), Wq3 / bq3 and the action rows of Wq2 scaled so that Q depends on the action (condition a)."""
    net = dims[:6]
    th = R.init_params(net, seed)
    lay, _ = R.layout(net)
    rng = np.random.RandomState(seed + 1000)
    for name, scale, shift in (("Ws", 0.01, 0.0), ("bs", 0.0, 1.0), ("Wal", 100.0, 0.0), ("bal", 100.0, 0.0),
                               ("Wq3", 100.0, 0.0), ("bq3", 100.0, 0.0)):
        off, shp = lay[name]
        n = int(np.prod(shp))
        th[off:off + n] = th[off:off + n] * scale + shift
        if name == "bs":
            th[off:off + n] += rng.uniform(-0.2, 0.2, n).astype(np.float32)
    off, shp = lay["Wq2"]
    th[off + net[2] * shp[1]:off + shp[0] * shp[1]] *= ASCALE
    return th


def oracle(dims, theta, dtype=torch.float32, lr=(ALR, ELR)):
    smin, smax, amin, amax = bounds(dims[0], dims[1])
    return R.TorchActorExpert(dims[:6], dims[6], dims[7], theta, lr[0], lr[1], TAU, smin, smax, amin, amax, dtype=dtype)


def batch(rng, dims, B):
    """states in [-1, 1], actions inside the action bounds, rewards in [-16, 0]; update()'s order (s, a, s2, r, gamma)"""
    S, A = dims[:2]
    amax = bounds(S, A)[3]
    return (rng.uniform(-1, 1, (B, S)), rng.uniform(-1, 1, (B, A)) * amax, rng.uniform(-1, 1, (B, S)), rng.uniform(-16, 0, B),
            np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def draws(rng, dims, B):
    """(u [B][n] uniform in [0, 1), eps [B][n][A] standard normal), float32"""
    return rng.random_sample((B, dims[6])).astype(np.float32), rng.standard_normal((B, dims[6], dims[1])).astype(np.float32)


def target_apart(theta, rng):
    return (theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32)


def nudge(o32, b, u):
    """condition (b): every u further than 1e-4 from every cdf entry of its row, on the restatement's weights after the
    expert step (a copy of the restatement takes that step); offending draws are moved 3e-4 off the entry"""
    alpha = copy.deepcopy(o32).update(*b, None, None, stop_after_expert=True)["alpha"]
    cdf = R.cdf_of(alpha)                                                          # [B][M]
    u = np.array(u, np.float32)
    for i in range(cdf.shape[1]):
        c = cdf[:, i:i + 1]
        near = np.abs(u.astype(np.float64) - c) <= 2e-4
        moved = np.where(c + 3e-4 < 1.0, c + 3e-4, c - 3e-4)
        u = np.where(near, moved, u).astype(np.float32)
    return u


def condition_failures(taps, dims, u):
    """conditions (a) to (d) of the tests' inputs, from the fp32 restatement's taps of one update; [] when all hold"""
    S, A, L1, La, Le, M, n, k = dims
    B = taps["q"].size
    out = []
    sq, sa = taps["sample_q"].reshape(B, n), taps["samples"].reshape(B, n, A)
    if k < n:                                                                      # (a)
        scale = float(np.max(np.abs(sq)))
        for b in range(B):
            order = np.argsort(-sq[b], kind="stable")
            last_in, first_out = order[k - 1], order[k]                            # the k-th and (k+1)-th largest q
            if np.array_equal(sa[b][last_in], sa[b][first_out]):
                continue                                                           # the same action (clipped to a bound)
            if sq[b][last_in] - sq[b][first_out] <= 1e-4 * scale:
                out.append("a: row %d gap %.3e" % (b, (sq[b][last_in] - sq[b][first_out]) / scale))
    cdf = R.cdf_of(taps["alpha"])                                                  # (b)
    gap = np.min(np.abs(np.asarray(u, np.float64).reshape(B, n, 1) - cdf[:, None, :]))
    if gap <= 1e-4:
        out.append("b: a draw %.3e from a cdf entry" % gap)
    if M > 1:                                                                      # (c)
        top = np.sort(taps["alpha_next"], axis=1)[:, -2:]
        if np.min(top[:, 1] - top[:, 0]) <= 1e-4:
            out.append("c: alpha gap %.3e" % np.min(top[:, 1] - top[:, 0]))
    lp = taps["logp_selected"]                                                     # (d)
    if not (np.all(np.isfinite(lp)) and np.min(lp) >= -40 and np.max(lp) <= 40):
        out.append("d: log density in [%.1f, %.1f]" % (np.min(lp), np.max(lp)))
    return out


def find_seed(dims, B, n_updates, seeds, theta_seed=3):
    """the first seed of `seeds` whose n_updates minibatches and draws satisfy every condition on the fp32 restatement;
    None if there is none"""
    for seed in seeds:
        rng = np.random.RandomState(seed)
        theta = theta_for_tests(dims, theta_seed)
        o = oracle(dims, theta)
        o.theta_t = torch.as_tensor(target_apart(theta, rng)).to(o.dt)
        ok = True
        for _ in range(n_updates):
            b = batch(rng, dims, B)
            u, eps = draws(rng, dims, B)
            u = nudge(o, b, u)
            if condition_failures(o.update(*b, u, eps, taps=True), dims, u):
                ok = False
                break
        if ok:
            return seed
    return None


def seeds_float64(alpha, mean, sigma, chosen):
    """The kernel's summed backward seeds (rlcontrol_amd/csrc/ae_generic.hip) in numpy float64: for every
    row the gradient of L = -(1 / (B k)) sum log clip(p, 1e-30, 1e30) with respect to (alpha [B][M], mean [B][M][A],
    sigma [B][M][A]), summed over the row's k chosen actions [B][k][A]; log space, responsibilities w_jm = alpha_m N_m / p"""
    B, k, A = chosen.shape
    z = (chosen[:, :, None, :] - mean[:, None]) / sigma[:, None]                    # [B][k][M][A]
    logc = np.log(alpha)[:, None] + np.sum(-0.5 * np.log(2 * np.pi) - np.log(sigma)[:, None] - 0.5 * z * z, axis=3)
    mx = logc.max(axis=2, keepdims=True)
    logp = mx[..., 0] + np.log(np.sum(np.exp(logc - mx), axis=2))
    inside = (logp >= np.log(1e-30)) & (logp <= np.log(1e30))
    w = np.exp(logc - logp[..., None]) * inside[..., None]                          # [B][k][M]
    G = -1.0 / (B * k)
    d_mean = G * np.sum(w[..., None] * z / sigma[:, None], axis=1)
    d_sigma = G * np.sum(w[..., None] * (z * z - 1.0) / sigma[:, None], axis=1)
    d_alpha = G * np.sum(w, axis=1) / alpha
    loss = G * np.sum(np.clip(logp, np.log(1e-30), np.log(1e30)))
    return loss, d_alpha, d_mean, d_sigma
