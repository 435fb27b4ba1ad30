"""Inputs shared by tests/test_ac.py (CPU) and tests/test_gpu_ac.py: the cases, the weights, the minibatches and draws,
the bars, the conditions on the inputs and the float64 form of the kernel's summed backward seeds.

Parity unpinned: no reference fixture exercises this agent; every bar below is the project's own."""
import numpy as np
import torch

import torch_ref_ac as R

ALR, CLR, TAU = 1e-3, 1e-2, 0.01
ASCALE = 100.0       # test weights: the factor on the action rows of Wq2 (theta_for_tests)

# ((S, A, L1, La, Lc, n, k), batch, critic_update, actor_update)
CASES = [((1, 1, 16, 16, 16, 1, 1), 2, "mean", "ll"),                     # w_0 = q_0 - q_0 = 0: a zero actor gradient
         ((3, 1, 32, 24, 20, 30, 6), 17, "sampled", "ll"),                # the shipped modes, ragged everywhere
         ((2, 2, 16, 20, 16, 65, 5), 5, "expected", "cem"),               # n one past a wave
         ((4, 6, 32, 32, 32, 10, 10), 9, "expected", "ll_update_all"),    # largest A; k = n
         ((3, 1, 200, 200, 200, 30, 6), 32, "sampled", "ll"),             # the shipped shape
         ((3, 1, 200, 200, 200, 30, 6), 100, "mean", "cem")]              # the shipped widths at batch 100

# project bars (relative to the largest element of the float64 twin's quantity, _rel below)
BAR_TAP, BAR_GRAD, BAR_LATER = 1e-5, 5e-5, 2e-4
TAPS = ("q", "y", "a_next", "raw_samples", "samples", "sample_q", "weights")

# For every case the first seed of range(200) whose three updates (weights theta_for_tests(dims, 3), a target apart, then
# batch / draws per update from RandomState(seed)) satisfy the conditions of condition_failures below at every update:
# what find_seed(case, 3, range(200)) returns.
CASE_SEEDS = dict(zip(CASES, (0, 0, 0, 0, 0, 4)))


def case_id(v):
    if isinstance(v, tuple) and len(v) == 4 and isinstance(v[0], tuple):
        return "%s-B%d-%s-%s" % (("x".join(map(str, v[0])),) + tuple(v[1:]))
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def bounds(S, A):
    """state bounds inside the states' range (the clip is active), action scales that differ per dimension"""
    amax = np.linspace(1.0, 2.0, A) if A > 1 else np.array([2.0])
    return -np.ones(S) * 0.8, np.ones(S) * 0.8, amax


def theta_for_tests(dims, seed):
    """The reference's initialisers put every sigma at e^2 and make Q nearly flat in the action.  For the tests: the
    sigma head scaled and shifted so that sigma lies between 0.2 and 0.9 (its pre-activation in [0.85, 1.08]), Wq3 / bq3
    and the action rows of Wq2 scaled so that Q depends on the action; the alpha head scaled up so that a kernel that
    moved it would show."""
    net = dims[:5]
    th = R.init_params(net, seed)
    lay, _ = R.layout(net)
    rng = np.random.RandomState(seed + 1000)
    for name, scale, shift in (("Wls", 0.001, 0.0), ("bls", 0.0, 0.95), ("Wal", 100.0, 0.0), ("bal", 100.0, 0.0),
                               ("Wq3", 100.0, 0.0), ("bq3", 100.0, 0.0)):
        off, shp = lay[name]
        n = int(np.prod(shp))
        th[off:off + n] = th[off:off + n] * scale + shift
        if name == "bls":
            th[off:off + n] += rng.uniform(-0.1, 0.1, n).astype(np.float32)
    off, shp = lay["Wq2"]
    th[off + net[2] * shp[1]:off + shp[0] * shp[1]] *= ASCALE
    return th


def oracle(case, theta, dtype=torch.float32, lr=(ALR, CLR)):
    dims, _, cu, au = case
    smin, smax, amax = bounds(dims[0], dims[1])
    return R.TorchActorCritic(dims[:5], dims[5], dims[6], cu, au, theta, lr[0], lr[1], TAU, smin, smax, amax, dtype=dtype)


def batch(rng, dims, B):
    """states in [-1, 1], actions inside the action range, rewards in [-16, 0]; update()'s order (s, a, s2, r, gamma)"""
    S, A = dims[:2]
    amax = bounds(S, A)[2]
    return (rng.uniform(-1, 1, (B, S)), rng.uniform(-1, 1, (B, A)) * amax, rng.uniform(-1, 1, (B, S)), rng.uniform(-16, 0, B),
            np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def draws(rng, case):
    """(eps_next [B][n_next][A] or None, eps [B][n][A]) standard normal, float32: the agent's documented order"""
    dims, B, cu, _ = case
    nd = R.next_draws(cu, dims[5])
    eps_next = rng.standard_normal((B, nd, dims[1])).astype(np.float32) if nd else None
    return eps_next, rng.standard_normal((B, dims[5], dims[1])).astype(np.float32)


def target_apart(theta, rng):
    return (theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32)


def pair(case, rng, theta=None):
    """(theta, target, fp32 restatement, float64 twin), the target apart from theta"""
    theta = theta_for_tests(case[0], 3) if theta is None else theta
    target = target_apart(theta, rng)
    o32, o64 = oracle(case, theta), oracle(case, theta, torch.float64)
    for o in (o32, o64):
        o.theta_t = torch.as_tensor(target).to(o.dt)
    return theta, target, o32, o64


def checked(t32, t64, o32, o64, step):
    """every quantity the device is held to after update `step` (0-based): (label, fp32 restatement, twin, project bar);
    gradient tensors that are exactly zero in the twin (another optimizer's, the alpha head, case 1) are compared
    separately"""
    out = [("tap " + k, t32[k], t64[k], BAR_TAP if step == 0 else BAR_LATER) for k in TAPS]
    out.append(("theta_target", o32.theta_t.numpy(), o64.theta_t.numpy(), BAR_TAP if step == 0 else BAR_LATER))
    for which in ("grads_c", "grads_a"):
        for name, (off, shp) in o32.layout.items():
            sl = slice(off, off + int(np.prod(shp)))
            if np.any(t64[which][sl]):
                out.append(("%s %s" % (which, name), t32[which][sl], t64[which][sl], BAR_GRAD if step == 0 else BAR_LATER))
    return out


def bound(e_ref, bar):
    """max(project bar, 3 x the fp32 restatement's own error against the twin), never above 4 x the project bar"""
    return min(max(bar, 3.0 * e_ref), 4.0 * bar)


def condition_failures(case, t32, t64, o32, o64, step):
    """the conditions on a case's inputs, from the restatement's and the twin's taps of one update; [] when all hold"""
    dims, B, cu, au = case
    S, A, L1, La, Lc, n, k = dims
    out = []
    for label, ref, twin, bar in checked(t32, t64, o32, o64, step):                 # (1) the restatement inside the cap
        e = _rel(ref, twin)
        if e > bar * 4.0 / 3.0:
            out.append("1: %s restatement %.3e > 4/3 x %.0e" % (label, e, bar))
    if au == "cem" and k < n:                                                      # (2) the selection is well posed
        sq, sa = t32["sample_q"].reshape(B, n), t32["samples"].reshape(B, n, A)
        scale = float(np.max(np.abs(sq)))
        for b in range(B):
            order = np.argsort(-sq[b], kind="stable")
            last_in, first_out = order[k - 1], order[k]                            # the k-th and (k+1)-th largest q
            if np.array_equal(sa[b][last_in], sa[b][first_out]):
                continue                                                           # the same action
            if sq[b][last_in] - sq[b][first_out] <= 1e-4 * scale:
                out.append("2: row %d gap %.3e" % (b, (sq[b][last_in] - sq[b][first_out]) / scale))
    if au == "cem" and not np.array_equal(t32["weights"], t64["weights"]):
        out.append("2: the restatement and its twin select different sets")
    for name in ("sigma", "sigma_next"):                                           # (3)
        if np.min(t32[name]) < 0.2 or np.max(t32[name]) > 0.9:
            out.append("3: %s in [%.3f, %.3f]" % (name, np.min(t32[name]), np.max(t32[name])))
    return out


def steps(case, seed, n_updates=3):
    """the case's schedule: yields (step, minibatch, eps_next, eps, t32, t64, o32, o64) after every update of the
    restatement and its twin; the first item yielded before any update is (theta, target)"""
    rng = np.random.RandomState(seed)
    theta, target, o32, o64 = pair(case, rng)
    yield theta, target
    for step in range(n_updates):
        b = batch(rng, case[0], case[1])
        eps_next, eps = draws(rng, case)
        t32 = o32.update(*b, eps_next, eps, taps=True)
        t64 = o64.update(*b, eps_next, eps, taps=True)
        yield step, b, eps_next, eps, t32, t64, o32, o64


def find_seed(case, n_updates, seeds):
    """the first seed of `seeds` whose n_updates minibatches and draws satisfy every condition; None if there is none"""
    for seed in seeds:
        it = steps(case, seed, n_updates)
        next(it)
        if all(not condition_failures(case, t32, t64, o32, o64, step) for step, _, _, _, t32, t64, o32, o64 in it):
            return seed
    return None


def seeds_float64(mu, sigma, raw, w, R_rows):
    """The kernel's summed backward seeds (rlcontrol_amd/csrc/ac_generic.hip) in numpy float64: the
    gradient of L = -(1 / R) sum_rows sum_j w_j logN(raw_j; mu, sigma) with respect to (mu [B][A], sigma [B][A]); raw
    [B][n][A], w [B][n]"""
    z = (raw - mu[:, None]) / sigma[:, None]
    G = -1.0 / R_rows
    return (G * np.sum(w[..., None] * z / sigma[:, None], axis=1),
            G * np.sum(w[..., None] * (z * z - 1.0) / sigma[:, None], axis=1))
