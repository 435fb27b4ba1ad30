"""The second half of every update kernel against the CPU oracles: Adam's m and v, the parameters after the step and the
Polyak average into a target that starts AWAY from the weights (tests/optimizer_state_checks.py, checks a to e).

Schedule of every case: set the weights, write a target that is theta + U(-0.05, 0.05), two warm-up updates on the GPU (m, v
non-zero, beta powers non-trivial), read the whole state back, copy it into a fresh oracle, one update on the same minibatch
on both sides with the gradient taps on, read the state back, check.  Selecting the kernel is a requirement: a refusal
fails the test.  DDPG's two optimizers each leave part of the blob alone; those ranges of m and v are filled with noise
first so that check d has bits to lose."""
import numpy as np
import pytest

import optimizer_state_checks as C
from optimizer_state_cases import population_cases, single_update_cases, tap_cases

pytestmark = pytest.mark.gpu


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _seed_state(case, pop, agent, theta, rng):
    spec = case.spec()
    pop.set_params(agent, theta, init_target=False)
    pop.set_blob(agent, "theta_target", case.target_apart(theta, rng))
    for slot, (mn, vn) in case.SLOTS.items():
        free = ~C._mask(spec.P, [r for o in spec.opts if o.slot == slot for r in o.ranges])
        if free.any():
            pop.set_blob(agent, mn, np.where(free, rng.uniform(-1e-3, 1e-3, spec.P), 0.0))
            pop.set_blob(agent, vn, np.where(free, rng.uniform(0, 1e-6, spec.P), 0.0))


def _print_gradients(case, spec, got, want, label):
    """the gradient taps against the oracle's per tensor, as a fraction of tol_g: check a's bounds follow from tol_g"""
    worst = (0.0, "", "")
    for opt in spec.opts:
        for name, off, n in C._tensors(spec, opt.ranges):
            w = want[opt.grads][off:off + n]
            if np.any(w):
                e = _rel(got[opt.grads][off:off + n], w) / spec.tol_g(name, n)
                worst = max(worst, (e, opt.name, name))
    print("%s gradients: worst tensor at %.3f of tol_g (%s %s)" % ((label,) + worst))


def _update_batch(case, pop, agent, b):
    if case.EPS:
        pop.update_batch(agent, *b[:5], eps=b[5])
    else:
        pop.update_batch(agent, *b)


@pytest.mark.parametrize("case", single_update_cases(), ids=lambda c: c.id)
def test_optimizer_state_and_target_after_one_update(hip_lib, case):
    rng = np.random.RandomState(21)
    spec = case.spec()
    pop = case.pop()
    pop.enable_grad_taps(True)
    _seed_state(case, pop, 0, case.theta0(), rng)
    for _ in range(2):
        _update_batch(case, pop, 0, case.batch(rng))
    before = case.pop_state(pop)
    o = case.oracle(before["theta"])
    C.load_oracle(o, before)
    b = case.batch(rng)
    _update_batch(case, pop, 0, b)
    taps = o.update(*b, taps=True)
    after = case.pop_state(pop)
    _print_gradients(case, spec, case.pop_grads(pop), case.grads(taps), case.id)
    pop.close()
    C.check_update(spec, before, after, oracle_after=C.oracle_state(o), grads=case.grads(taps), label=case.id)


@pytest.mark.parametrize("case,lrs", population_cases(), ids=lambda v: v.id if hasattr(v, "id") else "lr")
def test_population_offsets_reach_the_optimizer_state(hip_lib, case, lrs):
    """three agents with their own seeds, weights and learning rates updated in ONE launch from a shared replay: the
    per-agent offsets into m, v and the target under checks a to e (agent 2)"""
    NA, N, B, A = 3, 400, case.B, case.A
    rng = np.random.RandomState(33)
    pop = case.pop(n_agents=NA, lr=lrs, cap=N)
    pop.enable_grad_taps(True)
    data = case.replay(rng, N)
    for i in range(NA):
        _seed_state(case, pop, i, case.theta0(seed=40 + i), rng)
        pop.replay_add_batch(i, *data)
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(3 * NA)]).reshape(3, NA, 1, B).astype(np.int64)
    eps = rng.randn(3, NA, 1, B, A)
    kw = lambda k: dict(eps=eps[k]) if case.EPS else {}
    for k in range(2):
        pop.update(1, host_indices=idx[k], **kw(k))
    before = case.pop_state(pop, 2)
    lr = tuple(float(np.float32(l[2])) for l in lrs)
    spec = case.spec(lr=lr)
    o = case.oracle(before["theta"], lr=lr)
    C.load_oracle(o, before)
    pop.update(1, host_indices=idx[2], **kw(2))
    taps = o.update(*case.from_replay(data, idx[2, 2, 0], eps[2, 2, 0]), taps=True)
    after = case.pop_state(pop, 2)
    _print_gradients(case, spec, case.pop_grads(pop, 2), case.grads(taps), case.id)
    pop.close()
    C.check_update(spec, before, after, oracle_after=C.oracle_state(o), grads=case.grads(taps), label=case.id + " agent 2")


@pytest.mark.parametrize("case", tap_cases(), ids=lambda c: c.id)
def test_gradient_taps_do_not_change_the_state(hip_lib, case):
    """the path that is measured (taps off) and the path that is compared (taps on) leave bit-identical blobs and beta
    powers after two updates from identical state"""
    NA, N, B, A = 2, 400, case.B, case.A
    states = []
    for taps in (True, False):
        rng = np.random.RandomState(44)
        pop = case.pop(n_agents=NA, cap=N)
        pop.enable_grad_taps(taps)
        data = case.replay(rng, N)
        for i in range(NA):
            _seed_state(case, pop, i, case.theta0(seed=60 + i), rng)
            pop.replay_add_batch(i, *data)
        idx = np.stack([rng.choice(N, B, replace=False) for _ in range(2 * NA)]).reshape(NA, 2, B).astype(np.int64)
        pop.update(2, host_indices=idx, **(dict(eps=rng.randn(NA, 2, B, A)) if case.EPS else {}))
        states.append([case.pop_state(pop, i) for i in range(NA)])
        pop.close()
    for i in range(NA):
        on, off = states[0][i], states[1][i]
        assert not np.array_equal(on["theta"], case.theta0(seed=60 + i))        # the updates ran
        for k in ("theta", "theta_target", "pw"):
            assert np.array_equal(on[k], off[k]), (i, k)
        for which in ("m", "v"):
            for slot in on[which]:
                assert np.array_equal(on[which][slot], off[which][slot]), (i, which, slot)
    print("%s: %d agents, theta / theta_target / %s / beta powers bit-identical with taps on and off"
          % (case.id, NA, " / ".join(n for mv in case.SLOTS.values() for n in mv)))
