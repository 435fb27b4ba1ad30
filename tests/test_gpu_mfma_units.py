"""One parity case for every compiled MFMA update unit (tests/mfma_unit_cases.py).

Schedule of every case, that of tests/test_gpu_optimizer_state.py: set the weights, write a target that sits apart from
them, fill the Adam ranges no optimizer owns with noise, two warm-up updates on the GPU, copy the whole state into a fresh
oracle, one update on the same minibatch on both sides with the gradient taps on, then checks a to e of
tests/optimizer_state_checks.py and the forward taps of the family at 1e-5 (SoftActorCritic's logp at the 2e-4 its own
tests hold it to).  The kernel goes through Case.select_kernel: a refusal fails the test.  The test id starts with the unit
the dispatcher launches for the case.

A quantity that misses its plain bar is held by the rule of tests/test_gpu_clamp_gates.py instead -- device against the
float64 twin <= max(bar, 3 x the fp32 oracle against the twin) -- only if the case lists it in mfma_unit_cases.HELD."""
import numpy as np
import pytest

import mfma_unit_cases as U
import optimizer_state_checks as C

pytestmark = pytest.mark.gpu

CASES = U.gpu_cases()          # every case but those of mfma_unit_cases.NOT_LAUNCHED


def _update_batch(case, pop, b):
    if case.EPS:
        pop.update_batch(0, *b[:5], eps=b[5])
    else:
        pop.update_batch(0, *b)


def _tap(case, label, name, dev, ref32, twin, bar):
    """the plain bar against the fp32 oracle; for a quantity listed in HELD, the `_held` rule against the float64 twin"""
    e = U.rel(dev, ref32)
    print("%s %s: device against the oracle %.3e (bar %.0e)" % (label, name, e, bar))
    if name in U.HELD.get(U.case_id(case), ()):
        t64 = twin()[name]
        e_dev, e_ref = U.rel(dev, t64), U.rel(ref32, t64)
        bound = max(bar, U.HELD_FACTOR * e_ref)
        print("%s %s held: device %.3e, restatement %.3e, bound %.3e" % (label, name, e_dev, e_ref, bound))
        assert e_dev <= bound, (label, name, e_dev, e_ref, bound)
    else:
        assert e < bar, (label, name, e)
    return e


@pytest.mark.parametrize("case", CASES, ids=U.case_id)
def test_unit_matches_the_oracle_after_one_update(hip_lib, case):
    label = U.case_id(case)
    rng = U.schedule_rng(case)
    spec, theta = case.spec(), case.theta0()
    pop = case.pop()
    pop.enable_grad_taps(True)
    target, noise = U.seed_arrays(case, spec, theta, rng)
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", target)
    for slot, mv in noise.items():
        if mv is not None:
            pop.set_blob(0, case.SLOTS[slot][0], mv[0])
            pop.set_blob(0, case.SLOTS[slot][1], mv[1])
    for _ in range(2):
        _update_batch(case, pop, case.batch(rng))
    before = case.pop_state(pop)
    o = case.oracle(before["theta"])
    C.load_oracle(o, before)
    b = case.batch(rng)
    _update_batch(case, pop, b)
    taps = o.update(*b, taps=True)
    after = case.pop_state(pop)
    dev_taps = {k: pop.last_tap(0, k) for k in U.FORWARD_TAPS[case.NAME] if k in taps}
    dev_grads = case.pop_grads(pop)
    pop.close()

    cache = []

    def twin():
        if not cache:
            cache.append(U.twin_update(case, before, b))
        return cache[0]
    assert dev_taps, label
    for k, dev in dev_taps.items():
        _tap(case, label, k, dev, taps[k], twin, U.tap_bar(case, k))
    grads = case.grads(taps)
    worst = (0.0, "")
    for tap, name, off, n in U.owned_tensors(spec):
        w = grads[tap][off:off + n]
        assert np.any(w) and np.any(dev_grads[tap][off:off + n]), (label, tap, name)
        worst = max(worst, (U.rel(dev_grads[tap][off:off + n], w) / spec.tol_g(name, n), "%s %s" % (tap, name)))
    print("%s gradients: worst tensor at %.3f of tol_g (%s)" % ((label,) + worst))
    C.check_update(spec, before, after, oracle_after=C.oracle_state(o), grads=grads, label=label)
