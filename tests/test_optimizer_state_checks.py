"""CPU tests of tests/optimizer_state_checks.py: the oracles themselves pass checks b to d on every case the GPU file
runs (this is where the two unit bounds are measured), and a damaged after-state is rejected by the check named for the
damage -- the proof that tests/test_gpu_optimizer_state.py would fail on a subtly wrong kernel."""
import numpy as np
import pytest

import optimizer_state_checks as C
from optimizer_state_cases import DDPGCase, single_update_cases


def _unique(cases):
    seen, out = set(), []
    for c in cases:                                   # the oracle does not know about kernels
        key = (c.NAME, c.dims, c.B, tuple(sorted(c.kw.items())))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


ORACLE_CASES = _unique(single_update_cases())


def run_oracle(case, seed=0, noise_unowned=False):
    """the schedule of the GPU file on the oracle alone: target apart, two warm-up updates, one compared update"""
    rng = np.random.RandomState(seed + 21)
    th = case.theta0()
    o = case.oracle(th)
    st = C.oracle_state(o)
    st["theta_target"] = case.target_apart(th, rng)
    if noise_unowned:                                 # something to lose in the ranges an optimizer does not own
        for slot in st["m"]:
            st["m"][slot] = rng.uniform(-1e-3, 1e-3, th.size).astype(np.float32)
            st["v"][slot] = rng.uniform(0, 1e-6, th.size).astype(np.float32)
    C.load_oracle(o, st)
    for _ in range(2):
        o.update(*case.batch(rng))
    before = C.oracle_state(o)
    taps = o.update(*case.batch(rng), taps=True)
    return before, C.oracle_state(o), case.grads(taps)


@pytest.mark.parametrize("case", ORACLE_CASES, ids=lambda c: c.id)
def test_oracle_passes_its_own_adam_and_polyak_checks(case):
    """checks b, c, d on the oracle's own states (a and e are trivially exact here).  The C oracles are held to the counts
    the module's bounds were derived from (the GPU bounds are 4 x and 2 x these); the torch oracles, whose gradient sums
    may round differently from one CPU to the next, to the bounds the kernels are held to."""
    before, after, _ = run_oracle(case)
    spec = case.spec()
    in_c = case.NAME == "ddpg" or (case.NAME in ("sac", "naf") and not case.kw.get("norm"))
    adam_bound, polyak_bound = (C.ORACLE_ADAM_UNITS, C.ORACLE_POLYAK_UNITS) if in_c else (C.ADAM_UNITS, C.POLYAK_UNITS)
    out = C.check_update(spec, before, after, label=case.id, adam_bound=adam_bound, polyak_bound=polyak_bound)
    forms = C.polyak_forms_units(spec, before, after)
    print("%s Polyak, the larger of the two float32 forms: %.2f units" % (case.id, forms))
    assert forms <= polyak_bound
    assert out["adam_units"] > 0 and forms > 0        # the update moved something: the counts are not vacuous


def test_unit_bounds_are_the_stated_multiples_of_the_oracle_measurements():
    assert C.ADAM_UNITS == 4 * C.ORACLE_ADAM_UNITS and C.POLYAK_UNITS == 2 * C.ORACLE_POLYAK_UNITS


# ------------------------------------------------------------------------------------------ mutations
MUT = DDPGCase((8, 2, 64, 48, 40), 17, "generic")     # critic width 40: the last 16-column tile is partly filled


@pytest.fixture(scope="module")
def mut():
    before, after, grads = run_oracle(MUT, noise_unowned=True)
    return MUT.spec(), before, after, grads


def _f32_adam_theta(spec, before, after, pw=None, lr_of=None, eps_inside=False):
    """the oracle's float32 arithmetic restated in numpy (oracle/ddpg_oracle.c adam_range), with room for mistakes"""
    f = np.float32
    pw = np.asarray(before["pw"] if pw is None else pw, np.float32)
    th = before["theta"].copy()
    for opt in spec.opts:
        lr = f((lr_of or {}).get(opt.name, opt.lr))
        alpha = lr * np.sqrt(f(1) - pw[opt.pw[1]]) / (f(1) - pw[opt.pw[0]])
        m, v = after["m"][opt.slot], after["v"][opt.slot]
        den = np.sqrt(v + f(1e-8)) if eps_inside else np.sqrt(v) + f(1e-8)
        k = C._mask(spec.P, opt.ranges)
        th[k] = (th - (m * alpha) / den)[k]
    return th


def _f32_polyak(tt, th, tau):
    return (tt + np.float32(tau) * (th - tt)).astype(np.float32)


def _copy(st):
    return {k: ({s: a.copy() for s, a in v.items()} if isinstance(v, dict) else v.copy()) for k, v in st.items()}


def _rejected(spec, before, bad, after, grads):
    with pytest.raises(C.CheckFailed) as e:
        C.check_update(spec, before, bad, oracle_after=after, grads=grads, quiet=True)
    return e.value.checks


def test_the_undamaged_state_passes_every_check(mut):
    spec, before, after, grads = mut
    C.check_update(spec, before, after, oracle_after=after, grads=grads, label="undamaged")
    # and the numpy restatement the mutations below are built from reproduces the oracle
    redo = _copy(after)
    redo["theta"] = _f32_adam_theta(spec, before, after)
    redo["theta_target"] = _f32_polyak(before["theta_target"], redo["theta"], spec.tau)
    C.check_update(spec, before, redo, oracle_after=after, grads=grads, label="restated")


def test_tau_times_1_3_fails_check_c(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    bad["theta_target"] = _f32_polyak(before["theta_target"], after["theta"], 1.3 * spec.tau)
    assert _rejected(spec, before, bad, after, grads) == ["c"]


def test_polyak_from_the_weights_before_the_step_fails_check_c(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    bad["theta_target"] = _f32_polyak(before["theta_target"], before["theta"], spec.tau)
    assert _rejected(spec, before, bad, after, grads) == ["c"]


def test_polyak_skipped_on_the_actor_tensors_fails_check_c(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    lo, hi = spec.layout["Wa2"][0], spec.layout["Wc2"][0]
    bad["theta_target"][lo:hi] = before["theta_target"][lo:hi]
    assert _rejected(spec, before, bad, after, grads) == ["c"]


def _block(spec, name, rows, cols):
    off, (nr, nc) = spec.layout[name]
    return (off + np.arange(nr * nc).reshape(nr, nc)[rows, cols]).ravel()


def test_a_16x16_block_of_v_left_at_its_old_value_fails_check_a(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    i = _block(spec, "Wa2", slice(16, 32), slice(16, 32))
    bad["v"]["actor"][i] = before["v"]["actor"][i]
    assert "a" in _rejected(spec, before, bad, after, grads)


def test_a_column_strip_of_m_in_the_partly_filled_last_tile_left_at_its_old_value_fails_check_a(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    i = _block(spec, "Wc2", slice(0, 16), slice(32, 40))       # columns 32..47 of a 40-wide matrix: 8 exist
    bad["m"]["critic"][i] = before["m"]["critic"][i]
    assert "a" in _rejected(spec, before, bad, after, grads)


def test_m_with_beta1_0_99_fails_check_a(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    k = C._mask(spec.P, spec.opts[1].ranges)
    m, g = before["m"]["actor"], grads["grads_a"]
    bad["m"]["actor"][k] = (m + (g - m) * np.float32(1 - 0.99))[k]
    # theta and the target follow from the wrong m consistently: only the comparison with the oracle can see it
    bad["theta"] = _f32_adam_theta(spec, before, bad)
    bad["theta_target"] = _f32_polyak(before["theta_target"], bad["theta"], spec.tau)
    assert _rejected(spec, before, bad, after, grads) == ["a"]


def _with_theta(spec, before, after, theta):
    bad = _copy(after)
    bad["theta"] = theta
    bad["theta_target"] = _f32_polyak(before["theta_target"], theta, spec.tau)      # a consistent average of the wrong weights
    return bad


def test_the_step_with_the_beta_powers_of_the_next_step_fails_check_b(mut):
    spec, before, after, grads = mut
    pw = before["pw"] * np.array([0.9, 0.999, 0.9, 0.999], np.float32)
    bad = _with_theta(spec, before, after, _f32_adam_theta(spec, before, after, pw=pw))
    assert _rejected(spec, before, bad, after, grads) == ["b"]


def test_epsilon_inside_the_square_root_fails_check_b(mut):
    spec, before, after, grads = mut
    bad = _with_theta(spec, before, after, _f32_adam_theta(spec, before, after, eps_inside=True))
    assert _rejected(spec, before, bad, after, grads) == ["b"]


def test_the_critic_learning_rate_on_the_actor_range_fails_check_b(mut):
    spec, before, after, grads = mut
    bad = _with_theta(spec, before, after, _f32_adam_theta(spec, before, after, lr_of={"actor": spec.opts[0].lr}))
    assert _rejected(spec, before, bad, after, grads) == ["b"]


def test_an_unowned_m_range_decayed_by_beta1_fails_check_d(mut):
    spec, before, after, grads = mut
    bad = _copy(after)
    lo, hi = spec.layout["Wa2"][0], spec.layout["Wc2"][0]      # the actor branch in the critic's optimizer
    assert np.any(before["m"]["critic"][lo:hi])
    bad["m"]["critic"][lo:hi] *= np.float32(0.9)
    assert _rejected(spec, before, bad, after, grads) == ["d"]


def test_a_moved_target_where_the_average_does_not_reach_fails_check_d():
    """the KL agents average the V block only"""
    case = [c for c in ORACLE_CASES if c.NAME == "kl"][0]
    before, after, grads = run_oracle(case)
    spec = case.spec()
    C.check_update(spec, before, after, oracle_after=after, grads=grads, label=case.id)
    bad = _copy(after)
    lo = spec.layout["qW1"][0]
    bad["theta_target"][lo:lo + 16] = _f32_polyak(before["theta_target"], after["theta"], spec.tau)[lo:lo + 16]
    assert _rejected(spec, before, bad, after, grads) == ["d"]
