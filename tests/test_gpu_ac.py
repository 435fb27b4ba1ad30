"""ActorCritic on the MI355X against its torch restatement (tests/torch_ref_ac.py): the fused update with supplied draws
over the six cases of tests/ac_cases.py, the optimizer state per element, the exact-zero actor step of case 1, the replay
paths, the device's own draws, acting / Q values, what the library refuses, and the drop-in agent.

Parity unpinned: no reference fixture exercises this agent.

How a bound is formed: every comparison is made against the restatement's float64 twin.  e_ref = the fp32 restatement's
error against the twin on the same inputs; the device's error against the twin must be <= max(project bar, 3 e_ref), and
that bound never exceeds 4 x the project bar (ac_cases.bound).  Project bars: 1e-5 for the taps and theta_target of the
first update, 5e-5 per gradient tensor, 2e-4 for the updates after it, rtol 1e-6 for the beta powers.  Every measured
error is printed.  The inputs satisfy the conditions of ac_cases.condition_failures at every update, so the cem
selection is the same on the device, the restatement and the twin: the weight tap is compared exactly there."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import ac_cases as W
import optimizer_state_checks as C
import torch_ref_ac as R
from ac_cases import ALR, CLR, TAU, _rel
from optimizer_state_cases import Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLOBS = ("theta", "theta_target", "actor_m", "actor_v", "critic_m", "critic_v")


def _pop(case, n_agents=1, lr=(ALR, CLR), cap=512, seeds=None, **kw):
    from rlcontrol_amd.hip_ac import ACPopulation
    dims, B, cu, au = case
    smin, smax, amax = W.bounds(dims[0], dims[1])
    return ACPopulation(n_agents, *dims, B, cap, TAU, smin, smax, amax, lr[0], lr[1],
                        seeds=seeds if seeds is not None else list(range(7, 7 + n_agents)), critic_update=cu,
                        actor_update=au, **kw)


def _held(label, dev, ref32, twin, bar):
    """device against the twin <= min(max(bar, 3 x the fp32 restatement against the twin), 4 bar)"""
    e_dev, e_ref = _rel(dev, twin), _rel(ref32, twin)
    bound = W.bound(e_ref, bar)
    print("%s: device %.3e, restatement %.3e, bound %.3e" % (label, e_dev, e_ref, bound))
    assert e_dev <= bound, (label, e_dev, e_ref, bound)
    return e_dev


def _check_grads(label, which, g_dev, t32, t64, bar, layout):
    gmax = float(np.max(np.abs(t64[which])))
    for n, (off, shp) in layout.items():
        sl = slice(off, off + int(np.prod(shp)))
        if not np.any(t64[which][sl]):
            # not this optimizer's tensor, the alpha head, or case 1's zero weights: exactly zero on the device
            worst = float(np.max(np.abs(g_dev[sl])))
            print("%s %s %s: largest element %.3e of max|grads| %.3e" % (label, which, n, worst, gmax))
            assert worst == 0.0, (label, which, n, worst)
            continue
        _held("%s %s %s" % (label, which, n), g_dev[sl], t32[which][sl], t64[which][sl], bar)


def _start(case, pop, theta, target):
    pop.enable_grad_taps(True)
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", target)


@pytest.mark.parametrize("case", W.CASES, ids=W.case_id)
def test_three_updates_match_the_restatement(hip_lib, case):
    it = W.steps(case, W.CASE_SEEDS[case])
    theta, target = next(it)
    pop = _pop(case)
    assert pop.P == theta.size and pop.kernel_in_use() == "generic"
    _start(case, pop, theta, target)
    label = W.case_id(case)
    for step, b, eps_next, eps, t32, t64, o32, o64 in it:
        pop.update_batch(0, *b, eps_next=eps_next, eps=eps)
        assert W.condition_failures(case, t32, t64, o32, o64, step) == [], (label, step)
        bar = W.BAR_TAP if step == 0 else W.BAR_LATER
        if case[3] == "cem":
            assert np.array_equal(pop.last_tap(0, "weights"), t32["weights"]), (label, step)      # the selected set
        for k in W.TAPS:
            _held("%s update %d tap %s" % (label, step, k), pop.last_tap(0, k), t32[k], t64[k], bar)
        for which in ("grads_c", "grads_a"):
            _check_grads("%s update %d" % (label, step), which, pop.last_tap(0, which), t32, t64,
                         W.BAR_GRAD if step == 0 else W.BAR_LATER, o32.layout)
        # theta itself is printed, not bounded here (the first Adam step amplifies near-zero gradients: tests/test_gpu_wf.py);
        # theta' is held to the Adam formula on its own m', v' per element in the optimizer-state test below
        print("%s update %d theta: device %.3e, restatement %.3e" % (
            label, step, _rel(pop.get_blob(0, "theta"), o64.theta.numpy()), _rel(o32.theta.numpy(), o64.theta.numpy())))
        _held("%s update %d theta_target" % (label, step), pop.get_blob(0, "theta_target"), o32.theta_t.numpy(),
              o64.theta_t.numpy(), bar)
    assert np.allclose(pop.get_beta_powers(0), o32.pw, rtol=1e-6, atol=0)
    pop.close()


# ---- the optimizer state per element (tests/optimizer_state_checks.py, checks a to e) ----------------------------------
class ACCase(Case):
    NAME = "ac"
    SLOTS = {"actor": ("actor_m", "actor_v"), "critic": ("critic_m", "critic_v")}
    GRADS = ("grads_c", "grads_a")

    def __init__(self, case):
        Case.__init__(self, case[0], case[1], "generic")
        self.case = case

    def theta0(self, seed=3):
        return W.theta_for_tests(self.dims, seed)

    def oracle(self, theta, dtype=torch.float32):
        return W.oracle(self.case, theta, dtype)

    def spec(self, tol_g):
        """ddpg_spec's shape: the critic's Adam first (the shared layer and the Q block), then the actor's (everything
        before the alpha head); the alpha head belongs to neither; beta powers: the actor's, then the critic's; Polyak
        over every tensor"""
        lay, P = R.layout(self.dims[:5])
        q0, al0 = lay["Wq2"][0], lay["Wal"][0]
        opts = [C.Opt("critic", "critic", [(0, lay["Wp2"][0]), (q0, P)], CLR, (2, 3), "grads_c"),
                C.Opt("actor", "actor", [(0, al0)], ALR, (0, 1), "grads_a")]
        return C.Spec(lay, P, opts, [(0, P)], TAU, "tf", lambda name, n: tol_g[name])

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        return self.select_kernel(_pop(self.case, n_agents, lr or (ALR, CLR), cap, seeds))


@pytest.mark.parametrize("case", [ACCase(W.CASES[4]), ACCase(W.CASES[1])], ids=lambda c: c.id)
def test_optimizer_state_and_target_after_one_update(hip_lib, case):
    """the schedule of tests/test_gpu_optimizer_state.py: a target apart from the weights, two warm-up updates, the whole
    state copied into a fresh restatement (and its float64 twin), one update on every side.  The gradient tolerance that
    checks a derive their m / v bounds from is the one the parity test holds each tensor to."""
    dims, B = case.dims, case.B
    rng = np.random.RandomState(W.CASE_SEEDS[case.case])
    pop = case.pop()
    theta = case.theta0()
    _start(case.case, pop, theta, W.target_apart(theta, rng))
    for _ in range(2):
        wb = W.batch(rng, dims, B)
        wn, we = W.draws(rng, case.case)
        pop.update_batch(0, *wb, eps_next=wn, eps=we)
    before = case.pop_state(pop)
    o, o64 = case.oracle(before["theta"]), case.oracle(before["theta"], dtype=torch.float64)
    C.load_oracle(o, before)
    C.load_oracle(o64, before)
    b = W.batch(rng, dims, B)
    eps_next, eps = W.draws(rng, case.case)
    pop.update_batch(0, *b, eps_next=eps_next, eps=eps)
    taps, taps64 = o.update(*b, eps_next, eps, taps=True), o64.update(*b, eps_next, eps, taps=True)
    assert W.condition_failures(case.case, taps, taps64, o, o64, 2) == [], case.id
    after = case.pop_state(pop)
    grads = case.pop_grads(pop)
    tol_g = {}
    for name, (off, shp) in o.layout.items():
        sl = slice(off, off + int(np.prod(shp)))
        tol_g[name] = max([W.BAR_GRAD] + [W.bound(_rel(taps[w][sl], taps64[w][sl]), W.BAR_GRAD) for w in case.GRADS
                                          if np.any(taps64[w][sl])])
        print("%s gradient tolerance %s: %.3e" % (case.id, name, tol_g[name]))
    pop.close()
    C.check_update(case.spec(tol_g), before, after, oracle_after=C.oracle_state(o), grads=case.grads(taps), label=case.id)
    lay = o.layout                                                                   # the alpha head: Polyak only
    for name in R.ALPHA_HEAD:
        sl = slice(lay[name][0], lay[name][0] + int(np.prod(lay[name][1])))
        assert np.array_equal(after["theta"][sl], before["theta"][sl]), name
        for slot in ("actor", "critic"):
            assert not np.any(after["m"][slot][sl]) and not np.any(after["v"][slot][sl]), (name, slot)
        assert not np.any(grads["grads_a"][sl]) and not np.any(grads["grads_c"][sl]), name


# ---- case 1: w_0 = q_0 - q_0 = 0 ---------------------------------------------------------------------------------------
def test_one_sample_ll_gives_an_exactly_zero_actor_step(hip_lib):
    """n = 1 with actor_update ll: the baseline is the sample's own Q, so the weight is exactly 0.  The actor's gradient
    blob is exactly zero, the actor-only tensors and the actor's moments keep their bits, the critic step still matches"""
    case = W.CASES[0]
    it = W.steps(case, W.CASE_SEEDS[case], 1)
    theta, target = next(it)
    pop = _pop(case)
    _start(case, pop, theta, target)
    step, b, eps_next, eps, t32, t64, o32, o64 = next(it)
    assert eps_next is None
    pop.update_batch(0, *b, eps=eps)
    after = {k: pop.get_blob(0, k) for k in BLOBS}
    assert not np.any(pop.last_tap(0, "weights")) and not np.any(pop.last_tap(0, "grads_a"))
    assert not np.any(t64["weights"]) and not np.any(t64["grads_a"])
    lay = o32.layout
    for name, (off, shp) in lay.items():
        sl = slice(off, off + int(np.prod(shp)))
        if name in R.ACTOR_ONLY + R.ALPHA_HEAD:
            assert np.array_equal(after["theta"][sl].view(np.uint32), theta[sl].view(np.uint32)), name
        assert not np.any(after["actor_m"][sl]) and not np.any(after["actor_v"][sl]), name
    for k in ("q", "y", "a_next", "raw_samples", "samples", "sample_q"):
        _held("case 1 tap %s" % k, pop.last_tap(0, k), t32[k], t64[k], W.BAR_TAP)
    _check_grads("case 1", "grads_c", pop.last_tap(0, "grads_c"), t32, t64, W.BAR_GRAD, lay)
    assert not np.array_equal(after["theta"][:lay["Wp2"][0]], theta[:lay["Wp2"][0]])      # the critic moved W1, b1
    pop.close()


# ---- replay paths, K updates in one launch ------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [W.CASES[1], W.CASES[2]], ids=W.case_id)
def test_replay_paths_and_k_updates_in_one_launch(hip_lib, case):
    dims, B, cu, au = case
    NA, N, K = 2, 256, 3
    rng = np.random.RandomState(5)
    S, A, n = dims[0], dims[1], dims[5]
    nd = R.next_draws(cu, n)
    amax = W.bounds(S, A)[2]
    data = (rng.uniform(-1, 1, (N, S)), rng.uniform(-1, 1, (N, A)) * amax, rng.uniform(-16, 0, N), rng.uniform(-1, 1, (N, S)),
            np.where(rng.rand(N) < 0.2, 0.0, 0.99))
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(NA * K)]).reshape(NA, K, B).astype(np.int64)
    en = rng.standard_normal((NA, K, B, nd, A)).astype(np.float32)
    eps = rng.standard_normal((NA, K, B, n, A)).astype(np.float32)
    thetas = [W.theta_for_tests(dims, 30 + i) for i in range(NA)]

    def fresh(seeds=None):
        pop = _pop(case, n_agents=NA, cap=N, seeds=seeds)
        for i in range(NA):
            pop.set_params(i, thetas[i], init_target=True)
            pop.replay_add_batch(i, *data)
        return pop

    one = fresh()
    one.update(K, host_indices=idx, eps_next=en, eps=eps)      # K updates in one launch
    many = fresh()
    for k in range(K):                                         # K launches of one update
        many.update(1, host_indices=idx[:, k:k + 1], eps_next=en[:, k:k + 1], eps=eps[:, k:k + 1])
    staged = fresh()                                           # update_batch on the gathered rows, agent by agent
    s, a, r, s2, g = data
    for k in range(K):
        for i in range(NA):
            j = idx[i, k]
            staged.update_batch(i, s[j], a[j], s2[j], r[j], g[j], eps_next=en[i, k], eps=eps[i, k])
    for i in range(NA):
        for blob in BLOBS:
            assert np.array_equal(one.get_blob(i, blob), many.get_blob(i, blob)), (i, blob)
            assert np.array_equal(one.get_blob(i, blob), staged.get_blob(i, blob)), (i, blob)
        assert np.array_equal(one.get_beta_powers(i), many.get_beta_powers(i))
        assert np.array_equal(one.get_beta_powers(i), staged.get_beta_powers(i))
        for tap in ("q", "y", "a_next", "raw_samples", "samples", "sample_q", "weights"):
            assert np.array_equal(one.last_tap(i, tap), many.last_tap(i, tap)), (i, tap)
        assert not np.array_equal(one.get_blob(i, "theta"), thetas[i])
    many.close(); staged.close(); one.close()
    # the device sampler with the device's draws: K in one launch = K launches, bit for bit; agents with different keys differ
    runs = []
    for split in (False, True):
        pop = fresh(seeds=[21, 22])
        if split:
            for _ in range(K):
                pop.update(1)
        else:
            pop.update(K)
        runs.append([{b: pop.get_blob(i, b) for b in BLOBS} for i in range(NA)])
        pop.close()
    for i in range(NA):
        for blob in BLOBS:
            assert np.array_equal(runs[0][i][blob], runs[1][i][blob]), (i, blob)
    same = fresh(seeds=[21, 21])
    for i in range(NA):
        same.set_params(i, thetas[0], init_target=True)
    same.update(K)
    other = fresh(seeds=[21, 22])
    for i in range(NA):
        other.set_params(i, thetas[0], init_target=True)
    other.update(K)
    assert np.array_equal(same.get_blob(0, "theta"), same.get_blob(1, "theta"))
    assert not np.array_equal(other.get_blob(0, "theta"), other.get_blob(1, "theta"))
    same.close(); other.close()


@pytest.mark.parametrize("case", [W.CASES[3], W.CASES[1]], ids=W.case_id)
def test_device_draws_are_seeded_and_inside_the_action_range(hip_lib, case):
    dims, B, cu, au = case
    N = 64
    rng = np.random.RandomState(6)
    S, A, n = dims[0], dims[1], dims[5]
    amax = W.bounds(S, A)[2].astype(np.float32)
    data = (rng.uniform(-1, 1, (N, S)), rng.uniform(-1, 1, (N, A)) * amax, rng.uniform(-16, 0, N), rng.uniform(-1, 1, (N, S)),
            np.where(rng.rand(N) < 0.2, 0.0, 0.99))
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(2)]).reshape(1, 2, B).astype(np.int64)
    theta = W.theta_for_tests(dims, 8)

    def run(seed):
        pop = _pop(case, cap=N, seeds=[seed])
        pop.set_params(0, theta, init_target=True)
        pop.replay_add_batch(0, *data)
        pop.update(2, host_indices=idx)                         # eps_next, eps null: the device's Philox stream
        out = {k: pop.get_blob(0, k) for k in BLOBS}
        out["samples"] = pop.last_tap(0, "samples").reshape(B, n, A)
        out["a_next"] = pop.last_tap(0, "a_next").reshape(B, -1, A)
        out["raw"] = pop.last_tap(0, "raw_samples").reshape(B * n, A)
        out["act"] = np.stack([pop.act(data[0][:1], sample=True)[0] for _ in range(4)])
        pop.close()
        return out

    first, again, other = run(11), run(11), run(12)
    for k in first:
        assert np.array_equal(first[k], again[k]), k
    assert not np.array_equal(first["samples"], other["samples"]) and not np.array_equal(first["theta"], other["theta"])
    assert not np.array_equal(first["act"], other["act"]) and not np.array_equal(first["a_next"], other["a_next"])
    assert len(np.unique(first["act"], axis=0)) == 4            # the acting stream advances
    for out in (first, other):
        for x in (out["samples"], out["a_next"], out["act"]):
            assert np.all(np.isfinite(x)) and np.all(np.abs(x) <= amax)
        assert len(np.unique(out["raw"], axis=0)) == B * n       # every draw its own
        assert not np.array_equal(out["a_next"][:, 0], out["samples"][:, 0])          # the two streams are apart


# ---- acting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [W.CASES[4], W.CASES[2], W.CASES[3], W.CASES[0]], ids=W.case_id)
def test_act_and_qval_match_the_restatement(hip_lib, case):
    """one state per agent of a six-agent population, every agent with weights of its own"""
    dims = case[0]
    NA, S, A = 6, dims[0], dims[1]
    amax = W.bounds(S, A)[2]
    rng = np.random.RandomState(9)
    pop = _pop((dims, 32) + case[2:], n_agents=NA, cap=64)
    o32, o64 = [], []
    for i in range(NA):
        th = W.theta_for_tests(dims, 50 + i)
        pop.set_params(i, th, init_target=True)
        o32.append(W.oracle(case, th))
        o64.append(W.oracle(case, th, torch.float64))
    states = rng.uniform(-1, 1, (NA, S))
    eps = rng.standard_normal((NA, A)).astype(np.float32)
    greedy = pop.act(states)
    drawn = pop.act(states, sample=True, eps=eps)
    assert greedy.shape == (NA, A) and drawn.shape == (NA, A)
    for i in range(NA):
        for name, got, ref in (("greedy", greedy[i], o32[i].act(states[i:i + 1])[0]),
                               ("sampled", drawn[i], o32[i].sample(states[i:i + 1], eps[i:i + 1])[0])):
            e = float(np.max(np.abs(np.asarray(got, np.float64) - ref) / amax))
            print("act %s agent %d %s: %.3e" % (W.case_id(dims), i, name, e))
            assert e < 1e-5, (i, name, e)
    assert np.all(np.abs(drawn) <= amax.astype(np.float32)) and not np.array_equal(drawn, greedy)
    # queued: all six (stream wait), a sub-range, and one agent (the completion word); greedy and sampled
    for first, n in ((0, NA), (3, 2), (5, 1)):
        sl = slice(first, first + n)
        assert pop.act_queue(states[sl], first_agent=first) == n
        assert np.array_equal(pop.act_fetch(n, first_agent=first), greedy[sl]), (first, n)
        assert pop.act_queue(states[sl], first_agent=first, sample=True, eps=eps[sl]) == n
        assert np.array_equal(pop.act_fetch(n, first_agent=first), drawn[sl]), (first, n)
    actions = rng.uniform(-1, 1, (NA, A)) * amax
    for i in (0, NA - 1):
        rows = rng.uniform(-1, 1, (NA, S))
        _held("qval %s agent %d" % (W.case_id(dims), i), pop.qval(i, rows, actions), o32[i].qval(rows, actions),
              o64[i].qval(rows, actions), 1e-5)
    pop.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_name(hip_lib):
    from rlcontrol_amd._lib import RlcError
    base = ((3, 1, 32, 32, 32, 30, 6), 16, "sampled", "ll")

    def with_dims(**kw):
        names = ("S", "A", "L1", "La", "Lc", "n", "k")
        d = dict(zip(names, base[0]), **kw)
        return (tuple(d[k] for k in names),) + base[1:]
    with pytest.raises(RlcError, match="layer"):
        _pop(base, norm_type="layer")
    with pytest.raises(RlcError, match="batch"):
        _pop(base, norm_type="batch")
    with pytest.raises(RlcError, match=r"action_dim <= 6 \(got 7\)"):
        _pop(with_dims(A=7))
    with pytest.raises(RlcError, match=r"num_samples <= 1024 \(got 1025\)"):
        _pop(with_dims(n=1025))
    with pytest.raises(RlcError, match=r"top_k = int\(num_samples \* rho\) must be in \[1, num_samples\] for actor_update cem \(got 0 of 30\)"):
        _pop(with_dims(k=0)[:2] + ("sampled", "cem"))
    _pop(with_dims(k=0)).close()                                                     # top_k is read for cem only
    with pytest.raises(RlcError, match=r"need \d+ B of LDS \(> 65536\)"):
        _pop(with_dims(L1=9000, La=9000, Lc=20000))
    with pytest.raises(ValueError, match="critic_update 'random_q'"):
        _pop(base[:2] + ("random_q", "ll"))
    with pytest.raises(ValueError, match="actor_update 'reparam'"):
        _pop(base[:2] + ("sampled", "reparam"))
    _pop(((3, 6, 32, 32, 32, 1024, 1024), 4, "expected", "cem")).close()             # exactly at the limits
    pop = _pop(base)
    with pytest.raises(RlcError, match="any-shape kernel only"):
        pop.set_kernel("mfma")
    with pytest.raises(RlcError, match="no latency mode"):
        pop.set_split(2)
    with pytest.raises(ValueError, match="eps_next must be given"):
        pop.update_batch(0, np.zeros((16, 3)), np.zeros((16, 1)), np.zeros((16, 3)), np.zeros(16), np.zeros(16),
                         eps=np.zeros((16, 30, 1), np.float32))
    pop.set_kernel("generic"); pop.set_kernel("auto"); pop.set_split(1)
    assert pop.kernel_in_use() == "generic"
    pop.close()


# ---- the drop-in agent -------------------------------------------------------------------------------------------------
def _config(seed, **over):
    from rlcontrol_amd.environments.environments import create_environment
    from rlcontrol_amd.utils.config import Config
    env = create_environment({"environment": "Pendulum-v0", "TotalMilSteps": 0.001, "EpisodeSteps": -1,
                              "EvalIntervalMilSteps": 0.0005, "EvalEpisodes": 2})
    cfg = Config()
    cfg.merge_config({"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min,
                      "state_max": env.state_max, "action_dim": env.action_dim, "action_min": env.action_min,
                      "action_max": env.action_max})
    cfg.merge_config(dict({"critic_update": "sampled", "actor_update": "ll", "norm_type": "input_norm",
                           "exploration_policy": "none", "shared_l1_dim": 200, "actor_l2_dim": 200, "critic_l2_dim": 200,
                           "actor_lr": 0.001, "critic_lr": 0.01, "rho": 0.2, "num_samples": 30, "num_modal": 1,
                           "sample_for_eval": "False", "equal_modal_selection": "False", "batch_size": 32,
                           "buffer_size": 5000, "writer": None, "replay_sampler": "reference"}, **over))
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": seed})
    return cfg, env


@pytest.mark.parametrize("policy", ["none", "ou_noise"])
def test_dropin_agent_follows_a_population_fed_the_same_minibatches_and_draws(hip_lib, policy):
    """60 seeded random transitions through agent.update / agent.step: the agent's blobs equal, bit for bit, those of an
    ACPopulation given the same transitions, minibatch indices and draws -- the draws of a RandomState(seed) consumed in
    the agent's documented order (per update eps_next then eps, per sampled action [1][1][A]).  exploration_policy none:
    every training action is that population's sample for the same draw; ou_noise: the population's greedy action plus
    the host's OU noise, and no acting draw is consumed."""
    from rlcontrol_amd.hip_ac import ACPopulation
    from rlcontrol_amd.utils.exploration_policy import make_policy
    from rlcontrol_amd.utils.main_utils import create_agent
    seed, batch, steps = 2, 32, 60
    cfg, env = _config(seed, batch_size=batch, exploration_policy=policy)
    agent = create_agent("ActorCritic", cfg)
    mgr = agent.network_manager
    pop = mgr.population
    dims = (env.state_dim, env.action_dim, 200, 200, 200)
    A, n = env.action_dim, 30
    sampled = policy == "none"
    assert pop.P == 82204 and pop.dims == dims and (pop.n, pop.k) == (30, 6)
    assert mgr.use_external_exploration == (not sampled)
    theta0 = pop.get_blob(0, "theta")
    assert np.array_equal(pop.get_blob(0, "theta_target"), theta0)
    twin_pop = ACPopulation(1, *dims, 30, 6, batch, int(cfg.buffer_size), cfg.tau, env.state_min, env.state_max,
                            env.action_max, cfg.actor_lr, cfg.critic_lr, seeds=[np.uint64(seed)])
    twin_pop.set_params(0, theta0, init_target=True)
    drawn = []
    inner = mgr.update_from_replay

    def recording(indices, next_state=None):
        drawn.append(np.array(indices, np.int64))
        return inner(indices, next_state=next_state)
    mgr.update_from_replay = recording
    shadow = np.random.RandomState(seed)                       # the agent's stream, consumed in the same order
    noise = None if sampled else make_policy(cfg, mgr.random_seed, mgr.action_dim, mgr.action_min, mgr.action_max)[1]
    train_steps = [0]

    def expected_action(state):
        if sampled:
            e1 = shadow.standard_normal((1, 1, A)).astype(np.float32)
            return twin_pop.act(state.reshape(1, -1), sample=True, eps=e1)[0]
        train_steps[0] += 1
        return noise.generate(twin_pop.act(state.reshape(1, -1))[0], train_steps[0])

    amax = np.asarray(env.action_max, np.float64).reshape(-1)
    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(env.state_min, np.float64), np.asarray(env.state_max, np.float64)
    obs = rng.uniform(lo, hi)
    agent.reset()
    if noise is not None:
        noise.reset()
    want = expected_action(obs)
    a = agent.start(obs, True)
    assert np.array_equal(a, want)
    fetched = updates = 0
    for t in range(steps):
        obs_n, r = rng.uniform(lo, hi), float(rng.uniform(-16, 0))
        done = bool(rng.rand() < 0.02)
        agent.update(obs, obs_n, r, a, done, False)
        twin_pop.replay_add(0, obs, a, r, obs_n, 0.0 if done else cfg.gamma)
        if len(drawn) > updates:
            en = shadow.standard_normal((batch, 1, A)).astype(np.float32)
            ee = shadow.standard_normal((batch, n, A)).astype(np.float32)
            twin_pop.update(1, host_indices=drawn[-1], eps_next=en, eps=ee)
            updates = len(drawn)
        fetched += mgr._queued_state is not None
        want = expected_action(obs_n)
        a = agent.step(obs_n, True)
        assert np.array_equal(a, want), t
        if sampled:
            assert np.all(np.abs(a) <= amax)
        obs = obs_n
    assert updates == steps - batch and fetched > 0.9 * updates
    for blob in BLOBS:
        assert np.array_equal(pop.get_blob(0, blob), twin_pop.get_blob(0, blob)), blob
    assert np.array_equal(pop.get_beta_powers(0), twin_pop.get_beta_powers(0))
    assert not np.array_equal(pop.get_blob(0, "theta"), theta0)
    # evaluation: the greedy action, no draw consumed
    state = shadow.get_state()[1].copy()
    assert np.array_equal(agent.step(obs, False), twin_pop.act(obs.reshape(1, -1))[0])
    assert np.array_equal(mgr.rng.get_state()[1], state)
    twin_pop.close()


RUN_KEYS = {"random_seed", "total_timesteps", "eval_interval_timesteps", "episodes_per_eval", "eval_episode_rewards",
            "eval_episode_steps", "timesteps_at_eval", "train_episode_steps", "train_episode_rewards",
            "total_train_episodes", "eval_time", "train_time"}


def test_main_host_loop_writes_the_result_pickle(hip_lib, tmp_path):
    """main.py with the shipped ac.json on Bimodal1DEnv: settings 0 to 2 (sampled actions, OU noise, the next actor_lr),
    60 training steps each"""
    import pickle
    import main as drv
    ej = tmp_path / "Bimodal1DEnv.json"
    with open(os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json")) as f:
        env_json = json.load(f)
    env_json.update({"TotalMilSteps": 0.00006, "EvalIntervalMilSteps": 0.00004, "EvalEpisodes": 1})
    ej.write_text(json.dumps(env_json))
    drv.main(["--env_json", str(ej), "--agent_json", os.path.join(ROOT, "jsonfiles", "agent", "ac.json"),
              "--indices", "0", "1", "3", "--save_dir", str(tmp_path), "--quiet"])
    files = glob.glob(str(tmp_path / "*results" / "data_*.pkl"))
    assert len(files) == 1, os.listdir(str(tmp_path))
    with open(files[0], "rb") as f:
        data = pickle.load(f)
    assert data["experiment"]["agent"]["agent_name"] == "ActorCritic"
    runs = [r for d in data["experiment_data"].values() for r in d["runs"]]
    assert len(runs) == 3 and all(set(r) == RUN_KEYS for r in runs)
    for run in runs:
        assert run["total_timesteps"] == 60
        assert np.isfinite(run["eval_episode_rewards"]).all() and np.isfinite(run["train_episode_rewards"]).all()
