"""WireFitting on the MI355X against its torch restatement (tests/torch_ref_wf.py): the fused update, the optimizer state
per element, the replay paths, acting / Q values, what the library refuses, and the drop-in agent.

Parity unpinned: no reference fixture exercises this agent.

How a bound is formed.  1 / distance is ill-conditioned (the 1e-5 floor makes w as large as 1e5), so the project's usual
bars sit inside fp32 noise for some tensors.  Every comparison is therefore made against the restatement's float64 twin:
e_ref = the fp32 restatement's error against the twin on the same inputs, and the device's error against the twin must be
<= max(project bar, 3 e_ref) -- device and restatement are two fp32 evaluations of the same expression in different
summation orders, and the device adds its own dense-layer order on top.  Project bars: 1e-5 for the taps and
theta_target of the first update, 2e-4 for the updates after it, 5e-5 per gradient tensor, rtol 1e-6 for the beta powers.
Every measured error is printed."""
import glob
import json
import os

import numpy as np
import pytest
import torch

import optimizer_state_checks as C
import torch_ref_wf as R
import wf_cases as W
from optimizer_state_cases import Case
from wf_cases import AMAX0, LR, TAU

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _pop(dims, B, n_agents=1, lr=LR, cap=512, seeds=None, **kw):
    from rlcontrol_amd.hip_wf import WFPopulation
    smin, smax = W.bounds(dims[0])
    return WFPopulation(n_agents, *dims, B, cap, TAU, smin, smax, AMAX0, lr,
                        seeds=seeds if seeds is not None else list(range(7, 7 + n_agents)), **kw)


def _held(label, dev, ref32, twin, bar):
    """device against the twin <= max(bar, 3 x the fp32 restatement against the twin)"""
    e_dev, e_ref = _rel(dev, twin), _rel(ref32, twin)
    bound = max(bar, 3.0 * e_ref)
    print("%s: device %.3e, restatement %.3e, bound %.3e" % (label, e_dev, e_ref, bound))
    assert e_dev <= bound, (label, e_dev, e_ref, bound)
    return e_dev


def _check_grads(label, dims, g_dev, t32, t64, bar, layout):
    gmax = float(np.max(np.abs(t64["grads"])))
    for n, (off, shp) in layout.items():
        sl = slice(off, off + int(np.prod(shp)))
        if dims[4] == 1 and n in ("Wa", "ba", "kappa"):
            # one wire: Q = qhat_0 whatever the action, these gradients are zero -- no relative error to take
            worst = float(np.max(np.abs(g_dev[sl])))
            print("%s gradient %s: largest element %.3e of max|grads| %.3e" % (label, n, worst, gmax))
            assert worst <= 1e-6 * gmax, (label, n, worst)
            continue
        _held("%s gradient %s" % (label, n), g_dev[sl], t32["grads"][sl], t64["grads"][sl], bar)


UPDATE_CASES = [(d, B, False) for d, B in W.SHAPES] + [((3, 1, 32, 24, 7), 17, True), ((3, 1, 200, 200, 100), 32, True)]


@pytest.mark.parametrize("dims,B,hit", UPDATE_CASES, ids=lambda v: W.shape_id(v) if not isinstance(v, bool) else ("on_a_wire" if v else "generic"))
def test_three_updates_match_the_restatement(hip_lib, dims, B, hit):
    # seed 23: the first for which the tie-free condition holds in every case and update (with 100 wires and 100 rows two
    # wire values within 1e-4 of each other are common: seeds 17 to 22 each have such a row in some case); searched on the
    # restatement alone
    rng = np.random.RandomState(23)
    theta = R.init_params(dims, 3)
    target = W.target_apart(theta, rng)
    pop = _pop(dims, B)
    assert pop.P == theta.size and pop.kernel_in_use() == "generic"
    pop.enable_grad_taps(True)
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", target)
    o32, o64 = W.oracle(dims, theta), W.oracle(dims, theta, torch.float64)
    for o in (o32, o64):
        o.theta_t = o.theta_t * 0 + torch.as_tensor(target).to(o.dt)
    label = W.shape_id(dims) + "/B%d%s" % (B, "/on a wire" if hit else "")
    for step in range(3):
        b = W.batch(rng, dims, B)
        if hit:
            b = W.on_a_wire(o32, b)
        W.assert_tie_free(o32, b, label)
        pop.update_batch(0, *b)
        t32, t64 = o32.update(*b, taps=True), o64.update(*b, taps=True)
        bar = 1e-5 if step == 0 else 2e-4
        for k in ("q", "y", "max_q"):
            _held("%s update %d tap %s" % (label, step, k), pop.last_tap(0, k), t32[k], t64[k], bar)
        _check_grads("%s update %d" % (label, step), dims, pop.last_tap(0, "grads"), t32, t64, 5e-5 if step == 0 else 2e-4,
                     o32.layout)
        # theta itself is printed, not bounded here: the first Adam step is lr g / (|g| + 3.2e-7), so elements with a
        # gradient near zero move by up to lr for a gradient error of 3e-7 -- no bound on theta follows from the gradient
        # bars.  theta' is held to the Adam formula on its own m', v' per element in the optimizer-state test below.
        print("%s update %d theta: device %.3e, restatement %.3e" % (
            label, step, _rel(pop.get_blob(0, "theta"), o64.theta.numpy()), _rel(o32.theta.numpy(), o64.theta.numpy())))
        _held("%s update %d theta_target" % (label, step), pop.get_blob(0, "theta_target"), o32.theta_t.numpy(),
              o64.theta_t.numpy(), bar)
    assert np.allclose(pop.get_beta_powers(0), o32.pw, rtol=1e-6, atol=0)
    pop.close()


# ---- the optimizer state per element (tests/optimizer_state_checks.py, checks a to e) ----------------------------------
class WFCase(Case):
    NAME = "wf"

    def __init__(self, dims, B):
        Case.__init__(self, dims, B, "generic")

    def batch(self, rng):
        return W.batch(rng, self.dims, self.B)

    def theta0(self, seed=2):
        return R.init_params(self.dims, seed)

    def oracle(self, theta, lr=None, dtype=torch.float32):
        return W.oracle(self.dims, theta, dtype, (lr or (LR,))[0])

    def spec(self, tol_g, lr=None):
        lay, P = R.layout(self.dims)
        s = C.naf_spec(lay, P, (lr or (LR,))[0], TAU)                  # one Adam and the average over every tensor
        return s._replace(tol_g=lambda name, n: tol_g[name])

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        return self.select_kernel(_pop(self.dims, self.B, n_agents, (lr or (LR,))[0], cap, seeds))


@pytest.mark.parametrize("case", [WFCase((3, 1, 200, 200, 100), 32), WFCase((5, 2, 48, 64, 33), 32)], ids=lambda c: c.id)
def test_optimizer_state_and_target_after_one_update(hip_lib, case):
    """the schedule of tests/test_gpu_optimizer_state.py: a target apart from the weights, two warm-up updates, the whole
    state copied into a fresh restatement (and its float64 twin), one update on every side.  The gradient tolerance that
    checks a derive their m / v bounds from is the one the parity test holds each tensor to: max(5e-5, 3 e_ref)."""
    rng = np.random.RandomState(21)
    pop = case.pop()
    pop.enable_grad_taps(True)
    theta = case.theta0()
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", W.target_apart(theta, rng))
    for _ in range(2):
        pop.update_batch(0, *case.batch(rng))
    before = case.pop_state(pop)
    o, o64 = case.oracle(before["theta"]), case.oracle(before["theta"], dtype=torch.float64)
    C.load_oracle(o, before)
    C.load_oracle(o64, before)
    b = case.batch(rng)
    W.assert_tie_free(o, b, case.id)
    pop.update_batch(0, *b)
    taps, taps64 = o.update(*b, taps=True), o64.update(*b, taps=True)
    after = case.pop_state(pop)
    grads = case.pop_grads(pop)
    tol_g = {}
    for name, (off, shp) in o.layout.items():
        sl = slice(off, off + int(np.prod(shp)))
        tol_g[name] = max(5e-5, 3.0 * _rel(taps["grads"][sl], taps64["grads"][sl]))
        print("%s gradient %s: device %.3e against the restatement, tolerance %.3e" % (
            case.id, name, _rel(grads["grads"][sl], taps["grads"][sl]), tol_g[name]))
    pop.close()
    C.check_update(case.spec(tol_g), before, after, oracle_after=C.oracle_state(o), grads=case.grads(taps), label=case.id)


# ---- replay paths -----------------------------------------------------------------------------------------------------
def test_replay_path_host_indices_and_device_sampler(hip_lib):
    dims, B, NA, N, K = (5, 2, 48, 64, 33), 32, 2, 512, 2
    rng = np.random.RandomState(5)
    S, A = dims[:2]
    data = (rng.uniform(-1, 1, (N, S)), rng.uniform(-2, 2, (N, A)), rng.uniform(-16, 0, N), rng.uniform(-1, 1, (N, S)),
            np.where(rng.rand(N) < 0.2, 0.0, 0.99))
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(NA * K)]).reshape(NA, K, B).astype(np.int64)
    thetas = [R.init_params(dims, 30 + i) for i in range(NA)]

    def fresh():
        pop = _pop(dims, B, n_agents=NA, cap=N)
        for i in range(NA):
            pop.set_params(i, thetas[i], init_target=True)
            pop.replay_add_batch(i, *data)
        return pop

    one = fresh()
    one.update(K, host_indices=idx)                          # K updates in one launch
    many = fresh()
    for k in range(K):                                       # K launches of one update
        many.update(1, host_indices=idx[:, k:k + 1])
    for i in range(NA):
        for blob in ("theta", "theta_target", "adam_m", "adam_v"):
            assert np.array_equal(one.get_blob(i, blob), many.get_blob(i, blob)), (i, blob)
        assert np.array_equal(one.get_beta_powers(i), many.get_beta_powers(i))
        o = W.oracle(dims, thetas[i])
        s, a, r, s2, g = data
        for k in range(K):
            j = idx[i, k]
            t = o.update(s[j], a[j], s2[j], r[j], g[j], taps=True)
        for tap in ("q", "y", "max_q"):
            e = _rel(one.last_tap(i, tap), t[tap])
            print("replay agent %d tap %s after %d updates: %.3e" % (i, tap, K, e))
            assert e < 2e-4, (i, tap, e)
        assert not np.array_equal(one.get_blob(i, "theta"), thetas[i])
    many.close()
    one.update(3)                                            # the device's Philox sampler
    for i in range(NA):
        for blob in ("theta", "theta_target", "adam_m", "adam_v"):
            assert np.all(np.isfinite(one.get_blob(i, blob))), (i, blob)
        for tap in ("q", "y", "max_q"):
            assert np.all(np.isfinite(one.last_tap(i, tap))), (i, tap)
    one.close()


# ---- acting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(3, 1, 200, 200, 100), (2, 2, 16, 20, 65), (4, 6, 32, 32, 10), (1, 1, 16, 16, 1)],
                         ids=W.shape_id)
def test_act_and_qval_match_the_restatement(hip_lib, dims):
    """one state per agent of a six-agent population, every agent with weights of its own"""
    NA, S, A, N = 6, dims[0], dims[1], dims[4]
    rng = np.random.RandomState(9)
    pop = _pop(dims, 32, n_agents=NA, cap=64)
    o32, o64 = [], []
    for i in range(NA):
        th = R.init_params(dims, 50 + i)
        pop.set_params(i, th, init_target=True)
        o32.append(W.oracle(dims, th))
        o64.append(W.oracle(dims, th, torch.float64))
    states = rng.uniform(-1, 1, (NA, S))
    act, wa, wq = pop.act(states, with_wires=True)
    assert act.shape == (NA, A) and wa.shape == (NA, N, A) and wq.shape == (NA, N)
    for i in range(NA):
        W.assert_tie_free(o32[i], (states[i:i + 1], None, states[i:i + 1]), "act agent %d" % i)
        want, widx = o32[i].act(states[i:i + 1])
        ahat, qhat = o32[i].wires(states[i:i + 1])
        assert np.array_equal(act[i], wa[i, widx[0]])                               # the arg-max wire, its own bits
        for name, got, ref in (("action", act[i], want[0]), ("wire actions", wa[i], ahat[0]), ("wire values", wq[i], qhat[0])):
            scale = float(np.max(np.abs(ref))) if name == "wire values" else AMAX0   # actions: the action range
            e = float(np.max(np.abs(np.asarray(got, np.float64) - ref))) / scale
            print("act %s agent %d %s: %.3e" % (W.shape_id(dims), i, name, e))
            assert e < 1e-5, (i, name, e)
    assert np.array_equal(pop.act(states), act)                                     # out_wires NULL
    # queued: all six (stream wait), a sub-range, and one agent (the completion word)
    for first, n in ((0, NA), (3, 2), (5, 1)):
        assert pop.act_queue(states[first:first + n], first_agent=first) == n
        a2, wa2, wq2 = pop.act_fetch(n, first_agent=first, with_wires=True)
        assert np.array_equal(a2, act[first:first + n]), (first, n)
        assert np.array_equal(wa2, wa[first:first + n]) and np.array_equal(wq2, wq[first:first + n]), (first, n)
        assert pop.act_queue(states[first:first + n], first_agent=first) == n
        assert np.array_equal(pop.act_fetch(n, first_agent=first), act[first:first + n]), (first, n)
    actions = rng.uniform(-2, 2, (NA, A))
    for i in (0, NA - 1):
        rows = rng.uniform(-1, 1, (NA, S))
        _held("qval %s agent %d" % (W.shape_id(dims), i), pop.qval(i, rows, actions), o32[i].qval(rows, actions),
              o64[i].qval(rows, actions), 1e-5)
    if N == 1:                                                                      # one wire: Q is its value, bit for bit
        rows = np.repeat(states[:1], NA, axis=0)
        assert np.array_equal(pop.qval(0, rows, actions), np.repeat(wq[0], NA))
    pop.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_name(hip_lib):
    from rlcontrol_amd._lib import RlcError
    dims = (3, 1, 32, 32, 8)
    with pytest.raises(RlcError, match="layer"):
        _pop(dims, 16, norm_type="layer")
    with pytest.raises(RlcError, match="batch"):
        _pop(dims, 16, norm_type="batch")
    with pytest.raises(RlcError, match="action_dim <= 6"):
        _pop((3, 7, 32, 32, 8), 16)
    with pytest.raises(RlcError, match=r"app_points \* action_dim <= 1024 \(got 513 \* 2\)"):
        _pop((3, 2, 32, 32, 513), 16)
    with pytest.raises(RlcError, match="app_points must be >= 1"):
        _pop((3, 1, 32, 32, 0), 16)
    with pytest.raises(RlcError, match=r"need \d+ B of LDS \(> 65536\)"):
        _pop((3, 1, 9000, 9000, 8), 16)
    pop = _pop((3, 2, 32, 32, 512), 16)                                             # exactly at the limit
    pop.close()
    pop = _pop(dims, 16)
    with pytest.raises(RlcError, match="any-shape kernel only"):
        pop.set_kernel("mfma")
    with pytest.raises(RlcError, match="no latency mode"):
        pop.set_split(2)
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
    cfg.merge_config(dict({"norm_type": "input_norm", "exploration_policy": "ou_noise", "l1_dim": 200, "l2_dim": 200,
                           "learning_rate": 0.001, "app_points": 100, "batch_size": 32, "buffer_size": 5000,
                           "writer": None, "replay_sampler": "reference"}, **over))
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": seed})
    return cfg, env


def test_dropin_agent_follows_a_population_fed_the_same_minibatches(hip_lib):
    """200 seeded random transitions through agent.update / agent.step: the agent's theta equals, bit for bit, that of a
    WFPopulation given the same transitions and the same minibatch indices; every action is the restatement's arg-max
    wire (on the weights of that moment) plus the host's OU noise."""
    from rlcontrol_amd.hip_wf import WFPopulation
    from rlcontrol_amd.utils.exploration_policy import make_policy
    from rlcontrol_amd.utils.main_utils import create_agent
    seed, batch = 2, 32
    cfg, env = _config(seed, batch_size=batch)
    agent = create_agent("WireFitting", cfg)
    mgr = agent.network_manager
    pop = mgr.population
    dims = (env.state_dim, env.action_dim, 200, 200, 100)
    assert pop.P == 81300 and pop.dims == dims
    theta0 = pop.get_blob(0, "theta")
    assert np.array_equal(pop.get_blob(0, "theta_target"), theta0)
    amax0 = float(np.reshape(env.action_max, -1)[0])
    twin_pop = WFPopulation(1, *dims, batch, int(cfg.buffer_size), cfg.tau, env.state_min, env.state_max, amax0,
                            cfg.learning_rate, seeds=[np.uint64(seed)])
    twin_pop.set_params(0, theta0, init_target=True)
    drawn = []
    inner = mgr.update_from_replay

    def recording(indices, next_state=None):
        drawn.append(np.array(indices, np.int64))
        return inner(indices, next_state=next_state)
    mgr.update_from_replay = recording
    uses, noise = make_policy(cfg, seed, env.action_dim, env.action_min, env.action_max)     # the host policy's stream
    assert uses and mgr.use_external_exploration

    def restated_greedy(state):
        o = R.TorchWireFitting(dims, pop.get_blob(0, "theta"), cfg.learning_rate, cfg.tau, env.state_min, env.state_max, amax0)
        W.assert_tie_free(o, (state.reshape(1, -1), None, state.reshape(1, -1)), "drop-in")
        return o.act(state.reshape(1, -1))[0][0]

    rng = np.random.RandomState(seed)
    lo, hi = np.asarray(env.state_min, np.float64), np.asarray(env.state_max, np.float64)
    obs = rng.uniform(lo, hi)
    agent.reset(); noise.reset()
    greedy = pop.act(obs.reshape(1, -1))[0]
    assert np.max(np.abs(greedy - restated_greedy(obs))) <= 1e-5 * amax0
    a = agent.start(obs, True)
    assert np.array_equal(a, noise.generate(greedy, 1))
    fetched = updates = 0
    for t in range(200):
        obs_n, r = rng.uniform(lo, hi), float(rng.uniform(-16, 0))
        done = bool(rng.rand() < 0.02)
        agent.update(obs, obs_n, r, a, done, False)
        twin_pop.replay_add(0, obs, a, r, obs_n, 0.0 if done else cfg.gamma)
        if len(drawn) > updates:
            twin_pop.update(1, host_indices=drawn[-1])
            updates = len(drawn)
        if t + 1 == batch:
            assert updates == 0 and np.array_equal(pop.get_blob(0, "theta"), theta0)   # learn gate: size > batch (Q12)
        fetched += mgr._queued_state is not None
        greedy = pop.act(obs_n.reshape(1, -1))[0]                          # after the update, as step() sees it
        if t % 10 == 0:
            assert np.max(np.abs(greedy - restated_greedy(obs_n))) <= 1e-5 * amax0, t
        a = agent.step(obs_n, True)
        assert np.array_equal(a, noise.generate(greedy, t + 2)), t          # arg-max wire + the OU stream, clipped
        obs = obs_n
    assert updates == 200 - batch and fetched > 0.9 * updates
    for blob in ("theta", "theta_target", "adam_m", "adam_v"):
        assert np.array_equal(pop.get_blob(0, blob), twin_pop.get_blob(0, blob)), blob
    assert np.array_equal(pop.get_beta_powers(0), twin_pop.get_beta_powers(0))
    assert not np.array_equal(pop.get_blob(0, "theta"), theta0)
    assert agent.replay_buffer.get_size() == 200
    twin_pop.close()


RUN_KEYS = {"random_seed", "total_timesteps", "eval_interval_timesteps", "episodes_per_eval", "eval_episode_rewards",
            "eval_episode_steps", "timesteps_at_eval", "train_episode_steps", "train_episode_rewards",
            "total_train_episodes", "eval_time", "train_time"}


def test_main_host_loop_writes_the_result_pickle(hip_lib, tmp_path):
    import pickle
    import main as drv
    agent = {"agent": "WireFitting", "sweeps": {"norm_type": ["input_norm"], "exploration_policy": ["ou_noise"], "l1_dim": [32],
                                                "l2_dim": [32], "learning_rate": [1e-3], "app_points": [12],
                                                "batch_size": [16], "buffer_size": [1000]}}
    aj = tmp_path / "wirefitting.json"
    aj.write_text(json.dumps(agent))
    drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json"), "--agent_json", str(aj),
              "--indices", "0", "1", "1", "--save_dir", str(tmp_path), "--quiet"])
    files = glob.glob(str(tmp_path / "Bimodal1DEnv_wirefittingresults" / "data_0_1_1.pkl"))
    assert len(files) == 1, os.listdir(str(tmp_path))
    with open(files[0], "rb") as f:
        data = pickle.load(f)
    runs = data["experiment_data"][0]["runs"]
    assert len(runs) == 1 and set(runs[0]) == RUN_KEYS
    run = runs[0]
    assert run["total_timesteps"] == 750 and run["total_train_episodes"] == 750
    assert np.isfinite(run["eval_episode_rewards"]).all() and np.isfinite(run["train_episode_rewards"]).all()
    assert np.all(run["eval_episode_rewards"] == run["eval_episode_rewards"][:, :1])      # greedy: identical episodes
