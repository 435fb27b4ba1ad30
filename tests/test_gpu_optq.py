"""OptimalQ on the MI355X against its torch restatement (tests/torch_ref_optq.py): the fused update (target prelude, grid-max
pass, online step), the optimizer state per element, the replay paths, acting / Q values, what the library refuses, and
the drop-in agent through the host loop.

a_star condition (the index of a maximum is not stable under rounding when two nodes' values nearly tie): for every row the
restatement's Q at the node the DEVICE chose lies within 1e-5 * max|Q| of the restatement's own maximum, and the device's
node differs from the restatement's in at most 2 % of a case's rows (a case of the update test: its three updates).
Measured on an MI355X: 1 of the 96 rows of the shipped shape (4001 nodes at 1e-3: near an interior maximum neighbouring
nodes lie within a few fp32 ulps of each other), no row of any other case; DESIGN.md 5.12 has the analysis."""
import glob
import json
import os

import numpy as np
import pytest

import optimizer_state_checks as C
import torch_ref_optq as R
from optimizer_state_cases import TAU, Case

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR = 1e-3


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _bounds(S):
    return -np.ones(S) * 1.5, np.ones(S) * 1.5              # inside the states' range: the clip is active


def _theta(dims, seed):
    th = R.init_params(dims, seed)
    th[R.layout(dims)[0]["W3"][0]:] *= 100.0                # an output layer that matters to Q and to its maximum
    return th


def _pop(dims, B, grid, n_agents=1, lr=LR, cap=512, seeds=None, **kw):
    from rlcontrol_amd.hip_optq import OptQPopulation
    smin, smax = _bounds(dims[0])
    return OptQPopulation(n_agents, *dims, B, cap, TAU, smin, smax, lr,
                          seeds=seeds if seeds is not None else list(range(7, 7 + n_agents)),
                          node_actions=grid, **kw)


def _oracle(dims, theta, grid, lr=LR):
    smin, smax = _bounds(dims[0])
    return R.TorchOptimalQ(dims, theta, lr, TAU, smin, smax, grid)


def _batch(rng, dims, B):
    S, A = dims[:2]
    return (rng.uniform(-2, 2, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-2, 2, (B, S)), rng.uniform(-16, 0, B),
            np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def _node_of(grid32, rows):
    """index of each device-chosen grid row (exact fp32 match: the device returns rows of the uploaded grid)"""
    rows = np.asarray(rows, np.float32).reshape(-1, grid32.shape[1])
    out = []
    for r in rows:
        hit = np.nonzero(np.all(grid32 == r, axis=1))[0]
        assert hit.size >= 1, r
        out.append(int(hit[0]))
    return np.array(out)


def _check_a_star(qgrid, dev_nodes, label, cap_rows=None):
    """qgrid [n][n_nodes]: the restatement's Q at every node; dev_nodes [n]: the device's choice.  Returns the number of
    rows on another node; cap_rows: the rows the 2 % cap is taken of (this call's own when None, else the caller sums)"""
    qgrid = np.asarray(qgrid, np.float64)
    n = qgrid.shape[0]
    best = qgrid.max(1)
    at_dev = qgrid[np.arange(n), dev_nodes]
    gap = float(np.max(best - at_dev) / (np.max(np.abs(qgrid)) + 1e-30))
    differ = int(np.sum(dev_nodes != np.argmax(qgrid, 1)))
    print("%s a_star: worst gap %.3e of max|Q|, %d of %d rows on another node" % (label, gap, differ, n))
    assert np.all(best - at_dev <= 1e-5 * np.max(np.abs(qgrid))), (label, gap)
    if cap_rows is None:
        assert differ <= 0.02 * n, (label, differ, n)
    return differ


# (S, A, L1, L2), batch, (lo, hi), discretization, nodes
UPDATE_CASES = [((5, 1, 40, 24), 17, (-2.0, 2.0), 0.1, 41),
                ((3, 1, 200, 200), 32, (-2.0, 2.0), 1e-3, 4001),
                ((4, 2, 32, 48), 32, (-2.0, 2.0), 0.2, 441),
                ((3, 1, 64, 72), 100, (-1.0, 1.0), 0.01, 201),
                ((6, 3, 48, 40), 9, (-1.0, 1.0), 0.5, 125),
                ((5, 1, 40, 24), 17, (-2.0, 2.0), 8.0, 1)]


@pytest.mark.parametrize("dims,B,box,disc,nodes", UPDATE_CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_three_updates_match_the_restatement(hip_lib, dims, B, box, disc, nodes):
    """first update: taps 1e-5, gradients 5e-5 per tensor, theta / theta_target 1e-5; the two after it: taps 2e-4"""
    from rlcontrol_amd.hip_optq import action_grid
    grid = action_grid([box[0]], [box[1]], disc, dims[1])
    assert grid.shape == (nodes, dims[1])
    grid32 = grid.astype(np.float32)
    rng = np.random.RandomState(17)
    theta = _theta(dims, 3)
    target = (theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32)
    pop = _pop(dims, B, grid)
    assert pop.P == theta.size and pop.kernel_in_use() == "generic"
    pop.enable_grad_taps(True)
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", target)
    o = _oracle(dims, theta, grid)
    o.theta_t = o.theta_t * 0 + R.torch.as_tensor(target)
    label = "x".join(map(str, dims)) + "/B%d/%d nodes" % (B, nodes)
    differ = 0                                               # rows of the case (three updates) on another node
    for step in range(3):
        b = _batch(rng, dims, B)
        qgrid = o.grid_q(b[2], target=True).numpy()          # with the target of BEFORE this update
        pop.update_batch(0, *b)
        t = o.update(*b, taps=True)
        tol = 1e-5 if step == 0 else 2e-4
        for k in ("q", "y", "max_q"):
            e = _rel(pop.last_tap(0, k), t[k])
            print("%s update %d tap %s: %.3e" % (label, step, k, e))
            assert e < tol, (step, k, e)
        differ += _check_a_star(qgrid, _node_of(grid32, pop.last_tap(0, "a_star")), "%s update %d" % (label, step), 3 * B)
        if step == 0:
            g = pop.last_tap(0, "grads")
            for n, (off, shp) in o.layout.items():
                k = int(np.prod(shp))
                e = _rel(g[off:off + k], t["grads"][off:off + k])
                print("%s gradient %s: %.3e" % (label, n, e))
                assert e < 5e-5, (n, e)
            assert _rel(pop.get_blob(0, "theta"), o.theta.numpy()) < 1e-5
            assert _rel(pop.get_blob(0, "theta_target"), o.theta_t.numpy()) < 1e-5
    print("%s a_star: %d of the case's %d rows on another node" % (label, differ, 3 * B))
    assert differ <= 0.02 * 3 * B, (label, differ, 3 * B)
    assert _rel(pop.get_blob(0, "theta"), o.theta.numpy()) < 2e-4
    assert _rel(pop.get_blob(0, "theta_target"), o.theta_t.numpy()) < 2e-4
    assert np.allclose(pop.get_beta_powers(0), o.pw, rtol=1e-6, atol=0)
    pop.close()


# ---- the optimizer state per element (tests/optimizer_state_checks.py, checks a to e) ----------------------------------
class OptQCase(Case):
    NAME = "optq"

    def __init__(self, dims, B, box, disc):
        Case.__init__(self, dims, B, "generic")
        from rlcontrol_amd.hip_optq import action_grid
        self.grid = action_grid([box[0]], [box[1]], disc, self.A)

    def theta0(self, seed=2):
        return _theta(self.dims, seed)

    def oracle(self, theta, lr=None):
        return _oracle(self.dims, theta, self.grid, (lr or (LR,))[0])

    def spec(self, lr=None):
        lay, P = R.layout(self.dims)
        return C.naf_spec(lay, P, (lr or (LR,))[0], TAU, tol_g=5e-5)          # one Adam and the average over every tensor

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        return self.select_kernel(_pop(self.dims, self.B, self.grid, n_agents, (lr or (LR,))[0], cap, seeds))


@pytest.mark.parametrize("case", [OptQCase((3, 1, 200, 200), 32, (-2.0, 2.0), 1e-3), OptQCase((3, 1, 64, 72), 100, (-1.0, 1.0), 0.01)],
                         ids=lambda c: c.id)
def test_optimizer_state_and_target_after_one_update(hip_lib, case):
    """the schedule of tests/test_gpu_optimizer_state.py: a target apart from the weights, two warm-up updates, the whole
    state copied into a fresh restatement, one update on both sides"""
    rng = np.random.RandomState(21)
    spec = case.spec()
    pop = case.pop()
    pop.enable_grad_taps(True)
    theta = case.theta0()
    pop.set_params(0, theta, init_target=False)
    pop.set_blob(0, "theta_target", case.target_apart(theta, rng))
    for _ in range(2):
        pop.update_batch(0, *case.batch(rng))
    before = case.pop_state(pop)
    o = case.oracle(before["theta"])
    C.load_oracle(o, before)
    b = case.batch(rng)
    pop.update_batch(0, *b)
    taps = o.update(*b, taps=True)
    after = case.pop_state(pop)
    grads = case.pop_grads(pop)
    for name, off, n in C._tensors(spec, [(0, spec.P)]):
        print("%s gradient %s: %.3e" % (case.id, name, _rel(grads["grads"][off:off + n], taps["grads"][off:off + n])))
    pop.close()
    C.check_update(spec, before, after, oracle_after=C.oracle_state(o), grads=case.grads(taps), label=case.id)


# ---- replay paths -----------------------------------------------------------------------------------------------------
def test_replay_path_host_indices_and_device_sampler(hip_lib):
    from rlcontrol_amd.hip_optq import action_grid
    dims, B, NA, N, K = (4, 2, 32, 48), 32, 2, 512, 2
    grid = action_grid([-2.0], [2.0], 0.2, 2)
    rng = np.random.RandomState(5)
    S, A = dims[:2]
    data = (rng.uniform(-2, 2, (N, S)), rng.uniform(-2, 2, (N, A)), rng.uniform(-16, 0, N), rng.uniform(-2, 2, (N, S)),
            np.where(rng.rand(N) < 0.2, 0.0, 0.99))
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(NA * K)]).reshape(NA, K, B).astype(np.int64)
    thetas = [_theta(dims, 30 + i) for i in range(NA)]

    def fresh():
        pop = _pop(dims, B, grid, n_agents=NA, cap=N)
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
        o = _oracle(dims, thetas[i], grid)
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
        for tap in ("q", "y", "max_q", "a_star"):
            assert np.all(np.isfinite(one.last_tap(i, tap))), (i, tap)
    one.close()


# ---- acting -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,box,disc", [((3, 1, 200, 200), (-2.0, 2.0), 1e-3), ((4, 2, 32, 48), (-2.0, 2.0), 0.2),
                                           ((5, 1, 40, 24), (-2.0, 2.0), 8.0)], ids=["shipped", "two_dims", "one_node"])
def test_act_and_qval_match_the_restatement(hip_lib, dims, box, disc):
    """one state per agent of an eight-agent population, every agent with weights of its own"""
    from rlcontrol_amd.hip_optq import action_grid
    NA, S, A = 8, dims[0], dims[1]
    grid = action_grid([box[0]], [box[1]], disc, A)
    grid32 = grid.astype(np.float32)
    rng = np.random.RandomState(9)
    pop = _pop(dims, 32, grid, n_agents=NA, cap=64)
    oracles = []
    for i in range(NA):
        th = _theta(dims, 50 + i)
        pop.set_params(i, th, init_target=True)
        oracles.append(_oracle(dims, th, grid))
    states = rng.uniform(-2, 2, (NA, S))
    act, q = pop.act(states, with_q=True)
    assert act.shape == (NA, A) and q.shape == (NA,)
    qgrid = np.concatenate([oracles[i].grid_q(states[i:i + 1]).numpy() for i in range(NA)])
    _check_a_star(qgrid, _node_of(grid32, act), "act %s" % (dims,))
    e = _rel(q, qgrid.max(1))
    print("act %s out_q: %.3e" % (dims, e))
    assert e < 1e-5
    assert np.array_equal(pop.act(states), act)                                 # out_q NULL
    # queued: all eight (stream wait), a sub-range, and one agent (the completion word)
    for first, n in ((0, NA), (3, 2), (5, 1)):
        assert pop.act_queue(states[first:first + n], first_agent=first) == n
        a2, q2 = pop.act_fetch(n, first_agent=first, with_q=True)
        assert np.array_equal(a2, act[first:first + n]) and np.array_equal(q2, q[first:first + n]), (first, n)
    actions = rng.uniform(box[0], box[1], (NA, A))
    for i in (0, NA - 1):
        rows = rng.uniform(-2, 2, (NA, S))
        e = _rel(pop.qval(i, rows, actions), oracles[i].qval(rows, actions))
        print("qval %s agent %d: %.3e" % (dims, i, e))
        assert e < 1e-5
    pop.close()


# ---- refusals ----------------------------------------------------------------------------------------------------------
def test_refusals_by_name(hip_lib):
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.hip_optq import action_grid
    dims = (3, 1, 32, 32)
    grid = action_grid([-2.0], [2.0], 0.5, 1)
    with pytest.raises(RlcError, match="layer"):
        _pop(dims, 16, grid, norm_type="layer")
    with pytest.raises(RlcError, match="batch"):
        _pop(dims, 16, grid, norm_type="batch")
    with pytest.raises(RlcError, match="n_nodes 0"):
        _pop(dims, 16, np.zeros((0, 1)))
    with pytest.raises(RlcError, match="action_dim <= 6"):
        _pop((3, 7, 32, 32), 16, np.zeros((4, 7)))
    pop = _pop(dims, 16, grid)
    with pytest.raises(RlcError, match="any-shape kernel only"):
        pop.set_kernel("mfma")
    with pytest.raises(RlcError, match="latency mode"):
        pop.set_split(2)
    pop.set_kernel("generic"); pop.set_kernel("auto"); pop.set_split(1)
    assert pop.kernel_in_use() == "generic"
    pop.close()


# ---- the drop-in agent -------------------------------------------------------------------------------------------------
def _config(seed, batch=32):
    from rlcontrol_amd.environments.environments import create_environment
    from rlcontrol_amd.utils.config import Config
    env = create_environment({"environment": "Pendulum-v0", "TotalMilSteps": 0.001, "EpisodeSteps": -1,
                              "EvalIntervalMilSteps": 0.0005, "EvalEpisodes": 2})
    cfg = Config()
    cfg.merge_config({"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min,
                      "state_max": env.state_max, "action_dim": env.action_dim, "action_min": env.action_min,
                      "action_max": env.action_max})
    cfg.merge_config({"norm_type": "input_norm", "exploration_policy": "ou_noise", "l1_dim": 200, "l2_dim": 200,
                      "learning_rate": 0.001, "discretization": 0.05, "batch_size": batch, "buffer_size": 5000,
                      "writer": None, "replay_sampler": "reference"})
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": seed})
    return cfg, env


def test_dropin_agent_start_step_update(hip_lib):
    from rlcontrol_amd.hip_optq import action_grid
    from rlcontrol_amd.utils.exploration_policy import make_policy
    from rlcontrol_amd.utils.main_utils import create_agent
    seed, batch = 2, 32
    cfg, env = _config(seed, batch)
    agent = create_agent("OptimalQ", cfg)
    mgr = agent.network_manager
    pop = mgr.population
    grid32 = action_grid(env.action_min, env.action_max, 0.05, 1).astype(np.float32)
    assert pop.n_nodes == grid32.shape[0] == 81 and pop.P == 41401
    theta0 = pop.get_blob(0, "theta")
    assert np.array_equal(pop.get_blob(0, "theta_target"), theta0)
    uses, twin = make_policy(cfg, seed, env.action_dim, env.action_min, env.action_max)     # the host policy's stream
    assert uses and mgr.use_external_exploration
    for probe in ([1.0, 0.0, 0.5], [-1.0, 0.0, -2.0], [0.0, 1.0, 4.0]):
        a = agent.start(np.array(probe), False)                                            # greedy evaluation action
        assert a.shape == (1,) and np.any(grid32[:, 0] == a[0]), a
    env.set_random_seed(seed)
    obs = env.reset()
    agent.reset(); twin.reset()
    greedy = pop.act(obs.reshape(1, -1))[0]
    a = agent.start(obs, True)
    assert np.array_equal(a, twin.generate(greedy, 1))
    fetched = 0
    for t in range(100):
        obs_n, r, done, _ = env.step(a)
        agent.update(obs, obs_n, float(r), a, done, False)
        if t + 1 == batch:
            assert np.array_equal(pop.get_blob(0, "theta"), theta0)        # learn gate: size > max(warmup, batch) (Q12)
        fetched += mgr._queued_state is not None
        greedy = pop.act(obs_n.reshape(1, -1))[0]                          # after the update, as step() sees it
        assert np.any(grid32[:, 0] == greedy[0])
        a = agent.step(obs_n, True)
        assert np.array_equal(a, twin.generate(greedy, t + 2)), t          # greedy row + the OU stream, clipped
        obs = obs_n
    assert fetched == 100 - batch                                          # every step after the first update was queued
    for blob in ("theta", "theta_target", "adam_m", "adam_v"):
        assert np.all(np.isfinite(pop.get_blob(0, blob))), blob
    assert not np.array_equal(pop.get_blob(0, "theta"), theta0)
    assert agent.replay_buffer.get_size() == 100


RUN_KEYS = {"random_seed", "total_timesteps", "eval_interval_timesteps", "episodes_per_eval", "eval_episode_rewards",
            "eval_episode_steps", "timesteps_at_eval", "train_episode_steps", "train_episode_rewards",
            "total_train_episodes", "eval_time", "train_time"}


def test_main_host_loop_bimodal1d_writes_the_result_pickle(hip_lib, tmp_path):
    import pickle
    import main as drv
    agent = {"agent": "OptimalQ", "sweeps": {"norm_type": ["input_norm"], "exploration_policy": ["ou_noise"], "l1_dim": [32],
                                             "l2_dim": [32], "learning_rate": [1e-3], "discretization": [0.1],
                                             "batch_size": [16], "buffer_size": [1000]}}
    aj = tmp_path / "optimalq.json"
    aj.write_text(json.dumps(agent))
    drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json"), "--agent_json", str(aj),
              "--indices", "0", "1", "1", "--save_dir", str(tmp_path), "--quiet"])
    files = glob.glob(str(tmp_path / "Bimodal1DEnv_optimalqresults" / "data_0_1_1.pkl"))
    assert len(files) == 1, os.listdir(str(tmp_path))
    with open(files[0], "rb") as f:
        data = pickle.load(f)
    assert data["experiment"]["environment"]["env_name"] == "Bimodal1DEnv"
    runs = data["experiment_data"][0]["runs"]
    assert len(runs) == 1 and set(runs[0]) == RUN_KEYS
    run = runs[0]
    assert run["total_timesteps"] == 750 and run["total_train_episodes"] == 750
    assert run["eval_episode_rewards"].shape == (151, 10) and np.isfinite(run["eval_episode_rewards"]).all()
    assert np.all(run["eval_episode_rewards"] == run["eval_episode_rewards"][:, :1])      # greedy: identical episodes
    assert np.isfinite(run["train_episode_rewards"]).all()
    with pytest.raises(RuntimeError, match="--device_rollout is built for"):
        drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json"), "--agent_json", str(aj),
                  "--indices", "0", "1", "1", "--save_dir", str(tmp_path), "--device_rollout", "--quiet"])
