"""ReverseKL / ForwardKL with a two-dimensional action on the MFMA update kernel (kl_mfma_kernel.h, AD = 2).

The kernel is opt-in at action_dim 2 (`set_kernel("mfma")`, json key `hip_kernel`); a new population keeps the any-shape
kernel.  Tolerances are the ones tests/test_kl.py uses for the same quantities on the any-shape kernel
(test_kl_hip_multi_dimensional_actions_match_oracle, test_kl_kernel_switch_repacks_weights_and_optimizer_state) and
tests/test_gpu_bimodal.py uses for SoftActorCritic on Bimodal2DEnv.
"""
import numpy as np
import pytest
import torch

from oracle import kl_torch as K

MODES = ([("reverse", o, q) for o in K.OPTIM_TYPES for q in K.Q_UPDATE_TYPES] +
         [("forward", "intg", q) for q in K.Q_UPDATE_TYPES])
# the Bimodal2DEnv json shape; a shape of test_kl.py's MULTI; S + A at the limit with unequal widths; seven batch tiles
# (the first-layer image of Q in global memory) at the widest layers whose LDS plan fits at batch 100 and A = 2
SHAPES = [((2, 2, 200, 200, 200, 200), 32, 6), ((3, 2, 64, 64, 64, 64), 32, 6), ((6, 2, 48, 40, 44, 36), 12, 5),
          ((4, 2, 128, 128, 128, 128), 100, 5)]


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _lively(d, th):
    """the U(+-3e-3) output layers give an almost state-independent policy; widen them so every path carries signal"""
    lay, _ = d.layout()
    th = th.copy()
    for name, scale in (("pWm", 30.0), ("pWs", 30.0), ("qW3", 30.0), ("vW3", 30.0)):
        off, shp = lay[name]
        th[off:off + int(np.prod(shp))] *= scale
    return th


def _batch_a(rng, B, S, A):
    return (rng.uniform(-2, 2, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-2, 2, (B, S)),
            rng.uniform(-16, 0, B), np.where(rng.rand(B) < 0.2, 0.0, 0.99), rng.randn(B, A))


def _pop(kind, dims, B, optim="intg", qup="non_sac", l_param=None, action_max=None, n_agents=1):
    from rlcontrol_amd.hip_kl import KLPopulation
    S, A, L1A, L2A, L1C, L2C = dims
    return KLPopulation(kind, n_agents, S, A, L1A, L2A, L1C, L2C, B, 2048, 0.01, 2.0, 1e-3, 1e-2, 0.3,
                        seeds=list(range(5, 5 + n_agents)), n_param=64, optim_type=optim, q_update_type=qup,
                        l_param=l_param, action_max=action_max)


# ------------------------------------------------------------------------------------------ 1: parity with the oracle
@pytest.mark.gpu
@pytest.mark.parametrize("kind,optim,qup", MODES)
@pytest.mark.parametrize("dims,B,l_param", SHAPES)
def test_kl_mfma_two_dimensional_actions_match_oracle(hip_lib, kind, optim, qup, dims, B, l_param):
    """the body of test_kl.py::test_kl_hip_multi_dimensional_actions_match_oracle on the MFMA kernel"""
    d = K.KlDims(*dims)
    S, A = dims[0], dims[1]
    rng = np.random.RandomState(3)
    th = _lively(d, K.init_params(d, 1))
    amax = np.full(A, 2.0)
    pop = _pop(kind, dims, B, optim, qup, l_param=l_param, action_max=amax)
    assert pop.kernel_in_use() == "generic"
    pop.set_kernel("mfma")                               # a refusal is a failure here, not a skip
    assert pop.kernel_in_use() == "mfma"
    pop.enable_grad_taps(True)
    pop.set_params(0, th)
    o = K.KLOracle(kind, d, th, 1e-3, 1e-2, 0.3, 0.01, 2.0, 0, optim, qup, l_param=l_param, action_max=amax)
    assert pop.n_nodes == len(o.weights)
    lay, _ = d.layout()
    st, e1 = rng.uniform(-2, 2, (4, S)), rng.randn(4, A)
    for i in range(4):                                   # acting under the tile-blocked layout
        assert _rel(pop.act(st[i:i + 1]), o.act(st[i:i + 1])) < 1e-5
        assert _rel(pop.act(st[i:i + 1], sample=True, eps=e1[i:i + 1]), o.act(st[i:i + 1], eps=e1[i:i + 1])) < 1e-5
    for it in range(3):
        s, a, s2, r, g, eps = _batch_a(rng, B, S, A)
        pop.update_batch(0, s, a, s2, r, g, eps=eps)
        t = o.update(s, a, s2, r, g, eps, taps=True)
        tol = 1e-5 if it == 0 else 2e-4
        for k in ("q", "v", "q_pi", "logp"):
            err = _rel(pop.last_tap(0, k), t[k])
            print("update %d %s: %.3e" % (it, k, err))
            assert err < tol, (it, k)
        if "intgrl_q" in t:
            err = _rel(pop.last_tap(0, "intgrl_q"), t["intgrl_q"])
            print("update %d intgrl_q: %.3e" % (it, err))
            assert err < tol, it
        err = _rel(pop.last_tap(0, "loss"), t["loss"])
        print("update %d loss: %.3e" % (it, err))
        assert err < 10 * tol, it
        if it == 0:
            got = pop.last_tap(0, "grads")
            for n, (off, shp) in lay.items():
                k = int(np.prod(shp))
                # the sparse grid's weights cancel (both signs): the policy gradient is a difference of large sums
                bound = 3e-4 if (n[0] == "p" or k == 1) else 5e-5
                err = _rel(got[off:off + k], t["grads"][off:off + k])
                print("grad %s: %.3e (bound %.0e)" % (n, err, bound))
                assert err < bound, n
            vo = lay["vW1"][0]
            assert _rel(pop.get_blob(0, "theta_target")[vo:], o.theta_t.numpy()[vo:]) < 1e-5
    assert pop.get_step(0) == 3
    pop.close()


# ------------------------------------------------------------------------------------------ 2: the switch re-packs
SWITCH = dict(dims=(3, 2, 64, 64, 64, 64), B=32, l_param=6, seed=5, updates=4)


def _near_relu_kink(o, s, a, margin=1.5e-6):
    """as in tests/test_kl.py: a hidden pre-activation of a differentiated network within fp32 rounding of zero"""
    p = K._views(o.theta, o.lay)
    s = torch.tensor(np.asarray(s, np.float32))
    xq = torch.cat([s, torch.tensor(np.asarray(a, np.float32))], 1)
    worst = float("inf")
    for pre, x in (("p", s), ("q", xq), ("v", s)):
        z1 = x @ p[pre + "W1"] + p[pre + "b1"]
        z2 = torch.relu(z1) @ p[pre + "W2"] + p[pre + "b2"]
        worst = min(worst, z1.abs().min().item(), z2.abs().min().item())
    return worst < margin


def _switch_trajectory(apply=None):
    """the minibatches of the switch test and the oracle behind them; apply(done, batch) sees every minibatch kept.
    Returns (oracle, initial theta, minibatches drawn, minibatches kept)."""
    c = SWITCH
    d = K.KlDims(*c["dims"])
    rng = np.random.RandomState(c["seed"])
    th = _lively(d, K.init_params(d, 7))
    amax = np.full(2, 2.0)
    o = K.KLOracle("reverse", d, th, 1e-3, 1e-2, 0.3, 0.01, 2.0, 0, l_param=c["l_param"], action_max=amax)
    drawn = done = 0
    while done < c["updates"]:
        batch = _batch_a(rng, c["B"], c["dims"][0], 2)
        drawn += 1
        assert drawn <= 2 * c["updates"], "more than half of the drawn minibatches sit on a ReLU kink"
        if _near_relu_kink(o, batch[0], batch[1]):
            continue
        o.update(*batch)
        done += 1
        if apply:
            apply(done, batch)
    return o, th, drawn, done


def test_kl_switch_seed_leaves_out_at_most_half_of_the_minibatches():
    """CPU: the seed of the switch test keeps the share of minibatches left out (ReLU kink) within the cap"""
    _, _, drawn, kept = _switch_trajectory()
    assert kept == SWITCH["updates"] and drawn - kept <= drawn // 2, (drawn, kept)


@pytest.mark.gpu
def test_kl_mfma_action2_kernel_switch_repacks_weights_and_optimizer_state(hip_lib):
    """generic <-> mfma at action_dim 2: blobs are bit-equal across the re-pack (theta, target, m, v) and the two kernels
    continue the same trajectory to summation-order accuracy"""
    c = SWITCH
    d = K.KlDims(*c["dims"])
    amax = np.full(2, 2.0)
    pa = _pop("reverse", c["dims"], c["B"], l_param=c["l_param"], action_max=amax)
    pb = _pop("reverse", c["dims"], c["B"], l_param=c["l_param"], action_max=amax)
    pa.set_kernel("mfma")
    assert pa.kernel_in_use() == "mfma" and pb.kernel_in_use() == "generic"
    th = _lively(d, K.init_params(d, 7))
    for p in (pa, pb):
        p.set_params(0, th)
    assert np.array_equal(pa.get_blob(0, "theta"), th) and np.array_equal(pa.get_blob(0, "theta_target"), th)

    def apply(done, batch):
        s, a, s2, r, g, eps = batch
        pa.update_batch(0, s, a, s2, r, g, eps=eps)
        pb.update_batch(0, s, a, s2, r, g, eps=eps)
        if done == 2:                                # swap the kernels mid-trajectory
            names = ("theta", "theta_target", "adam_m", "adam_v")
            before = [{w: p.get_blob(0, w) for w in names} for p in (pa, pb)]
            pa.set_kernel("generic"); pb.set_kernel("mfma")
            assert pa.kernel_in_use() == "generic" and pb.kernel_in_use() == "mfma"
            for p, bf in zip((pa, pb), before):
                for w, v in bf.items():
                    assert np.array_equal(p.get_blob(0, w), v), w

    o, _, drawn, kept = _switch_trajectory(apply)
    assert drawn - kept <= drawn // 2
    lay, _ = d.layout()
    vo = lay["vW1"][0]
    for w in ("theta", "adam_m", "adam_v"):
        assert _rel(pa.get_blob(0, w), pb.get_blob(0, w)) < 2e-4, w
    assert _rel(pa.get_blob(0, "theta_target")[vo:], pb.get_blob(0, "theta_target")[vo:]) < 2e-4
    assert _rel(pa.get_blob(0, "theta"), o.theta.numpy()) < 2e-4
    pa.close(); pb.close()


# ------------------------------------------------------------------------------------------ 3: device loop, Bimodal2DEnv
# Chosen on the CPU (the restatement alone, test_kl_bimodal2d_cases_meet_every_rule_on_the_cpu): a mean bias that heads
# for the upper goal at nearly full stride reaches it at step 4 (rule 2) or 5 (rule 4, the limit) depending on the draw,
# and misses it once learning has moved the policy (rule 3); every visited state stays at least 0.05 (squared distance)
# off the goal radius, far beyond the trajectory tolerance, so device and restatement agree on every `done`.
KL_2D = dict(dims=(2, 2, 32, 32, 32, 32), B=16, total=90, limit=5, l_param=5, qv_lr=1e-3, init_seed=300,
             reverse=dict(seeds=[31, 7777777777], alpha=[0.2, 0.05], pi_lr=3e-3, mean_bias=2.0, log_std_bias=-1.0),
             forward=dict(seeds=[31, 7777777777], alpha=[0.2, 0.05], pi_lr=3e-3, mean_bias=2.0, log_std_bias=-1.0))


def kl_2d_thetas(kind):
    c, k = KL_2D, KL_2D[kind]
    d = K.KlDims(*c["dims"])
    lay = d.layout()[0]
    out = []
    for i in range(2):
        th = K.init_params(d, c["init_seed"])
        off, shp = lay["pWs"]
        th[off:off + int(np.prod(shp))] *= 0.02
        th[lay["pbm"][0]:lay["pbm"][0] + 2] = k["mean_bias"]
        th[lay["pbs"][0]:lay["pbs"][0] + 2] = k["log_std_bias"]
        out.append(th)
    return d, out


def kl_2d_oracle(kind, a):
    """BimodalKlRolloutOracle on the sparse grid of level l_param (its own _make_net builds the line rule), with
    environments that record how close a visited state came to a goal's radius"""
    from helpers.bimodal_rollout import Bimodal2D, BimodalKlRolloutOracle
    c, k = KL_2D, KL_2D[kind]

    class Recording2D(Bimodal2D):
        def step(self, action):
            out = Bimodal2D.step(self, action)
            for gx in (-4.0, 4.0):
                self.margins.append(abs((gx - self.x) ** 2 + (gx - self.y) ** 2 - 0.5))
            return out

    class Oracle2D(BimodalKlRolloutOracle):
        def _make_net(self, dims, theta, actor_lr, critic_lr, tau, state_min, state_max, action_max, clip_state):
            kind_, pi_lr, qv_lr, alpha, amax0, n_param, optim_type, q_update_type = self._kl
            return K.KLOracle(kind_, dims, theta, pi_lr, qv_lr, alpha, tau, amax0, n_param, optim_type, q_update_type,
                              l_param=c["l_param"], action_max=np.ones(2))

    d, thetas = kl_2d_thetas(kind)
    orc = Oracle2D(kind, d, thetas[a], k["pi_lr"], c["qv_lr"], k["alpha"][a], 0.01, 1.0, 0, k["seeds"][a], c["B"], 4096,
                   0.99, 0, c["limit"], c["total"], 40, 2).use_env("Bimodal2DEnv")
    margins = []
    orc.train_env, orc.test_env = Recording2D(), Recording2D()
    orc.train_env.margins = orc.test_env.margins = margins
    orc.run()
    orc.goal_margin = min(margins)
    return orc


@pytest.mark.parametrize("kind", ["reverse", "forward"])
def test_kl_bimodal2d_cases_meet_every_rule_on_the_cpu(kind):
    """CPU: the restatement alone meets episode rules 2, 3 and 4 and keeps clear of the goal radius"""
    for a in range(2):
        orc = kl_2d_oracle(kind, a)
        rc = orc.rule_counts
        assert rc[2] >= 1 and rc[3] >= 1 and rc[4] >= 1 and rc[1] == 0, rc
        assert orc.goal_margin >= 0.05, orc.goal_margin


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["reverse", "forward"])
def test_kl_mfma_bimodal2d_matches_cpu_restatement(hip_lib, kind):
    from test_gpu_bimodal import _check_2d, env_json
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_kl import KLPopulation
    c, k = KL_2D, KL_2D[kind]
    pop = KLPopulation(kind, 2, *c["dims"], c["B"], 4096, 0.01, 1.0, k["pi_lr"], c["qv_lr"], k["alpha"], seeds=k["seeds"],
                       n_param=64, l_param=c["l_param"], action_max=np.ones(2))
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma" and pop.n_nodes == 73
    for i, th in enumerate(kl_2d_thetas(kind)[1]):
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, env_json("Bimodal2DEnv", c["total"], c["limit"], 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(37) == 37
    exp.advance(1000)
    oracles = [kl_2d_oracle(kind, a) for a in range(2)]
    for orc in oracles:
        assert orc.goal_margin >= 0.05
    _check_2d(pop, exp, exp.results(), oracles, c["total"], c["B"], 5e-6, 5e-3)     # asserts the rule counts too
    for a, orc in enumerate(oracles):
        assert pop.get_step(a) == orc.net.step == orc.n_updates
        want = orc.net.theta.numpy()
        assert np.max(np.abs(pop.get_blob(a, "theta") - want)) < 5e-3 * np.max(np.abs(want))
    pop.close()


# ------------------------------------------------------------------------------------------ 4: refusals
@pytest.mark.gpu
def test_kl_mfma_refuses_what_it_does_not_cover(hip_lib):
    from rlcontrol_amd._lib import RlcError
    pop = _pop("reverse", (4, 3, 32, 32, 32, 32), 9, l_param=4, action_max=np.full(3, 2.0))
    with pytest.raises(RlcError, match="action_dim 1 and 2"):
        pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "generic"
    pop.close()
    pop = _pop("reverse", (7, 2, 32, 32, 32, 32), 9, l_param=5, action_max=np.full(2, 2.0))
    with pytest.raises(RlcError, match=r"state_dim \+ action_dim <= 8"):
        pop.set_kernel("mfma")
    pop.close()
    pop = _pop("reverse", (3, 2, 32, 32, 32, 32), 9, l_param=7, action_max=np.full(2, 2.0))
    assert pop.n_nodes == 461
    with pytest.raises(RlcError, match="at most 256 quadrature nodes"):
        pop.set_kernel("mfma")
    pop.close()
    pop = _pop("reverse", (2, 2, 200, 200, 200, 200), 100, l_param=5, action_max=np.full(2, 2.0))
    with pytest.raises(RlcError, match="160 KiB of LDS"):
        pop.set_kernel("mfma")
    pop.close()
    # latency mode stays at action_dim 1; a new population at action_dim 2 runs the any-shape kernel, and so does "auto"
    pop = _pop("reverse", (3, 2, 64, 64, 64, 64), 32, l_param=6, action_max=np.full(2, 2.0))
    assert pop.kernel_in_use() == "generic"
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    with pytest.raises(RlcError, match="action_dim 1"):
        pop.set_split(2)
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"
    pop.close()


# ------------------------------------------------------------------------------------------ 5: agent surface
def _agent_cfg(action_dim, **extra):
    from rlcontrol_amd.utils.config import Config
    cfg = Config()
    cfg.merge_config({"env_name": "synthetic", "state_dim": 4, "state_min": -np.ones(4), "state_max": np.ones(4),
                      "action_dim": action_dim, "action_min": -np.ones(action_dim), "action_max": np.ones(action_dim)})
    cfg.merge_config({"norm_type": "input_norm", "exploration_policy": "none", "actor_l1_dim": 32, "actor_l2_dim": 32,
                      "critic_l1_dim": 32, "critic_l2_dim": 32, "pi_lr": 1e-3, "qf_vf_lr": 1e-3,
                      "sample_for_eval": "False", "use_true_q": "False", "entropy_scale": 0.1, "l_param": 5, "N_param": 64,
                      "optim_type": "intg", "q_update_type": "non_sac", "buffer_size": 500, "writer": None,
                      "write_log": False, "write_plot": False, "random_seed": 0})
    cfg.merge_config(extra)
    return cfg


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["ReverseKL", "ForwardKL"])
def test_kl_dropin_agent_honours_hip_kernel(hip_lib, name):
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.utils.main_utils import create_agent
    agent = create_agent(name, _agent_cfg(2, hip_kernel="mfma"))
    pop = agent.network_manager.population
    assert pop.kernel_in_use() == "mfma" and pop.n_nodes == 73
    rng = np.random.RandomState(0)
    obs = rng.uniform(-1, 1, 4)
    agent.reset()
    a = agent.start(obs, True)
    for t in range(50):
        obs_n = rng.uniform(-1, 1, 4)
        agent.update(obs, obs_n, float(-np.sum(a ** 2)), a, False, False)
        a = agent.step(obs_n, True)
        obs = obs_n
        assert a.shape == (2,) and np.all(np.abs(a) <= 1.0)
    assert pop.get_step(0) == 50 - 32
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))
    # without the key: the any-shape kernel at action_dim 2, the MFMA kernel at action_dim 1, where "generic" is honoured
    assert create_agent(name, _agent_cfg(2)).network_manager.population.kernel_in_use() == "generic"
    assert create_agent(name, _agent_cfg(1)).network_manager.population.kernel_in_use() == "mfma"
    assert create_agent(name, _agent_cfg(1, hip_kernel="generic")).network_manager.population.kernel_in_use() == "generic"
    with pytest.raises(ValueError, match="hip_kernel"):
        create_agent(name, _agent_cfg(1, hip_kernel="fast"))
    with pytest.raises(RlcError, match="action_dim 1"):                       # hip_split with action_dim 2
        create_agent(name, _agent_cfg(2, hip_kernel="mfma", hip_split=2))
