"""ActorExpert on the CPU: the parameter layout, the shipped json, top_k, the restatement's draws against numpy's
RandomState, the torch restatement (tests/torch_ref_ae.py) against its float64 twin, the summed backward seeds the kernel
uses against autograd through the reference's own form (float64), the two optimizers' ownership, the ABI's symbols and
the loud failure of the agent without a GPU.

Parity unpinned: no reference fixture exercises this agent."""
import json
import os

import numpy as np
import pytest
import torch

import ae_cases as W
import torch_ref_ae as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def test_param_layout_order_and_count():
    from rlcontrol_amd.hip_ae import init_params, param_layout
    lay, P = param_layout(3, 1, 200, 200, 200, 1)
    assert list(lay) == list(R.NAMES)
    assert P == 800 + 40200 + 3 * 201 + 201 * 200 + 200 + 201 == 82204
    assert lay["Wq2"] == (800 + 40200 + 603, (201, 200)) and lay["bq3"] == (P - 1, (1,))
    for dims in [s[:6] for s, _ in W.SHAPES]:
        lay_r, P_r = R.layout(dims)
        lay_p, P_p = param_layout(*dims)
        assert P_r == P_p and list(lay_r.items()) == list(lay_p.items())
        assert np.array_equal(init_params(*dims, seed=4), R.init_params(dims, 4))
    th = init_params(3, 2, 200, 200, 200, 2, 0)
    lay, _ = param_layout(3, 2, 200, 200, 200, 2)
    v = {k: th[o:o + int(np.prod(s))] for k, (o, s) in lay.items()}
    assert 0.0 <= np.min(v["Ws"]) < 0.01 and 0.99 < np.max(v["Ws"]) <= 1.0             # the sigma head: U(0, 1)
    for name in ("Wal", "bal", "bs", "Wq3", "bq3"):                                      # +-3e-3
        assert np.max(np.abs(v[name])) <= 0.003 and (v[name].size < 50 or np.max(np.abs(v[name])) > 0.0025), name
    for name, fan_in in (("W1", 3), ("b1", 200), ("Wa2", 200), ("Wm", 200), ("Wq2", 202), ("bq2", 200)):
        lim = np.sqrt(3.0 / fan_in)                                                      # variance_scaling, FAN_IN, uniform
        assert 0.9 * lim < np.max(np.abs(v[name])) <= lim * (1 + 1e-6), name


def test_shipped_json_sweeps_sixteen_settings():
    from rlcontrol_amd.utils.main_utils import get_sweep_parameters
    with open(os.path.join(ROOT, "jsonfiles", "agent", "ae.json")) as f:
        aj = json.load(f, object_pairs_hook=__import__("collections").OrderedDict)
    assert aj["agent"] == "ActorExpert"
    params, total = get_sweep_parameters(aj["sweeps"], 0)
    assert total == 16
    assert dict(params) == {"norm_type": "input_norm", "exploration_policy": "none", "shared_l1_dim": 200, "actor_l2_dim": 200,
                            "expert_l2_dim": 200, "actor_lr": 0.01, "expert_lr": 1, "rho": 0.05, "num_samples": 120,
                            "num_modal": 1, "use_uniform_sampling": "False", "use_better_q_gd": "False",
                            "sarsa_update": "True", "sample_for_eval": "False", "use_true_q": "False"}
    got = [(get_sweep_parameters(aj["sweeps"], i)[0]["actor_lr"], get_sweep_parameters(aj["sweeps"], i)[0]["expert_lr"])
           for i in range(16)]
    assert got == [(a, e) for e in (1, 0.1, 0.01, 0.001) for a in (0.01, 0.001, 0.0001, 0.00001)]


def test_top_k_is_formed_as_the_reference_forms_it():
    from rlcontrol_amd.hip_ae import top_k
    assert [top_k(n, rho) for n, rho in ((120, 0.05), (30, 0.2), (1, 1.0))] == [6, 6, 1]


@pytest.mark.parametrize("M", [1, 2, 3, 8])
def test_mode_rule_is_numpy_choice(M):
    """RandomState.choice(M, n, p) consumes random_sample(n) and searches its cdf: the restatement's rule on the same
    uniforms gives the same modes"""
    p = np.random.RandomState(M).dirichlet(np.ones(M)).astype(np.float32)
    p64 = p.astype(np.float64) / p.astype(np.float64).sum()                              # choice wants a sum of 1 to 1e-8
    want = np.random.RandomState(5).choice(M, 500, p=p64)
    u = np.random.RandomState(5).random_sample(500)
    assert np.array_equal(R.modes_of(p64, u), want)


def test_normal_draw_is_mean_plus_sigma_times_standard_normal():
    mean, sigma = np.random.RandomState(1).uniform(-2, 2, (7, 3)), np.random.RandomState(2).uniform(0.01, 2, (7, 3))
    want = np.random.RandomState(9).normal(mean, sigma)
    got = mean + sigma * np.random.RandomState(9).standard_normal((7, 3))
    assert np.array_equal(got, want)


# the first seed of range(200) whose three updates satisfy conditions (a) to (d)
# on the fp32 restatement, found by ae_cases.find_seed; tests/test_gpu_ae.py uses the same
SEEDS = W.CASE_SEEDS


@pytest.mark.parametrize("dims,B", W.SHAPES, ids=W.shape_id)
def test_restatement_fp32_agrees_with_its_float64_twin(dims, B):
    """the conditions on the inputs hold at the recorded seed (one update here, three on the GPU), the taps agree at
    1e-5, the two gradient blobs per tensor at 1e-4 of the tensor's largest element, the selected sets exactly"""
    seed = SEEDS[(dims, B)]
    rng = np.random.RandomState(seed)
    theta = W.theta_for_tests(dims, 3)
    target = W.target_apart(theta, rng)
    o32, o64 = W.oracle(dims, theta), W.oracle(dims, theta, torch.float64)
    for o in (o32, o64):
        o.theta_t = torch.as_tensor(target).to(o.dt)
    b = W.batch(rng, dims, B)
    u, eps = W.draws(rng, dims, B)
    u = W.nudge(o32, b, u)
    t32, t64 = o32.update(*b, u, eps, taps=True), o64.update(*b, u, eps, taps=True)
    assert W.condition_failures(t32, dims, u) == []
    assert np.array_equal(t32["selected"], t64["selected"])
    for k in ("q", "y", "a_next", "samples", "sample_q", "actor_loss"):
        e = _rel(t32[k], t64[k])
        print("%s/B%d tap %s: %.3e" % (dims, B, k, e))
        assert e < 1e-5, k
    for which in ("grads_a", "grads_e"):
        for n, (off, shp) in o32.layout.items():
            sl = slice(off, off + int(np.prod(shp)))
            if not np.any(t64[which][sl]):
                assert not np.any(t32[which][sl]), (which, n)                            # not this optimizer's tensor
                continue
            e = _rel(t32[which][sl], t64[which][sl])
            print("%s/B%d %s %s: %.3e" % (dims, B, which, n, e))
            assert e < 1e-4, (which, n)


def test_find_seed_reports_the_recorded_seed_of_a_small_shape():
    dims, B = W.SHAPES[1]
    assert W.find_seed(dims, B, 3, range(200)) == SEEDS[(dims, B)]


@pytest.mark.parametrize("dims,B", W.SHAPES[:4], ids=W.shape_id)
def test_summed_seeds_equal_autograd_through_the_reference_form(dims, B):
    """float64: the gradient of the actor loss with respect to (alpha, mean, sigma) at B rows, the seeds summed over each
    row's k chosen actions in log space, against autograd through B*k stacked rows, the linear-space product and clamp"""
    S, A, L1, La, Le, M, n, k = dims
    rng = np.random.RandomState(4)
    alpha = rng.dirichlet(np.ones(M), B)
    mean = rng.uniform(-1.5, 1.5, (B, M, A))
    sigma = np.exp(rng.uniform(-3.0, 0.5, (B, M, A)))
    chosen = mean[np.arange(B)[:, None], rng.randint(0, M, (B, k))] + rng.standard_normal((B, k, A)) * 0.5
    if B > 1:
        sigma[0] = np.exp(-20.0)                                                         # row 0: density above 1e30 when on the mean
        chosen[0] = mean[0, 0]
    t = [torch.tensor(np.repeat(v, k, axis=0), dtype=torch.float64, requires_grad=True) for v in (alpha, mean, sigma)]
    loss = R.lossfunc(t[0], t[2], t[1], torch.tensor(chosen.reshape(B * k, A), dtype=torch.float64))
    g = [v.numpy().reshape((B, k) + v.shape[1:]).sum(axis=1) for v in torch.autograd.grad(loss, t)]
    mine = W.seeds_float64(alpha, mean, sigma, chosen)
    assert abs(mine[0] - loss.item()) <= 1e-12 * max(1.0, abs(loss.item()))
    for name, got, want in zip(("alpha", "mean", "sigma"), mine[1:], g):
        e = _rel(got, want)
        print("%s seeds %s: %.3e" % (W.shape_id(dims), name, e))
        assert e < 1e-10, name
    if B > 1 and A * 20 - 0.92 * A > 69.1:                                               # A >= 4: row 0 is clipped
        assert not np.any(mine[2][0]) and not np.any(mine[3][0]) and not np.any(g[1][0])


def test_expert_and_actor_steps_leave_each_others_tensors_untouched():
    dims, B = W.SHAPES[1]
    rng = np.random.RandomState(SEEDS[(dims, B)])
    theta = W.theta_for_tests(dims, 3)
    o = W.oracle(dims, theta)
    b = W.batch(rng, dims, B)
    u, eps = W.draws(rng, dims, B)
    stopped = __import__("copy").deepcopy(o)
    stopped.update(*b, None, None, stop_after_expert=True)
    taps = o.update(*b, u, eps, taps=True)
    for name, (off, shp) in o.layout.items():
        sl = slice(off, off + int(np.prod(shp)))
        before, mid, after = theta[sl], stopped.theta[sl].numpy(), o.theta[sl].numpy()
        if name in R.ACTOR_ONLY:
            assert np.array_equal(mid, before) and not np.array_equal(after, mid), name
            assert not np.any(taps["grads_e"][sl]) and not o.m_c[sl].any() and not o.v_c[sl].any(), name
        elif name in R.EXPERT_ONLY:
            assert not np.array_equal(mid, before) and np.array_equal(after, mid), name
            assert not np.any(taps["grads_a"][sl]) and not o.m_a[sl].any() and not o.v_a[sl].any(), name
        else:                                                                            # W1, b1: both
            assert not np.array_equal(mid, before) and not np.array_equal(after, mid), name
            assert o.m_a[sl].any() and o.m_c[sl].any(), name


def _config(seed=0, **over):
    from rlcontrol_amd.environments.environments import create_environment
    from rlcontrol_amd.utils.config import Config
    env = create_environment({"environment": "Pendulum-v0", "TotalMilSteps": 0.001, "EpisodeSteps": -1,
                              "EvalIntervalMilSteps": 0.0005, "EvalEpisodes": 2})
    cfg = Config()
    cfg.merge_config({"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min,
                      "state_max": env.state_max, "action_dim": env.action_dim, "action_min": env.action_min,
                      "action_max": env.action_max})
    cfg.merge_config(dict({"norm_type": "input_norm", "exploration_policy": "none", "shared_l1_dim": 200, "actor_l2_dim": 200,
                           "expert_l2_dim": 200, "actor_lr": 0.001, "expert_lr": 0.01, "rho": 0.05, "num_samples": 120,
                           "num_modal": 1, "use_uniform_sampling": "False", "use_better_q_gd": "False",
                           "sarsa_update": "True", "sample_for_eval": "False", "use_true_q": "False", "batch_size": 32,
                           "buffer_size": 5000, "writer": None, "replay_sampler": "reference"}, **over))
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": seed})
    return cfg, env


def test_create_agent_reaches_the_constructor_and_fails_loudly_without_a_gpu(hip_lib):
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.utils.main_utils import _AGENTS, create_agent
    assert _AGENTS["ActorExpert"] == ("rlcontrol_amd.agents.ActorExpert", "ActorExpert")
    cfg, _ = _config()
    if torch.cuda.is_available():
        agent = create_agent("ActorExpert", cfg)                                # no SystemExit(0): the agent is known
        assert agent.network_manager.population.P == 82204 and agent.network_manager.top_k == 6
        agent.network_manager.population.close()
    else:
        with pytest.raises(RlcError):
            create_agent("ActorExpert", cfg)
    with pytest.raises(ValueError, match="norm_type 'layer' is not implemented"):
        create_agent("ActorExpert", _config(norm_type="layer")[0])
    for key in ("use_true_q", "use_better_q_gd", "use_uniform_sampling"):
        with pytest.raises(NotImplementedError, match=key):
            create_agent("ActorExpert", _config(**{key: "True"})[0])
    with pytest.raises(ValueError, match="any-shape kernel only"):
        create_agent("ActorExpert", _config(hip_kernel="mfma")[0])


def test_abi_exports_every_ae_symbol(hip_lib):
    from rlcontrol_amd import _lib
    want = ["rlc_ae_" + n for n in ("create", "param_count", "set_blob", "get_blob", "set_beta_powers", "get_beta_powers",
                                    "init_target", "act", "act_queue", "act_fetch", "update", "update_batch", "last_tap",
                                    "enable_grad_taps", "qval", "set_kernel", "get_kernel", "set_split")]
    assert [n for n in _lib.EXPORTS if n.startswith("rlc_ae_")] == want
    with open(os.path.join(ROOT, "include", "rlcontrol_hip.h")) as f:
        header = f.read()
    for name in want:
        assert hasattr(hip_lib, name), name
        assert ("int %s(" % name) in header, name


def test_device_rollout_refuses_the_agent_by_name(tmp_path):
    import main as drv
    with pytest.raises(RuntimeError, match=r"--device_rollout is built for .*\(got 'ActorExpert'\)"):
        drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Pendulum-v0.json"),
                  "--agent_json", os.path.join(ROOT, "jsonfiles", "agent", "ae.json"),
                  "--indices", "0", "1", "1", "--save_dir", str(tmp_path), "--device_rollout", "--quiet"])
    assert not os.listdir(str(tmp_path))                                        # nothing ran, nothing was written
