"""WireFitting on the CPU: the parameter layout, the torch restatement (tests/torch_ref_wf.py) against its float64 twin,
the interpolation's gradient against finite differences and against the closed-form seeds the kernel uses (float64), the
shipped json, and the loud failure of the agent without a GPU.

Parity unpinned: no reference fixture exercises this agent."""
import json
import os

import numpy as np
import pytest
import torch

import torch_ref_wf as R
import wf_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def test_param_layout_order_and_count():
    from rlcontrol_amd.hip_wf import init_params, param_layout
    lay, P = param_layout(3, 1, 200, 200, 100)
    assert list(lay) == ["W1", "b1", "W2", "b2", "Wa", "ba", "Wq", "bq", "kappa"]
    assert P == 81300
    assert lay["Wa"] == (600 + 200 + 40000 + 200, (200, 100)) and lay["kappa"] == (81200, (100,))
    for dims in [s for s, _ in W.SHAPES]:
        lay_r, P_r = R.layout(dims)
        lay_p, P_p = param_layout(*dims)
        assert P_r == P_p and list(lay_r.items()) == list(lay_p.items())
        assert np.array_equal(init_params(*dims, seed=4), R.init_params(dims, 4))
    th = init_params(3, 1, 200, 200, 100, 0)
    v = {k: th[o:o + int(np.prod(s))] for k, (o, s) in lay.items()}
    for b in ("b1", "b2", "ba", "bq"):
        assert not v[b].any()                                                   # zero biases
    assert 0.95 * np.sqrt(6.0 / 203) < np.max(np.abs(v["W1"])) <= np.sqrt(6.0 / 203)      # Xavier-uniform
    assert 0.95 * np.sqrt(6.0 / 400) < np.max(np.abs(v["W2"])) <= np.sqrt(6.0 / 400)
    assert 0.99 < np.max(np.abs(v["Wa"])) <= 1.0 and 0.99 < np.max(np.abs(v["Wq"])) <= 1.0
    assert 0.0025 < np.max(np.abs(v["kappa"])) <= 0.003


def test_shipped_json_sweeps_seven_settings():
    from rlcontrol_amd.utils.main_utils import get_sweep_parameters
    with open(os.path.join(ROOT, "jsonfiles", "agent", "wirefitting.json")) as f:
        aj = json.load(f, object_pairs_hook=__import__("collections").OrderedDict)
    assert aj["agent"] == "WireFitting"
    params, total = get_sweep_parameters(aj["sweeps"], 0)
    assert total == 7
    assert dict(params) == {"norm_type": "input_norm", "exploration_policy": "ou_noise", "l1_dim": 200, "l2_dim": 200,
                            "learning_rate": 1, "app_points": 100}
    assert [get_sweep_parameters(aj["sweeps"], i)[0]["learning_rate"] for i in range(7)] == [1, 0.5, 0.1, 0.05, 0.01, 0.005, 0.001]


def _pair(dims, seed):
    theta = R.init_params(dims, seed)
    rng = np.random.RandomState(seed + 100)
    o32, o64 = W.oracle(dims, theta), W.oracle(dims, theta, torch.float64)
    tgt = W.target_apart(theta, rng)
    for o in (o32, o64):
        o.theta_t = o.theta_t * 0 + torch.as_tensor(tgt).to(o.dt)
    return o32, o64, rng


@pytest.mark.parametrize("dims,B", W.SHAPES, ids=W.shape_id)
@pytest.mark.parametrize("hit", [False, True], ids=["generic", "on_a_wire"])
def test_restatement_fp32_agrees_with_its_float64_twin(dims, B, hit):
    """The taps at 1e-5; the gradient tensors at 1e-4 of their largest element at a generic action (the level
    tests/test_optq.py holds its twin to).  With the action on a wire the seed -2 g e (a - ahat) multiplies the ROUNDING
    NOISE of a - ahat (about 1e-7: an ulp of an action near 2) by e <= w |qhat - Q| with w = 1e5 at the 1e-5 floor: an
    error of order 1e5 x 1e-7 = 1e-2 of the seed's scale is fp32 arithmetic, not a bug, and 1e-2 is the bound there."""
    o32, o64, rng = _pair(dims, 1)
    b = W.batch(rng, dims, B)
    if hit:
        b = W.on_a_wire(o32, b)
    W.assert_tie_free(o32, b)
    a32, i32 = o32.act(b[0][:5])
    a64, i64 = o64.act(b[0][:5])
    assert np.array_equal(i32, i64) and _rel(a32, a64) < 1e-5
    assert _rel(o32.qval(b[0], b[1]), o64.qval(b[0], b[1])) < 1e-5
    t32, t64 = o32.update(*b, taps=True), o64.update(*b, taps=True)
    for k in ("q", "y", "max_q"):
        e = _rel(t32[k], t64[k])
        print("%s/B%d tap %s: %.3e" % (dims, B, k, e))
        assert e < 1e-5, k
    gmax = np.max(np.abs(t64["grads"]))
    for n, (off, shp) in o32.layout.items():
        k = int(np.prod(shp))
        if dims[4] == 1 and n in ("Wa", "ba", "kappa"):                         # one wire: Q = qhat_0, these are zero
            assert np.max(np.abs(t32["grads"][off:off + k])) <= 1e-6 * gmax, n
            continue
        e = _rel(t32["grads"][off:off + k], t64["grads"][off:off + k])
        print("%s/B%d gradient %s: %.3e" % (dims, B, n, e))
        assert e < (1e-2 if hit else 1e-4), n


def _interp_inputs(n, N, A, seed, hit):
    rng = np.random.RandomState(seed)
    ahat = np.tanh(rng.uniform(-1.5, 1.5, (n, N, A))) * W.AMAX0
    qhat = rng.uniform(-3, 3, (n, N))
    kappa = rng.uniform(-0.5, 0.5, N)
    a = rng.uniform(-2, 2, (n, A))
    if hit == "argmax":
        a = ahat[np.arange(n), np.argmax(qhat, 1)].copy()
    elif hit == "other":
        a = ahat[np.arange(n), (np.argmax(qhat, 1) + 1) % N].copy()
    return ahat, qhat, a, kappa, rng.uniform(-16, 0, n)


@pytest.mark.parametrize("hit", [None, "argmax", "other"], ids=["generic", "on_the_argmax_wire", "on_another_wire"])
def test_interpolation_gradient_float64(hit):
    """autograd of the restated interpolation against central differences, and against the closed-form seeds the kernel
    writes (wf_cases.seeds_float64), at a generic action and with the action exactly on a wire (distance = the 1e-5 floor
    plus c (M - qhat): the floor alone on the arg-max wire)"""
    n, N, A = 4, 9, 2
    ahat, qhat, a, kappa, y = _interp_inputs(n, N, A, 3, hit)
    t = [torch.tensor(v, dtype=torch.float64, requires_grad=True) for v in (ahat, qhat, kappa)]
    ta, ty = torch.tensor(a, dtype=torch.float64), torch.tensor(y, dtype=torch.float64)
    loss = lambda: torch.mean((ty - R.interpolate(t[0], t[1], ta, t[2])) ** 2)
    g_a, g_q, g_k = [v.numpy() for v in torch.autograd.grad(loss(), t)]
    Q, dq, da, dk = W.seeds_float64(ahat, qhat, a, kappa, y)
    assert _rel(Q, R.interpolate(t[0], t[1], ta, t[2]).detach().numpy()) < 1e-13
    for name, mine, auto in (("qhat", dq, g_q), ("ahat", da, g_a), ("kappa", dk, g_k)):
        e = _rel(mine, auto)
        print("seeds %s (%s): %.3e" % (name, hit, e))
        assert e < 1e-11, name
    # central differences, step 1e-5 (on a wire the distance's length scale is sqrt(1e-5) = 3e-3).  The error is taken
    # against the largest gradient element of the three inputs: with every row on its arg-max wire Q = M to 1e-5 and the
    # gradients with respect to ahat and kappa are themselves 1e-4 and smaller, below the differences' own rounding
    h = 1e-5
    scale = max(float(np.max(np.abs(v))) for v in (g_a, g_q, g_k))
    for name, var, auto in (("qhat", t[1], g_q), ("ahat", t[0], g_a), ("kappa", t[2], g_k)):
        fd = np.zeros(auto.size)
        flat = var.detach().reshape(-1)
        with torch.no_grad():
            for i in range(flat.numel()):
                keep = float(flat[i])
                flat[i] = keep + h; up = float(loss())
                flat[i] = keep - h; dn = float(loss())
                flat[i] = keep
                fd[i] = (up - dn) / (2 * h)
        e = float(np.max(np.abs(fd - auto.ravel()))) / scale
        print("finite differences %s (%s): %.3e of the largest gradient element" % (name, hit, e))
        assert e < 1e-6, name


def _config(seed=0, **over):
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


def test_create_agent_reaches_the_constructor_and_fails_loudly_without_a_gpu(hip_lib):
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.utils.main_utils import _AGENTS, create_agent
    assert _AGENTS["WireFitting"] == ("rlcontrol_amd.agents.WireFitting", "WireFitting")
    cfg, _ = _config()
    if torch.cuda.is_available():
        agent = create_agent("WireFitting", cfg)                                # no SystemExit(0): the agent is known
        assert agent.network_manager.population.P == 81300
        agent.network_manager.population.close()
    else:
        with pytest.raises(RlcError):
            create_agent("WireFitting", cfg)
    with pytest.raises(ValueError, match="norm_type 'layer' is not implemented"):
        create_agent("WireFitting", _config(norm_type="layer")[0])


def test_device_rollout_refuses_the_agent_by_name(tmp_path):
    import main as drv
    with pytest.raises(RuntimeError, match=r"--device_rollout is built for .*\(got 'WireFitting'\)"):
        drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Pendulum-v0.json"),
                  "--agent_json", os.path.join(ROOT, "jsonfiles", "agent", "wirefitting.json"),
                  "--indices", "0", "1", "1", "--save_dir", str(tmp_path), "--device_rollout", "--quiet"])
    assert not os.listdir(str(tmp_path))                                        # nothing ran, nothing was written
