"""GPU tests of the Bimodal toy environments in the on-device experiment loop, through the C ABI.

  * the device arithmetic (csrc/rollout_env.h: bimodal1d_*, bimodal2d_*) against the reference's own recorded steps
    (tests/golden/bimodal_envs.json), with the recorded actions forced onto the device;
  * the loop against the CPU restatement (tests/helpers/bimodal_rollout.py) on the same Philox streams, shaped like
    tests/test_gpu_rollout.py::test_rollout_matches_cpu_restatement and with its tolerances (2e-6 before the first
    update, 2e-3 after, exact bookkeeping), for all five agents and both kernel families where the shape allows;
  * main.py --device_rollout on Bimodal1DEnv.json.

Reward tolerance.  The device computes the reward in float64 in the reference's expression order, contraction off;
the only difference to the host is the device's `exp` against libm's.  Measured on an MI355X over all 1393 recorded
1-D steps (7 variants x 199 actions, the recorded float32 actions reproduced exactly on the device): worst relative
difference REWARD_REL_MEASURED; the tests assert at 4 x that.  Bimodal2DEnv's reward is
125 * mixture - 2, so the same relative error of `exp` appears relative to reward + 2.
"""
import json
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REWARD_REL_MEASURED = 1.98e-16
REWARD_RTOL = 4 * REWARD_REL_MEASURED

SMIN1, SMAX1, AMIN1, AMAX1 = [-2.0], [2.0], [-2.0], [2.0]
SMIN2, SMAX2, AMIN2, AMAX2 = [-6.0, -6.0], [6.0, 6.0], [-1.0, -1.0], [1.0, 1.0]


def gold():
    with open(os.path.join(ROOT, "tests", "golden", "bimodal_envs.json")) as f:
        return json.load(f)["envs"]


def env_json(name, total, limit, interval, episodes):
    return {"environment": name, "TotalMilSteps": total / 1e6, "EpisodeSteps": limit,
            "EvalIntervalMilSteps": interval / 1e6, "EvalEpisodes": episodes}


def rel_diff(got, want):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))


# ---------------------------------------------------------------------------------------------------
# environment arithmetic
# ---------------------------------------------------------------------------------------------------
def _forced_ddpg(S, A, magnitudes, signs, smin, smax):
    """A DDPG population whose agents act exactly sign * magnitude: zero weights, an output bias of +-20 (tanh is
    exactly +-1 in float32), action_max = magnitude, no OU noise, no learning."""
    from rlcontrol_amd.hip_ddpg import DDPGPopulation, param_layout
    mags = [float(m) for m in magnitudes]
    n = len(signs)
    pop = DDPGPopulation(n, S, A, 16, 16, 16, 4, 64, 0.01, smin, smax, [-m for m in mags], mags, 0.0, 0.0,
                         seeds=list(range(1, n + 1)), ou_sigma=0.0, ou_mu=0.0)
    pop.set_kernel("generic")
    layout, P = param_layout(S, A, 16, 16, 16, "input_norm", False)
    for i, sg in enumerate(signs):
        th = np.zeros(P, np.float32)
        off = layout["ba3"][0]
        th[off:off + A] = 20.0 * np.asarray(sg, np.float32)
        pop.set_params(i, th, init_target=True)
    return pop


def measure_1d_rewards_on_the_fixture(names=None):
    """worst relative difference device reward vs the reference's recorded reward over the recorded actions, each
    reproduced exactly on the device; also checks s' and gamma exactly.  Returns {name: worst}."""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    out = {}
    for name, rec in gold().items():
        if name == "Bimodal2DEnv" or (names is not None and name not in names):
            continue
        want = {s[0]: s for s in rec["steps"]}
        worst = 0.0
        for mag in sorted(set(abs(a) for a in want)):
            pop = _forced_ddpg(1, 1, [mag], [[1.0], [-1.0]], SMIN1, SMAX1)
            DeviceExperiment(pop, env_json(name, 3, 1, 3, 1), warmup_steps=1000).run()
            for agent, sign in ((0, 1.0), (1, -1.0)):
                assert pop.replay_size(agent) == 3
                s, a, r, s2, g = pop.replay_gather(agent, np.arange(3))
                act, s2w, rw, done = want[sign * mag if mag else 0.0]
                assert np.all(a == act) and np.all(s == 0.0) and np.all(g == 0.0)
                assert np.all(s2[:, 0] == np.float32(s2w[0]))
                worst = max(worst, rel_diff(r, [rw] * 3))
            pop.close()
        out[name] = worst
    return out


def test_1d_rewards_on_the_recorded_actions(hip_lib):
    worst = measure_1d_rewards_on_the_fixture()
    for name, w in sorted(worst.items()):
        print("device reward vs the reference's recorded reward, %s: worst relative difference %.3e" % (name, w))
    assert len(worst) == 7 and max(worst.values()) <= REWARD_RTOL, worst


@pytest.mark.parametrize("variant", range(7))
def test_1d_replay_obeys_the_environment(hip_lib, variant):
    """A NAF run with a wide exploration draw (actions all over [-2, 2], both bounds reached): every stored
    (s, a, r, s', gamma) is the environment's function of the stored float32 action; gamma and s' exactly."""
    from helpers.bimodal_rollout import VARIANTS_1D, reward_1d
    from oracle.naf import NafDims, init_params
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_naf import NAFPopulation
    name = VARIANTS_1D[variant][0]
    N, n_agents = 300, 3
    pop = NAFPopulation(n_agents, 1, 1, 32, 32, 16, 1024, 0.01, SMIN1, SMAX1, AMAX1, [1e-3] * n_agents,
                        seeds=[1000 * variant + i for i in range(n_agents)])
    for i in range(n_agents):
        pop.set_params(i, init_params(NafDims(1, 1, 32, 32), 70 + i), init_target=True)
    res = DeviceExperiment(pop, env_json(name, N, -1, 100, 2), noise_scale=4.0).run()
    worst = 0.0
    for agent in range(n_agents):
        tr, er, tl, el, ts, _, _, n_started, tc = res[agent]
        assert tl == [1] * N and tc == list(range(1, N + 1)) and n_started == N and ts == [0, 100, 200, 300]
        assert np.all(np.array(el) == 1) and pop.replay_size(agent) == N
        s, a, r, s2, g = pop.replay_gather(agent, np.arange(N))
        assert np.all(g == 0.0) and np.all(s == 0.0) and np.array_equal(s2, a)
        assert a.min() == -2.0 and a.max() == 2.0 and len(np.unique(a)) > N // 2
        want = np.array([reward_1d(name, float(x)) for x in a[:, 0]])
        worst = max(worst, rel_diff(r, want))
        assert np.array_equal(np.array(tr), r)                         # one-step episodes: the return is the reward
    print("%s: worst relative reward difference over %d stored actions %.3e" % (name, n_agents * N, worst))
    assert worst <= REWARD_RTOL
    pop.close()


def test_2d_recorded_trajectories_on_the_device(hip_lib):
    """the four recorded constant-action trajectories (into each goal, obliquely into a goal, into the wall), forced
    onto the device: s' after the float32 cast and `done` exactly, the reward to the tolerance of the module docstring"""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    traj = gold()["Bimodal2DEnv"]["trajectories"]
    for tname in ("into_upper_goal", "into_lower_goal", "oblique_into_lower_goal", "into_the_wall"):
        steps = traj[tname]
        act = np.array(steps[0][0])
        assert all(st[0] == steps[0][0] for st in steps)
        n, ends = len(steps), steps[-1][3]
        limit = n + 2 if ends else n                       # a goal run ends by `done`, the wall run by the limit
        pop = _forced_ddpg(2, 2, np.abs(act), [np.sign(act)], SMIN2, SMAX2)
        exp = DeviceExperiment(pop, env_json("Bimodal2DEnv", n, limit, n, 0), gamma=0.9, warmup_steps=1000)
        res = exp.run()
        tr, er, tl, el, ts, _, _, n_started, tc = res[0]
        assert tl == [n] and tc == [n] and pop.replay_size(0) == n
        s, a, r, s2, g = pop.replay_gather(0, np.arange(n))
        assert np.all(a == act)
        assert np.array_equal(s2, np.array([st[1] for st in steps]).astype(np.float32))
        assert np.array_equal(s[1:], s2[:-1]) and np.all(s[0] == 0.0)
        assert g.tolist() == [0.9] * (n - 1) + [0.0 if ends else 0.9]
        want = np.array([st[2] for st in steps])
        assert np.all(np.abs(r - want) <= REWARD_RTOL * (want + 2.0)), (tname, r - want)
        assert abs(tr[0] - want.sum()) <= n * REWARD_RTOL * 2.0
        pop.close()


# ---------------------------------------------------------------------------------------------------
# rollout against the CPU restatement
# ---------------------------------------------------------------------------------------------------
def _replay_arrays(orc):
    return [np.array([t[i] for t in orc.replay]) for i in range(5)]


def _check_1d(pop, exp, res, oracles, total, B, evals, atol_pre=2e-6, atol=2e-3):
    for a, orc in enumerate(oracles):
        tr, er, tl, el, ts, _, _, n_started, tc = res[a]
        # --- exact bookkeeping (rule 1: every one-step episode is stored with gamma 0)
        assert orc.rule_counts == {1: total, 2: 0, 3: 0, 4: 0}
        assert tl == orc.train_len == [1] * total and tc == orc.train_cum == list(range(1, total + 1))
        assert ts == orc.timesteps_at_eval == evals and el == orc.eval_len and n_started == orc.n_started == total
        assert pop.replay_size(a) == len(orc.replay) == total
        obs, ep_step = exp.observation(a)
        assert ep_step == orc.last_step == 1
        s, act, r, s2, g = pop.replay_gather(a, np.arange(total))
        os_, oa, orr, os2, og = _replay_arrays(orc)
        assert np.array_equal(g, og) and np.all(g == 0.0) and np.array_equal(s, os_) and np.all(s == 0.0)
        pre = B + 1
        assert np.allclose(act[:pre], oa[:pre], atol=atol_pre) and np.allclose(s2[:pre], os2[:pre], atol=atol_pre)
        assert np.allclose(act, oa, atol=atol) and np.allclose(s2, os2, atol=atol) and np.allclose(obs, orc.last_obs, atol=atol)
        assert np.allclose(er[0], orc.eval_ret[0], rtol=1e-5, atol=1e-4)      # evaluation 0: initial weights
        # the reward has slope up to 1.5 / (0.1 sqrt(e)) ~ 9 per unit of action: the action tolerance times 10
        assert np.allclose(r, orr, atol=10 * atol) and np.allclose(er, orc.eval_ret, atol=10 * atol)
        assert np.allclose(tr, orc.train_ret, atol=10 * atol)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_ddpg_bimodal1d_matches_cpu_restatement(hip_lib, kernel):
    from helpers.bimodal_rollout import BimodalRolloutOracle
    from oracle.ddpg import Dims
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_ddpg import DDPGPopulation, init_params
    dims, B, total = (1, 1, 32, 32, 32), 16, 110
    seeds, lr_a, lr_c = [11, 7777777777], [1e-3, 5e-4], [1e-2, 2e-3]
    pop = DDPGPopulation(2, *dims, B, 4096, 0.01, SMIN1, SMAX1, AMIN1, AMAX1, lr_a, lr_c, seeds=seeds)
    pop.set_kernel(kernel)                                 # S = 1 is an MFMA shape (rlc_mfma_supported): no skip
    thetas = [init_params(*dims, 100 + i) for i in range(2)]
    for i, th in enumerate(thetas):
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, env_json("Bimodal1DEnv", total, 1, 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(60) == 60                           # two calls: the schedule must survive the split
    exp.advance(1000)
    assert exp.total_steps == total
    oracles = [BimodalRolloutOracle(Dims(*dims), thetas[a], lr_a[a], lr_c[a], 0.01, SMIN1, SMAX1, AMIN1, AMAX1, seeds[a],
                                    B, 4096, 0.99, 0, 1, total, 40, 2).use_env("Bimodal1DEnv").run() for a in range(2)]
    _check_1d(pop, exp, exp.results(), oracles, total, B, [0, 40, 80])
    for a, orc in enumerate(oracles):
        th = pop.get_blob(a, "theta")
        assert np.max(np.abs(th - orc.net.theta)) < 2e-3 * np.max(np.abs(orc.net.theta))
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_sac_bimodal1d_matches_cpu_restatement(hip_lib, kernel):
    from helpers.bimodal_rollout import BimodalSacRolloutOracle
    from oracle.sac import SacDims, init_params
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_sac import SACPopulation
    name, dims, B, total = "Bimodal1DEnv_uneq_var1", (1, 1, 32, 32, 32, 32), 16, 90
    seeds, pi_lr, qv_lr, alpha = [21, 99999999999], [1e-3, 5e-4], [1e-3, 2e-3], [0.2, 0.05]
    pop = SACPopulation(2, *dims, B, 4096, 0.01, -2.0, 2.0, 2.0, pi_lr, qv_lr, alpha, seeds=seeds)
    pop.set_kernel(kernel)
    d = SacDims(*dims)
    thetas = []
    for i in range(2):
        th = init_params(d, 300 + i)
        off, shp = d.layout()[0]["pWs"]
        th[off:off + int(np.prod(shp))] *= 0.02          # well-conditioned log-std head (tests/test_sac.py)
        thetas.append(th)
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, env_json(name, total, -1, 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(37) == 37
    exp.advance(1000)
    oracles = [BimodalSacRolloutOracle(d, thetas[a], pi_lr[a], qv_lr[a], alpha[a], 0.01, -2.0, 2.0, 2.0, seeds[a], B, 4096,
                                       0.99, 0, 1, total, 40, 2).use_env(name).run() for a in range(2)]
    _check_1d(pop, exp, exp.results(), oracles, total, B, [0, 40, 80], atol_pre=5e-6, atol=5e-3)
    for a, orc in enumerate(oracles):
        assert np.max(np.abs(pop.get_blob(a, "theta") - orc.net.theta)) < 5e-3 * np.max(np.abs(orc.net.theta))
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_naf_bimodal1d_matches_cpu_restatement(hip_lib, kernel):
    from helpers.bimodal_rollout import BimodalNafRolloutOracle
    from oracle.naf import NafDims, init_params
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_naf import NAFPopulation
    name, dims, B, total, noise = "Bimodal1DEnv_eq_var2", (1, 1, 32, 32), 16, 90, 0.3
    seeds, lr = [8, 123456789012], [1e-3, 3e-4]
    pop = NAFPopulation(2, *dims, B, 4096, 0.01, SMIN1, SMAX1, AMAX1, lr, seeds=seeds)
    pop.set_kernel(kernel)
    d = NafDims(*dims)
    thetas = [init_params(d, 40 + i) for i in range(2)]
    for i in range(2):
        pop.set_params(i, thetas[i], init_target=True)
    exp = DeviceExperiment(pop, env_json(name, total, 1, 40, 2), gamma=0.99, warmup_steps=0, noise_scale=noise)
    exp.advance(50)
    exp.advance(1000)
    oracles = [BimodalNafRolloutOracle(d, thetas[a], lr[a], 0.01, SMIN1, SMAX1, AMAX1, noise, seeds[a], B, 4096, 0.99, 0, 1,
                                       total, 40, 2).use_env(name).run() for a in range(2)]
    _check_1d(pop, exp, exp.results(), oracles, total, B, [0, 40, 80], atol_pre=1e-5, atol=5e-3)
    for a, orc in enumerate(oracles):
        assert np.max(np.abs(pop.get_blob(a, "theta") - orc.net.theta)) < 5e-3 * np.max(np.abs(orc.net.theta))
    pop.close()


@pytest.mark.parametrize("kind,kernel,name", [("reverse", "mfma", "Bimodal1DEnv"), ("reverse", "generic", "Bimodal1DEnv"),
                                              ("forward", "mfma", "Bimodal1DEnv_eq_var3"),
                                              ("forward", "generic", "Bimodal1DEnv_uneq_var2")])
def test_kl_bimodal1d_matches_cpu_restatement(hip_lib, kind, kernel, name):
    from helpers.bimodal_rollout import BimodalKlRolloutOracle
    from oracle.kl_torch import KlDims, init_params
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_kl import KLPopulation
    dims, B, n_param, total = (1, 1, 32, 32, 32, 32), 16, 18, 90
    seeds, pi_lr, qv_lr, alpha = [21, 99999999999], [1e-3, 5e-4], [1e-3, 2e-3], [0.2, 0.05]
    pop = KLPopulation(kind, 2, *dims, B, 4096, 0.01, 2.0, pi_lr, qv_lr, alpha, seeds=seeds, n_param=n_param)
    pop.set_kernel(kernel)
    d = KlDims(*dims)
    thetas = [init_params(d, 300 + i) for i in range(2)]
    for i in range(2):
        pop.set_params(i, thetas[i], init_target=True)
    exp = DeviceExperiment(pop, env_json(name, total, 1, 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(37) == 37
    exp.advance(1000)
    oracles = [BimodalKlRolloutOracle(kind, d, thetas[a], pi_lr[a], qv_lr[a], alpha[a], 0.01, 2.0, n_param, seeds[a], B,
                                      4096, 0.99, 0, 1, total, 40, 2).use_env(name).run() for a in range(2)]
    _check_1d(pop, exp, exp.results(), oracles, total, B, [0, 40, 80], atol_pre=5e-6, atol=5e-3)
    for a, orc in enumerate(oracles):
        assert pop.get_step(a) == orc.net.step == orc.n_updates
        want = orc.net.theta.numpy()
        assert np.max(np.abs(pop.get_blob(a, "theta") - want)) < 5e-3 * np.max(np.abs(want))
    pop.close()


# ---- Bimodal2DEnv: rules 2, 3 and 4 -------------------------------------------------------------------
# Initial weights and the step limit are pinned so that the CPU restatement meets every rule (checked on the CPU when
# the cases were chosen; asserted below): an output bias that heads for the upper goal at nearly full stride reaches it
# at step 4 (rule 2) or 5 (rule 4, the limit) depending on the exploration draw, and misses it once learning has moved
# the policy (rule 3).  The seeds keep every visited state at least 0.05 (squared distance) off the goal radius, far
# beyond the trajectory tolerance, so device and restatement agree on every `done`.
DDPG_2D = dict(dims=(2, 2, 32, 32, 32), B=16, total=110, limit=5, seeds=[31, 7777777777], lr_a=1e-3, lr_c=1e-2, bias=1.5)
SAC_2D = dict(dims=(2, 2, 32, 32, 32, 32), B=16, total=90, limit=5, seeds=[21, 99999999999], pi_lr=1e-3, qv_lr=1e-3,
              alpha=0.2, mean_bias=2.0, log_std_bias=-1.0)


def ddpg_2d_thetas():
    from oracle.ddpg import Dims, init_params
    d = Dims(*DDPG_2D["dims"])
    out = []
    for i in range(2):
        th = init_params(d, 100)
        off = d.layout()[0]["ba3"][0]
        th[off:off + 2] = DDPG_2D["bias"]
        out.append(th)
    return d, out


def ddpg_2d_oracle(a):
    from helpers.bimodal_rollout import BimodalRolloutOracle
    c = DDPG_2D
    d, thetas = ddpg_2d_thetas()
    return BimodalRolloutOracle(d, thetas[a], c["lr_a"], c["lr_c"], 0.01, SMIN2, SMAX2, AMIN2, AMAX2, c["seeds"][a], c["B"],
                                4096, 0.99, 0, c["limit"], c["total"], 40, 2).use_env("Bimodal2DEnv").run()


def sac_2d_thetas():
    from oracle.sac import SacDims, init_params
    d = SacDims(*SAC_2D["dims"])
    lay = d.layout()[0]
    out = []
    for i in range(2):
        th = init_params(d, 300)
        off, shp = lay["pWs"]
        th[off:off + int(np.prod(shp))] *= 0.02
        th[lay["pbm"][0]:lay["pbm"][0] + 2] = SAC_2D["mean_bias"]
        th[lay["pbs"][0]:lay["pbs"][0] + 2] = SAC_2D["log_std_bias"]
        out.append(th)
    return d, out


def sac_2d_oracle(a):
    from helpers.bimodal_rollout import BimodalSacRolloutOracle
    c = SAC_2D
    d, thetas = sac_2d_thetas()
    return BimodalSacRolloutOracle(d, thetas[a], c["pi_lr"], c["qv_lr"], c["alpha"], 0.01, -6.0, 6.0, 1.0, c["seeds"][a],
                                   c["B"], 4096, 0.99, 0, c["limit"], c["total"], 40, 2).use_env("Bimodal2DEnv").run()


def _check_2d(pop, exp, res, oracles, total, B, atol_pre, atol):
    for a, orc in enumerate(oracles):
        n2, n3, n4 = orc.rule_counts[2], orc.rule_counts[3], orc.rule_counts[4]
        assert n2 >= 1 and n3 >= 1 and n4 >= 1 and orc.rule_counts[1] == 0, orc.rule_counts
        tr, er, tl, el, ts, _, _, n_started, tc = res[a]
        assert tl == orc.train_len and tc == orc.train_cum and len(tl) == n2 + n3 + n4
        assert ts == orc.timesteps_at_eval == [0, 40, 80] and el == orc.eval_len and n_started == orc.n_started
        assert pop.replay_size(a) == len(orc.replay) == total - n4                 # rule 4: not stored
        obs, ep_step = exp.observation(a)
        assert ep_step == orc.last_step
        s, act, r, s2, g = pop.replay_gather(a, np.arange(total - n4))
        os_, oa, orr, os2, og = _replay_arrays(orc)
        assert np.array_equal(g, og) and int(np.sum(g == 0.0)) == n2               # rule 2: gamma 0; rule 3: gamma
        pre = B + 1
        assert np.allclose(s[:pre], os_[:pre], atol=atol_pre) and np.allclose(act[:pre], oa[:pre], atol=atol_pre)
        assert np.allclose(r[:pre], orr[:pre], atol=1e-5) and np.allclose(s2[:pre], os2[:pre], atol=atol_pre)
        # after the first update: the walk adds up to `limit` actions, each within the action tolerance
        assert np.allclose(act, oa, atol=atol) and np.allclose(s, os_, atol=5 * atol) and np.allclose(s2, os2, atol=5 * atol)
        assert np.allclose(r, orr, atol=5 * atol) and np.allclose(obs, orc.last_obs, atol=5 * atol)
        assert np.allclose(tr, orc.train_ret, atol=25 * atol)
        assert np.allclose(er[0], orc.eval_ret[0], rtol=1e-5, atol=1e-4)      # evaluation 0: initial weights
        assert np.allclose(er, orc.eval_ret, atol=25 * atol)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_ddpg_bimodal2d_matches_cpu_restatement(hip_lib, kernel):
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    c = DDPG_2D
    pop = DDPGPopulation(2, *c["dims"], c["B"], 4096, 0.01, SMIN2, SMAX2, AMIN2, AMAX2, c["lr_a"], c["lr_c"], seeds=c["seeds"])
    pop.set_kernel(kernel)
    for i, th in enumerate(ddpg_2d_thetas()[1]):
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, env_json("Bimodal2DEnv", c["total"], c["limit"], 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(60) == 60
    exp.advance(1000)
    assert exp.total_steps == c["total"]
    oracles = [ddpg_2d_oracle(a) for a in range(2)]
    _check_2d(pop, exp, exp.results(), oracles, c["total"], c["B"], 2e-6, 2e-3)
    for a, orc in enumerate(oracles):
        assert np.max(np.abs(pop.get_blob(a, "theta") - orc.net.theta)) < 2e-3 * np.max(np.abs(orc.net.theta))
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)      # same number of Adam steps
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_sac_bimodal2d_matches_cpu_restatement(hip_lib, kernel):
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_sac import SACPopulation
    c = SAC_2D
    pop = SACPopulation(2, *c["dims"], c["B"], 4096, 0.01, -6.0, 6.0, 1.0, c["pi_lr"], c["qv_lr"], c["alpha"], seeds=c["seeds"])
    pop.set_kernel(kernel)
    for i, th in enumerate(sac_2d_thetas()[1]):
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, env_json("Bimodal2DEnv", c["total"], c["limit"], 40, 2), gamma=0.99, warmup_steps=0)
    assert exp.advance(37) == 37
    exp.advance(1000)
    oracles = [sac_2d_oracle(a) for a in range(2)]
    _check_2d(pop, exp, exp.results(), oracles, c["total"], c["B"], 5e-6, 5e-3)
    for a, orc in enumerate(oracles):
        assert np.max(np.abs(pop.get_blob(a, "theta") - orc.net.theta)) < 5e-3 * np.max(np.abs(orc.net.theta))
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)
    pop.close()


def test_rollout_create_names_the_environment(hip_lib):
    """a population of the wrong shape is refused with the environment's name; an unknown id is refused"""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    pop = DDPGPopulation(1, 3, 1, 16, 16, 16, 4, 64, 0.01, [-1, -1, -8], [1, 1, 8], [-2.0], [2.0], 1e-3, 1e-2, seeds=[1])
    with pytest.raises(Exception, match="Bimodal1DEnv family needs state_dim 1 / action_dim 1"):
        DeviceExperiment(pop, env_json("Bimodal1DEnv_eq_var1", 10, 1, 5, 1))
    with pytest.raises(Exception, match="Bimodal2DEnv needs state_dim 2 / action_dim 2"):
        DeviceExperiment(pop, env_json("Bimodal2DEnv", 10, 5, 5, 1))
    DeviceExperiment(pop, env_json("Pendulum-v0", 10, 5, 5, 1)).run()
    pop.close()


# ---------------------------------------------------------------------------------------------------
# main.py --device_rollout on the shipped Bimodal1DEnv.json
# ---------------------------------------------------------------------------------------------------
RUN_KEYS = {"random_seed", "total_timesteps", "eval_interval_timesteps", "episodes_per_eval", "eval_episode_rewards",
            "eval_episode_steps", "timesteps_at_eval", "train_episode_steps", "train_episode_rewards",
            "total_train_episodes", "eval_time", "train_time"}


def _check_bimodal1d_pickle(path):
    import pickle
    with open(path, "rb") as f:
        data = pickle.load(f)
    assert data["experiment"]["environment"]["env_name"] == "Bimodal1DEnv"
    assert sorted(data["experiment_data"]) == [0, 1]
    assert [r["random_seed"] for r in data["experiment_data"][0]["runs"]] == [0, 1, 2]     # indices 0, 2, 4
    assert [r["random_seed"] for r in data["experiment_data"][1]["runs"]] == [0, 1]        # indices 1, 3
    for sweep in (0, 1):
        for run in data["experiment_data"][sweep]["runs"]:
            assert set(run) == RUN_KEYS
            assert run["total_timesteps"] == 750 and run["eval_interval_timesteps"] == 5 and run["episodes_per_eval"] == 10
            assert run["eval_episode_rewards"].shape == (151, 10) and run["eval_episode_rewards"].dtype == np.float64
            assert run["eval_episode_steps"].shape == (151, 10) and np.all(run["eval_episode_steps"] == 1)
            assert run["timesteps_at_eval"].tolist() == list(range(0, 751, 5))
            assert run["train_episode_steps"].tolist() == [1] * 750 and run["total_train_episodes"] == 750
            assert run["train_episode_rewards"].shape == (750,) and np.isfinite(run["train_episode_rewards"]).all()
            # the reward of Bimodal1DEnv lies in (0, 1.5]; greedy evaluation episodes of one evaluation are identical
            assert np.all(run["eval_episode_rewards"] >= 0.0) and np.all(run["eval_episode_rewards"] <= 1.5 + 1e-9)
            assert np.all(run["eval_episode_rewards"] == run["eval_episode_rewards"][:, :1])
    return data


def test_main_device_rollout_bimodal1d_ddpg_pickle(hip_lib, tmp_path):
    import main as drv
    agent = {"agent": "DDPG", "sweeps": {"shared_l1_dim": [32], "actor_l2_dim": [32], "critic_l2_dim": [32],
                                         "actor_lr": [1e-3, 1e-4], "critic_lr": [1e-2], "norm_type": ["input_norm"],
                                         "exploration_policy": ["ou_noise"], "batch_size": [16],
                                         "buffer_size": [1000]}}
    aj = tmp_path / "ddpg.json"
    aj.write_text(json.dumps(agent))
    drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json"), "--agent_json", str(aj),
              "--indices", "0", "1", "5", "--save_dir", str(tmp_path), "--device_rollout", "--quiet"])
    data = _check_bimodal1d_pickle(tmp_path / "Bimodal1DEnv_ddpgresults" / "data_0_1_5.pkl")
    assert data["experiment_data"][1]["agent_params"]["actor_lr"] == 1e-4


@pytest.mark.parametrize("mode", [["--device_rollout"], []], ids=["device_loop", "host_loop"])
def test_main_bimodal1d_reverse_kl_pickle(hip_lib, tmp_path, mode):
    """the same pickle from the device loop and from the host loop (host environment, drop-in agent)"""
    import main as drv
    agent = {"agent": "ReverseKL",
             "sweeps": {"norm_type": ["input_norm"], "exploration_policy": ["none"], "actor_l1_dim": [32],
                        "actor_l2_dim": [32], "critic_l1_dim": [32], "critic_l2_dim": [32], "pi_lr": [1e-3],
                        "qf_vf_lr": [1e-3], "sample_for_eval": ["False"], "use_true_q": ["False"],
                        "entropy_scale": [0.1, 0.01], "l_param": [6], "N_param": [16], "optim_type": ["intg"],
                        "q_update_type": ["non_sac"], "batch_size": [16], "buffer_size": [1000]}}
    aj = tmp_path / "reverse_kl.json"
    aj.write_text(json.dumps(agent))
    drv.main(["--env_json", os.path.join(ROOT, "jsonfiles", "environment", "Bimodal1DEnv.json"), "--agent_json", str(aj),
              "--indices", "0", "1", "5", "--save_dir", str(tmp_path), "--quiet"] + mode)
    data = _check_bimodal1d_pickle(tmp_path / "Bimodal1DEnv_reverse_klresults" / "data_0_1_5.pkl")
    assert data["experiment_data"][1]["agent_params"]["entropy_scale"] == 0.01
