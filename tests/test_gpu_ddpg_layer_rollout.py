"""The layer-norm form of the DDPG MFMA update kernel inside the on-device experiment loop (set_kernel("mfma") on a
norm_type 'layer' population, then DeviceExperiment): the training step at the top of every iteration of the update loop
of rlc_ddpg_update_ln_mfma_kernel, against the loop around oracle/ddpg_variants.py (oracle.rollout.VariantRolloutOracle).

Constants and bounds are those of tests/test_gpu_rollout.py::test_ddpg_variant_rollout_matches_cpu_restatement:
Pendulum-v0 with 25-step episodes, an evaluation of 2 episodes every 40 steps, seeds [11, 7777777777], learning rates
[1e-3, 5e-4] / [1e-2, 2e-3]; exact bookkeeping; replay rows before the first update within 2e-6; afterwards 3e-3 on the
trajectory, 3e-3 relative on theta, rtol 1e-6 on Adam's beta powers; evaluation 0 within rtol 1e-5.  The "generic" legs
run the any-shape kernel: they show that the restatement and the bounds hold at each shape.  Selecting "mfma" is a
requirement: a refusal fails the test."""
import functools

import numpy as np
import pytest

import test_gpu_ddpg_layer_mfma as LM
from oracle.ddpg_variants import VDims

pytestmark = pytest.mark.gpu

SMIN, SMAX, AMIN, AMAX = [-1, -1, -8], [1, 1, 8], [-2.0], [2.0]
SEEDS, LR_A, LR_C = [11, 7777777777], [1e-3, 5e-4], [1e-2, 2e-3]
LIMIT, INTERVAL, EVAL_EPISODES = 25, 40, 2
BLOBS = LM.BLOBS
SMALL = ((3, 1, 32, 24, 40), 17)

# (S, A, H1, HA, HC), batch, total steps:
#   ragged widths with HA != HC and a ragged batch on two tiles;
#   batch 2: the policy scratch of the step is wider than two rows of either image;
#   the shipped json's shape (13 tiles, the split hand-off);
#   seven tiles with the padded last tile, the first update late in the run (the pre-update prefix is batch + 1 rows)
CASES = [((3, 1, 32, 24, 40), 17, 110), ((3, 1, 32, 24, 40), 2, 110), ((3, 1, 200, 200, 200), 32, 110),
         ((3, 1, 64, 72, 48), 100, 130)]


def _env(total, name="Pendulum-v0", limit=LIMIT):
    return {"environment": name, "TotalMilSteps": total / 1e6, "EpisodeSteps": limit,
            "EvalIntervalMilSteps": INTERVAL / 1e6, "EvalEpisodes": EVAL_EPISODES}


@functools.lru_cache(maxsize=None)
def _thetas(dims):
    d = VDims(*dims, norm=True)
    return tuple(LM._theta(d, 100 + i)[0] for i in range(2))       # gamma / beta off 1 / 0


@functools.lru_cache(maxsize=None)
def _oracles(dims, B, total):
    """the CPU restatement of both agents' runs: computed once per shape, read by every test that needs it"""
    from oracle.rollout import VariantRolloutOracle
    d = VDims(*dims, norm=True)
    return tuple(VariantRolloutOracle(d, _thetas(dims)[a], LR_A[a], LR_C[a], 0.01, SMIN, SMAX, AMIN, AMAX, SEEDS[a], B, 4096,
                                      0.99, 0, LIMIT, total, INTERVAL, EVAL_EPISODES).run() for a in range(2))


def _pop(dims, B, kernel, seeds=SEEDS):
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    pop = DDPGPopulation(2, *dims, B, 4096, 0.01, SMIN, SMAX, AMIN, AMAX, LR_A, LR_C, seeds=seeds, norm_type="layer")
    if kernel is not None:
        pop.set_kernel(kernel)                 # no skip: a refusal is a failure
        assert pop.kernel_in_use() == kernel
    for i, th in enumerate(_thetas(dims)):
        pop.set_params(i, th, init_target=True)
    return pop


def _check_against_oracle(pop, exp, dims, B, total, tag):
    n_ep = total // LIMIT                      # every episode ends at the step limit: truncated, not stored
    res = exp.results()
    for a, orc in enumerate(_oracles(dims, B, total)):
        tr, er, tl, el, ts, _, _, n_started, tc = res[a]
        # --- exact bookkeeping
        assert tl == orc.train_len == [LIMIT] * n_ep and tc == orc.train_cum == [LIMIT * (i + 1) for i in range(n_ep)]
        assert ts == orc.timesteps_at_eval == list(range(0, total + 1, INTERVAL)) and el == orc.eval_len
        assert n_started == n_ep + (1 if total % LIMIT else 0)
        n = total - n_ep
        assert pop.replay_size(a) == len(orc.replay) == n
        obs, ep_step = exp.observation(a)
        assert ep_step == orc.last_step == total % LIMIT
        s, act, r, s2, g = pop.replay_gather(a, np.arange(n))
        os_ = np.array([t[0] for t in orc.replay]); oa = np.array([t[1] for t in orc.replay])
        assert np.array_equal(g, np.array([t[4] for t in orc.replay]))
        pre = B + 1                            # no update has touched the weights yet: float rounding only
        e_pre = max(np.max(np.abs(s[:pre] - os_[:pre])), np.max(np.abs(act[:pre] - oa[:pre])))
        e_all = max(np.max(np.abs(s - os_)), np.max(np.abs(act - oa)))
        th = pop.get_blob(a, "theta")
        e_th = np.max(np.abs(th - orc.net.theta)) / np.max(np.abs(orc.net.theta))
        print("%s %s B%d agent %d: rows before the first update %.3e, all rows %.3e, theta rel %.3e" % (
            tag, dims, B, a, e_pre, e_all, e_th))
        assert np.allclose(s[:pre], os_[:pre], atol=2e-6) and np.allclose(act[:pre], oa[:pre], atol=2e-6)
        assert np.allclose(s, os_, atol=3e-3) and np.allclose(act, oa, atol=3e-3)
        assert np.allclose(er[0], orc.eval_ret[0], rtol=1e-5, atol=1e-4)      # evaluation 0: initial weights
        assert np.allclose(er, orc.eval_ret, rtol=3e-3, atol=3e-2)
        assert e_th < 3e-3
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)      # same number of Adam steps
        assert orc.n_updates >= 20                                             # (25 at batch 100 in 130 steps)


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("dims,B,total", CASES)
def test_layer_rollout_matches_cpu_restatement(hip_lib, dims, B, total, kernel):
    from rlcontrol_amd.device_experiment import DeviceExperiment
    pop = _pop(dims, B, kernel)
    exp = DeviceExperiment(pop, _env(total), gamma=0.99, warmup_steps=0)
    assert exp.advance(60) == 60               # two calls: the schedule must survive the split
    exp.advance(1000)
    assert exp.total_steps == total and pop.kernel_in_use() == kernel
    _check_against_oracle(pop, exp, dims, B, total, kernel)
    pop.close()


class _Bimodal2D(object):
    """Bimodal2DEnv with the layer-norm network: action_dim 2, the `_2` units.  Initial weights as
    tests/test_gpu_bimodal.py pins them for the plain network (an output bias heading for the upper goal).  With these
    seeds the CPU restatement meets every episode rule (`done` before the limit, the limit without `done`, `done` at the
    limit) and every visited state stays at least 0.06 (squared distance) off the goal radius, far beyond the
    trajectory tolerance: device and restatement agree on every `done` (checked on the CPU when the seeds were chosen)."""
    dims, B, total, limit, bias = (2, 2, 32, 24, 40), 16, 110, 5, 1.5
    seeds, lr_a, lr_c = [31, 8888888888], 1e-3, 1e-2
    smin, smax, amin, amax = [-6.0, -6.0], [6.0, 6.0], [-1.0, -1.0], [1.0, 1.0]

    @classmethod
    @functools.lru_cache(maxsize=None)
    def thetas(cls):
        d = VDims(*cls.dims, norm=True)
        out = []
        for i in range(2):
            th = LM._theta(d, 100)[0]
            off = d.layout()[0]["ba3"][0]
            th[off:off + 2] = cls.bias
            out.append(th)
        return d, tuple(out)

    @classmethod
    @functools.lru_cache(maxsize=None)
    def oracles(cls):
        from helpers.bimodal_rollout import _BimodalLoop
        from oracle.rollout import VariantRolloutOracle

        class Loop(_BimodalLoop, VariantRolloutOracle):        # composed as the helper composes its own four
            pass
        d, thetas = cls.thetas()
        return tuple(Loop(d, thetas[a], cls.lr_a, cls.lr_c, 0.01, cls.smin, cls.smax, cls.amin, cls.amax, cls.seeds[a],
                          cls.B, 4096, 0.99, 0, cls.limit, cls.total, INTERVAL, EVAL_EPISODES).use_env("Bimodal2DEnv").run()
                     for a in range(2))


def test_layer_rollout_action_dim_2_on_bimodal2d(hip_lib):
    """bounds of tests/test_gpu_bimodal.py::test_ddpg_bimodal2d_matches_cpu_restatement (2e-6 before the first update,
    2e-3 on the actions after it, the walk's and the returns' multiples of that, 2e-3 relative on theta)"""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    c = _Bimodal2D
    pop = DDPGPopulation(2, *c.dims, c.B, 4096, 0.01, c.smin, c.smax, c.amin, c.amax, c.lr_a, c.lr_c, seeds=c.seeds,
                         norm_type="layer")
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    for i, th in enumerate(c.thetas()[1]):
        pop.set_params(i, th, init_target=True)
    exp = DeviceExperiment(pop, _env(c.total, "Bimodal2DEnv", c.limit), gamma=0.99, warmup_steps=0)
    assert exp.advance(60) == 60
    exp.advance(1000)
    assert exp.total_steps == c.total
    res = exp.results()
    atol_pre, atol = 2e-6, 2e-3
    for a, orc in enumerate(c.oracles()):
        n2, n3, n4 = orc.rule_counts[2], orc.rule_counts[3], orc.rule_counts[4]
        assert n2 >= 1 and n3 >= 1 and n4 >= 1 and orc.rule_counts[1] == 0, orc.rule_counts
        tr, er, tl, el, ts, _, _, n_started, tc = res[a]
        assert tl == orc.train_len and tc == orc.train_cum and len(tl) == n2 + n3 + n4
        assert ts == orc.timesteps_at_eval == [0, 40, 80] and el == orc.eval_len and n_started == orc.n_started
        n = c.total - n4                                                           # rule 4: not stored
        assert pop.replay_size(a) == len(orc.replay) == n
        obs, ep_step = exp.observation(a)
        assert ep_step == orc.last_step
        s, act, r, s2, g = pop.replay_gather(a, np.arange(n))
        os_, oa, orr, os2, og = [np.array([t[i] for t in orc.replay]) for i in range(5)]
        assert np.array_equal(g, og) and int(np.sum(g == 0.0)) == n2               # rule 2: gamma 0; rule 3: gamma
        pre = c.B + 1
        print("Bimodal2DEnv agent %d: rules %s, actions before the first update %.3e, all actions %.3e" % (
            a, orc.rule_counts, np.max(np.abs(act[:pre] - oa[:pre])), np.max(np.abs(act - oa))))
        assert np.allclose(s[:pre], os_[:pre], atol=atol_pre) and np.allclose(act[:pre], oa[:pre], atol=atol_pre)
        assert np.allclose(r[:pre], orr[:pre], atol=1e-5) and np.allclose(s2[:pre], os2[:pre], atol=atol_pre)
        assert np.allclose(act, oa, atol=atol) and np.allclose(s, os_, atol=5 * atol) and np.allclose(s2, os2, atol=5 * atol)
        assert np.allclose(r, orr, atol=5 * atol) and np.allclose(obs, orc.last_obs, atol=5 * atol)
        assert np.allclose(tr, orc.train_ret, atol=25 * atol)
        assert np.allclose(er[0], orc.eval_ret[0], rtol=1e-5, atol=1e-4)           # evaluation 0: initial weights
        assert np.allclose(er, orc.eval_ret, atol=25 * atol)
        assert np.max(np.abs(pop.get_blob(a, "theta") - orc.net.theta)) < 2e-3 * np.max(np.abs(orc.net.theta))
        assert np.allclose(pop.get_beta_powers(a), orc.net.pw, rtol=1e-6)
    pop.close()


def _state(pop, exp):
    """everything a run leaves behind: the six blobs, the beta powers, the replay in insertion order, the logs"""
    out = []
    res = exp.results()
    for a in range(pop.n_agents):
        tr, er, tl, el, ts, _, _, n_started, tc = res[a]
        out.append(dict([(w, pop.get_blob(a, w)) for w in BLOBS] + [
            ("pw", np.asarray(pop.get_beta_powers(a))), ("train_ret", np.asarray(tr)), ("eval_ret", np.asarray(er)),
            ("train_len", np.asarray(tl)), ("eval_len", np.asarray(el)), ("train_cum", np.asarray(tc)),
            ("n_started", np.asarray(n_started)), ("obs", exp.observation(a)[0]), ("ep_step", np.asarray(exp.observation(a)[1]))]
            + list(zip(("s", "a", "r", "s2", "g"), pop.replay_gather(a, np.arange(pop.replay_size(a)))))))
    return out


def _assert_same_bits(one, two):
    assert len(one) == len(two)
    for a, (x, y) in enumerate(zip(one, two)):
        assert sorted(x) == sorted(y)
        for k in x:
            assert np.array_equal(x[k], y[k]), (a, k)


def test_layer_rollout_launch_boundaries_change_nothing(hip_lib):
    """one launch per stretch between evaluations against one launch per step: every launch zeroes the images anew, the
    step's scratch must leave nothing behind that the update reads"""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    dims, B = SMALL
    pops = [_pop(dims, B, "mfma") for _ in range(2)]
    exps = [DeviceExperiment(p, _env(110), gamma=0.99, warmup_steps=0) for p in pops]
    exps[0].run(chunk=5000)
    for i in range(110):
        assert exps[1].advance(1) == i + 1
    assert exps[0].total_steps == exps[1].total_steps == 110
    one, two = _state(pops[0], exps[0]), _state(pops[1], exps[1])
    assert not np.array_equal(one[0]["theta"], _thetas(dims)[0])           # learning happened
    _assert_same_bits(one, two)
    for p in pops:
        p.close()


def test_layer_rollout_kernel_is_chosen_before_the_rollout_is_attached(hip_lib):
    """Order of calls.  The device copy of the handle's views (the weight layout among them) is made when the rollout is
    created; a switch to the MFMA kernel afterwards is refused, as it is for the plain form, and leaves the population
    where it was: its run equals, bit for bit, the run of a population that was never asked."""
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_ddpg import DDPGPopulation, init_params
    dims, B = SMALL
    refusal = "cannot change once a rollout is attached"
    plain = DDPGPopulation(1, 3, 1, 32, 32, 32, 16, 256, 0.01, SMIN, SMAX, AMIN, AMAX, 1e-3, 1e-2, seeds=[3])
    plain.set_kernel("generic")
    plain.set_params(0, init_params(3, 1, 32, 32, 32, 5), init_target=True)
    DeviceExperiment(plain, _env(40), gamma=0.99, warmup_steps=0)
    with pytest.raises(RlcError, match=refusal):                           # what the plain form does
        plain.set_kernel("mfma")
    assert plain.kernel_in_use() == "generic"
    plain.close()
    pops = [_pop(dims, B, None) for _ in range(2)]
    exps = [DeviceExperiment(p, _env(110), gamma=0.99, warmup_steps=0) for p in pops]
    with pytest.raises(RlcError, match=refusal):
        pops[0].set_kernel("mfma")
    assert pops[0].kernel_in_use() == "generic"
    for e in exps:
        e.run()
    _assert_same_bits(_state(pops[0], exps[0]), _state(pops[1], exps[1]))
    _check_against_oracle(pops[0], exps[0], dims, B, 110, "generic after the refused switch")
    for p in pops:
        p.close()


def test_layer_rollout_refusals_and_the_way_back_to_the_any_shape_kernel(hip_lib):
    """With a rollout attached to a layer-norm population on the MFMA kernel: latency mode stays refused; set_kernel("auto")
    returns the population to the any-shape kernel (weights and optimizer state re-packed, the device copy of the views
    refreshed) and the loop goes on there, inside the bounds either kernel keeps on its own."""
    from rlcontrol_amd._lib import RlcError
    from rlcontrol_amd.device_experiment import DeviceExperiment
    dims, B = SMALL
    pop = _pop(dims, B, "mfma")
    exp = DeviceExperiment(pop, _env(110), gamma=0.99, warmup_steps=0)
    with pytest.raises(RlcError, match="one-workgroup kernels"):
        pop.set_split(2)
    assert exp.advance(60) == 60
    with pytest.raises(RlcError, match="one-workgroup kernels"):
        pop.set_split(2)
    assert pop.kernel_in_use() == "mfma"
    before = [pop.get_blob(a, w) for a in range(2) for w in BLOBS]
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"
    for x, y in zip(before, [pop.get_blob(a, w) for a in range(2) for w in BLOBS]):
        assert np.array_equal(x, y)                                        # the re-pack loses no bit
    with pytest.raises(RlcError, match="cannot change once a rollout is attached"):
        pop.set_kernel("mfma")                                             # the way back in stays closed
    assert pop.kernel_in_use() == "generic"
    exp.advance(1000)
    assert exp.total_steps == 110
    _check_against_oracle(pop, exp, dims, B, 110, "mfma, then generic from step 61")
    pop.close()


# ---------------------------------------------------------------------------------------------------
# main.py --device_rollout
# ---------------------------------------------------------------------------------------------------
RUN_KEYS = {"random_seed", "total_timesteps", "eval_interval_timesteps", "episodes_per_eval", "eval_episode_rewards",
            "eval_episode_steps", "timesteps_at_eval", "train_episode_steps", "train_episode_rewards",
            "total_train_episodes", "eval_time", "train_time"}


def _drive(sweeps, indices):
    """run_indices_on_device on Pendulum-v0 with an in-memory agent json; returns (data, [(indices, kernel in use)])"""
    import main as drv
    import rlcontrol_amd.environments.environments as envs
    env_json = {"environment": "Pendulum-v0", "TotalMilSteps": 0.00006, "EpisodeSteps": 25,
                "EvalIntervalMilSteps": 0.00004, "EvalEpisodes": 2}
    base = {"shared_l1_dim": [32], "actor_l2_dim": [32], "critic_l2_dim": [32], "actor_lr": [1e-3, 1e-4],
            "critic_lr": [1e-2], "norm_type": ["layer"], "exploration_policy": ["ou_noise"], "batch_size": [16],
            "buffer_size": [1000]}
    agent_json = {"agent": "DDPG", "sweeps": dict(base, **sweeps)}
    env = envs.create_environment(env_json)
    env_params = {"env_name": env.name, "state_dim": env.state_dim, "state_min": env.state_min, "state_max": env.state_max,
                  "action_dim": env.action_dim, "action_min": env.action_min, "action_max": env.action_max}
    seen = []
    data = drv.new_data_dict(agent_json, env_json)
    drv.run_indices_on_device(list(indices), agent_json, env_json, env_params,
                              {"write_log": False, "write_plot": False, "device": 0}, data, verbose=False,
                              inspect=lambda idx, pop: seen.append((list(idx), pop.kernel_in_use())))
    return data, seen


def test_main_device_rollout_reads_hip_kernel_for_ddpg(hip_lib):
    from rlcontrol_amd._lib import RlcError
    data, seen = _drive({"hip_kernel": ["mfma"]}, range(2))
    assert seen == [([0, 1], "mfma")]
    assert sorted(data["experiment_data"]) == [0, 1]
    data, seen = _drive({}, range(2))
    assert seen == [([0, 1], "generic")]                       # without the key: layer norm stays on the any-shape kernel
    data, seen = _drive({"hip_kernel": ["mfma", "generic"]}, range(4))
    assert len(seen) == 2 and sorted(k for _, k in seen) == ["generic", "mfma"]
    assert sorted(i for idx, _ in seen for i in idx) == [0, 1, 2, 3] and all(len(idx) == 2 for idx, _ in seen)
    by_kernel = {}
    for sweep, rec in data["experiment_data"].items():
        assert len(rec["runs"]) == 1 and set(rec["runs"][0]) == RUN_KEYS
        run = rec["runs"][0]
        by_kernel.setdefault(rec["agent_params"]["hip_kernel"], []).append(
            sorted((k, type(v), np.shape(v)) for k, v in run.items()))
        assert run["timesteps_at_eval"].tolist() == [0, 40] and run["train_episode_steps"].tolist() == [25, 25]
        assert run["eval_episode_rewards"].shape == (2, 2) and np.isfinite(run["eval_episode_rewards"]).all()
    assert sorted(by_kernel) == ["generic", "mfma"] and by_kernel["mfma"] == by_kernel["generic"]      # one pickle schema
    with pytest.raises(ValueError, match="hip_kernel"):
        _drive({"hip_kernel": ["fast"]}, range(2))
    # 200-wide layers at batch 100: refused with the library's message when the population is made, before any step
    with pytest.raises(RlcError, match=r"\d+ bytes of LDS .* 163840"):
        _drive({"hip_kernel": ["mfma"], "shared_l1_dim": [200], "actor_l2_dim": [200], "critic_l2_dim": [200],
                "batch_size": [100]}, range(2))
