"""The wide form of the DDPG MFMA update kernel (state_dim <= 32, action_dim in {1,2,3,4,6}; opt-in through
set_kernel("mfma")) against the CPU oracle, with the bounds of tests/test_gpu_ddpg.py: taps and every non-empty gradient
tensor within 1e-5 relative, gradient direction cosine > 1 - 1e-9, targets within 1e-5, beta powers rtol 1e-6.
Selecting "mfma" is a requirement here: a refusal fails the test."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _cos(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(x @ y / (np.linalg.norm(x) * np.linalg.norm(y) + 1e-300))


def _bounds(S, A):
    return -np.ones(S) * 2, np.ones(S) * 2, np.linspace(1.0, 2.0, A)


def _make(dims, B, n_agents=1, cap=4096, kernel="mfma", sep=False, norm_type="input_norm", seeds=None):
    from rlcontrol_amd.hip_ddpg import DDPGPopulation
    S, A, H1, HA, HC = dims
    smin, smax, amax = _bounds(S, A)
    pop = DDPGPopulation(n_agents, S, A, H1, HA, HC, B, cap, 0.01, smin, smax, -amax, amax, 1e-3, 1e-2,
                         seeds=seeds if seeds is not None else list(range(10, 10 + n_agents)), norm_type=norm_type,
                         separate_networks=sep)
    if kernel is not None:
        pop.set_kernel(kernel)                # no skip: a refusal is a failure
        assert pop.kernel_in_use() == kernel
    return pop


def _batch(rng, B, S, A):
    s = rng.uniform(-3, 3, (B, S))
    a = rng.uniform(-2, 2, (B, A))
    s2 = rng.uniform(-3, 3, (B, S))
    r = rng.uniform(-16, 0, B)
    g = np.where(rng.rand(B) < 0.2, 0.0, 0.99)
    return s, a, s2, r, g


def _replay(rng, N, S, A):
    """(s, a, r, s2, g) in replay_add_batch's order"""
    return (rng.uniform(-3, 3, (N, S)), rng.uniform(-2, 2, (N, A)), rng.uniform(-16, 0, N), rng.uniform(-3, 3, (N, S)),
            np.where(rng.rand(N) < 0.15, 0.0, 0.99))


# (S, A, H1, HA, HC), batch: the reference's MuJoCo shapes at its usual batch, a non-fused one (HA != HC), a small one, the
# padded seven-tile kernel, the largest state x action at the largest batch, a narrow state with wide actions; the last
# is the largest shape the LDS carve takes at batch 100 with 200-wide layers
CASES = [((11, 2, 200, 200, 200), 32), ((11, 3, 200, 200, 200), 32), ((17, 6, 200, 200, 200), 32),
         ((32, 4, 200, 160, 144), 64), ((9, 1, 64, 48, 40), 17), ((12, 3, 128, 128, 128), 100),
         ((32, 6, 128, 128, 128), 128), ((5, 3, 64, 64, 64), 16), ((17, 6, 200, 200, 200), 100)]
SEP_CASES = [((17, 6, 200, 200, 200), 32), ((12, 3, 128, 128, 128), 100)]


def _check_single_update(pop, o, lay, dims, B, label):
    rng = np.random.RandomState(11)
    s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
    pop.update_batch(0, s, a, s2, r, g)
    taps = o.update(s, a, s2, r, g, taps=True)
    for name in ("q", "y", "a_out", "dqda"):
        e = _rel(pop.last_tap(0, name), taps[name])
        print("%s %s: rel %.3e" % (label, name, e))
        assert e < 1e-5, name
    for which in ("grads_c", "grads_a"):
        got, want = pop.last_tap(0, which), taps[which]
        c = _cos(got, want)
        print("%s %s: 1 - cos %.3e" % (label, which, 1 - c))
        assert c > 1 - 1e-9, which
        for name, (off, shp) in lay.items():
            n = int(np.prod(shp))
            if np.any(want[off:off + n]):
                e = _rel(got[off:off + n], want[off:off + n])
                print("%s %s %s: rel %.3e" % (label, which, name, e))
                assert e < 1e-5, (which, name)
            else:
                assert not np.any(got[off:off + n]), (which, name)
    e = _rel(pop.get_blob(0, "theta_target"), o.theta_t)
    print("%s theta_target: rel %.3e" % (label, e))
    assert e < 1e-5
    assert np.allclose(pop.get_beta_powers(0), o.pw, rtol=1e-6)


@pytest.mark.parametrize("dims,B", CASES)
def test_wide_single_update_taps_and_gradients(hip_lib, dims, B):
    from oracle.ddpg import DDPGOracle, Dims, init_params
    pop = _make(dims, B)
    pop.enable_grad_taps(True)
    th = init_params(Dims(*dims), 3)
    pop.set_params(0, th)
    smin, smax, amax = _bounds(dims[0], dims[1])
    o = DDPGOracle(Dims(*dims), th, 1e-3, 1e-2, 0.01, smin, smax, amax)
    _check_single_update(pop, o, Dims(*dims).layout()[0], dims, B, "%s/%d" % (dims, B))
    pop.close()


@pytest.mark.parametrize("dims,B", SEP_CASES)
def test_wide_single_update_separate_networks(hip_lib, dims, B):
    from oracle.ddpg_variants import DDPGVariantOracle, VDims, init_params
    d = VDims(*dims, norm=False, separate=True)
    pop = _make(dims, B, sep=True)
    pop.enable_grad_taps(True)
    th = init_params(d, 2)
    pop.set_params(0, th)
    smin, smax, amax = _bounds(dims[0], dims[1])
    o = DDPGVariantOracle(d, th, 1e-3, 1e-2, 0.01, smin, smax, amax)
    _check_single_update(pop, o, d.layout()[0], dims, B, "separate %s/%d" % (dims, B))
    pop.close()


def test_wide_ten_updates_from_replay_with_host_indices(hip_lib):
    from oracle.ddpg import DDPGOracle, Dims, init_params
    from rlcontrol_amd.utils.custom_collections import DistinctIndexSampler
    dims, B, N = (17, 6, 200, 200, 200), 32, 4096
    pop = _make(dims, B, cap=N)
    th = init_params(Dims(*dims), 0)
    pop.set_params(0, th)
    s, a, r, s2, g = _replay(np.random.RandomState(5), N, dims[0], dims[1])
    pop.replay_add_batch(0, s, a, r, s2, g)
    smin, smax, amax = _bounds(dims[0], dims[1])
    o = DDPGOracle(Dims(*dims), th, 1e-3, 1e-2, 0.01, smin, smax, amax)
    smp = DistinctIndexSampler(0)
    for it in range(10):
        idx = smp.sample_n_k(N, B)
        pop.update(1, host_indices=idx)
        taps = o.update(s[idx], a[idx], s2[idx], r[idx], g[idx], taps=True)
        tol = 1e-5 if it == 0 else 2e-4
        for name in ("q", "y", "a_out", "dqda"):
            e = _rel(pop.last_tap(0, name), taps[name])
            print("update %d %s: rel %.3e" % (it, name, e))
            assert e < tol, (it, name)
    assert _rel(pop.get_blob(0, "theta_target"), o.theta_t) < 1e-4
    pop.close()


BLOBS = ("theta", "theta_target", "actor_m", "actor_v", "critic_m", "critic_v")


def test_wide_kernel_switch_round_trip_with_optimizer_state(hip_lib):
    """generic -> mfma -> generic re-packs the weights and both optimizers' state without touching a bit; one more
    update on each kernel from equal state agrees on the taps"""
    from oracle.ddpg import Dims, init_params
    dims, B = (17, 6, 200, 200, 200), 32
    rng = np.random.RandomState(2)
    pops = [_make(dims, B, kernel=None) for _ in range(2)]
    th = init_params(Dims(*dims), 9)
    for pop in pops:
        assert pop.kernel_in_use() == "generic"
        pop.set_params(0, th)
    for _ in range(2):                                  # optimizer state that is not all zero
        batch = _batch(rng, B, dims[0], dims[1])
        for pop in pops:
            pop.update_batch(0, *batch)
    a, b = pops
    before = {w: a.get_blob(0, w) for w in BLOBS}
    pw = a.get_beta_powers(0)
    for w in BLOBS:
        assert np.array_equal(b.get_blob(0, w), before[w]), w
    a.set_kernel("mfma")
    assert a.kernel_in_use() == "mfma"
    for w in BLOBS:
        assert np.array_equal(a.get_blob(0, w), before[w]), w
    a.set_kernel("generic")
    assert a.kernel_in_use() == "generic"
    for w in BLOBS:
        assert np.array_equal(a.get_blob(0, w), before[w]), w
    assert np.array_equal(a.get_beta_powers(0), pw)
    a.set_kernel("mfma")
    batch = _batch(rng, B, dims[0], dims[1])
    a.update_batch(0, *batch)                            # the wide MFMA kernel from the re-packed state
    b.update_batch(0, *batch)                            # the any-shape kernel from the same state
    for name in ("q", "y", "a_out", "dqda"):
        e = _rel(a.last_tap(0, name), b.last_tap(0, name))
        print("mfma vs generic %s: rel %.3e" % (name, e))
        assert e < 1e-5, name
    for pop in pops:
        pop.close()


def test_wide_k_updates_in_one_launch_equal_k_launches(hip_lib):
    from oracle.ddpg import Dims, init_params
    dims, B, N = (17, 6, 200, 200, 200), 32, 2000
    rng = np.random.RandomState(3)
    data = _replay(rng, N, dims[0], dims[1])
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(4)]).astype(np.int64)
    blobs = []
    for mode in ("one", "many"):
        pop = _make(dims, B, cap=N)
        pop.set_params(0, init_params(Dims(*dims), 5))
        pop.replay_add_batch(0, *data)
        if mode == "one":
            pop.update(4, host_indices=idx)
        else:
            for k in range(4):
                pop.update(1, host_indices=idx[k])
        blobs.append([pop.get_blob(0, w) for w in BLOBS])
        pop.close()
    for w, x, y in zip(BLOBS, *blobs):
        assert np.array_equal(x, y), w


def test_wide_acting_on_the_blocked_layout_equals_the_any_shape_path(hip_lib):
    from oracle.ddpg import DDPGOracle, Dims, init_params
    dims, NA = (17, 6, 200, 200, 200), 3
    rng = np.random.RandomState(4)
    smin, smax, amax = _bounds(dims[0], dims[1])
    pops = {k: _make(dims, 32, n_agents=NA, kernel=k) for k in ("generic", "mfma")}
    ths = [init_params(Dims(*dims), 30 + i) for i in range(NA)]
    for pop in pops.values():
        for i in range(NA):
            pop.set_params(i, ths[i])
    sts = rng.uniform(-3, 3, (NA, dims[0]))
    ref = pops["generic"].act(sts)
    got = pops["mfma"].act(sts)
    print("act: max abs difference %.3e" % float(np.max(np.abs(got - ref))))
    assert np.array_equal(got, ref) or _rel(got, ref) < 1e-6
    n = pops["mfma"].act_queue(sts)
    queued = pops["mfma"].act_fetch(n)
    assert np.array_equal(queued, got)
    for i in range(NA):
        o = DDPGOracle(Dims(*dims), ths[i], 1e-3, 1e-2, 0.01, smin, smax, amax)
        assert _rel(got[i], o.act(sts[i:i + 1])) < 1e-5
        many, acts = rng.uniform(-3, 3, (33, dims[0])), rng.uniform(-2, 2, (33, dims[1]))
        q = pops["mfma"].qval(i, many, acts)
        assert _rel(q, pops["generic"].qval(i, many, acts)) < 1e-6
        assert _rel(q, o.qval(many, acts)) < 1e-5
    for pop in pops.values():
        pop.close()


def test_wide_selection_is_opt_in_and_refusals_name_the_limit(hip_lib):
    from rlcontrol_amd._lib import RlcError
    pop = _make((17, 6, 200, 200, 200), 32, kernel=None)
    assert pop.kernel_in_use() == "generic"            # a new wide population starts on the any-shape kernel
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    with pytest.raises(RlcError, match=r"state_dim <= 8, action_dim <= 2"):
        pop.set_split(2)                               # latency mode has no wide form
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"            # auto does not choose the wide form
    pop.close()
    lead = "MFMA kernel does not support these dimensions"
    for dims, B, why in (((33, 2, 200, 200, 200), 32, r"state_dim <= 32"),
                         ((11, 5, 200, 200, 200), 32, r"action_dim in \{1, 2, 3, 4, 6\}"),
                         ((11, 7, 200, 200, 200), 32, r"action_dim in \{1, 2, 3, 4, 6\}"),
                         ((32, 6, 200, 200, 200), 128, r"\d+ bytes of LDS .* 163840")):
        pop = _make(dims, B, kernel=None)
        with pytest.raises(RlcError, match=lead + ".*" + why):
            pop.set_kernel("mfma")
        assert pop.kernel_in_use() == "generic"
        pop.close()
    pop = _make((17, 6, 200, 200, 200), 32, kernel=None, norm_type="layer")
    with pytest.raises(RlcError, match=lead + ".*layer"):
        pop.set_kernel("mfma")
    pop.close()
    # the narrow shapes keep their default
    pop = _make((8, 2, 200, 200, 200), 32, kernel=None)
    assert pop.kernel_in_use() == "mfma"
    pop.close()


def _agent_config(kernel):
    from rlcontrol_amd.utils.config import Config
    S, A = 17, 6
    cfg = Config()
    cfg.merge_config({"env_name": "synthetic-17-6", "state_dim": S, "state_min": -np.ones(S) * 5, "state_max": np.ones(S) * 5,
                      "action_dim": A, "action_min": -np.ones(A), "action_max": np.ones(A)})
    cfg.merge_config({"norm_type": "input_norm", "exploration_policy": "ou_noise", "shared_l1_dim": 200,
                      "actor_l2_dim": 200, "critic_l2_dim": 200, "actor_lr": 0.001, "critic_lr": 0.01,
                      "batch_size": 32, "buffer_size": 5000, "writer": None, "replay_sampler": "reference"})
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": 1})
    if kernel is not None:
        cfg.merge_config({"hip_kernel": kernel})
    return cfg


def test_wide_dropin_agent_follows_the_any_shape_agent(hip_lib):
    """create_agent("DDPG") at HalfCheetah's shape with hip_kernel "mfma" and "generic", driven by the same seeded
    random transitions for 200 steps"""
    from rlcontrol_amd.utils.main_utils import create_agent
    plain = create_agent("DDPG", _agent_config(None))
    assert plain.network_manager.population.kernel_in_use() == "generic"
    agents = {k: create_agent("DDPG", _agent_config(k)) for k in ("mfma", "generic")}
    for k, ag in agents.items():
        assert ag.network_manager.population.kernel_in_use() == k
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, 17)
    first = {k: ag.start(obs, True) for k, ag in agents.items()}
    assert np.allclose(first["mfma"], first["generic"], atol=1e-6), first
    for t in range(200):
        act = rng.uniform(-1, 1, 6)
        obs_n, r = rng.uniform(-1, 1, 17), float(rng.uniform(-1, 0))
        for ag in agents.values():
            ag.update(obs, obs_n, r, act, False, False)
            ag.step(obs_n, True)
        obs = obs_n
    pops = {k: ag.network_manager.population for k, ag in agents.items()}
    e = _rel(pops["mfma"].last_tap(0, "q"), pops["generic"].last_tap(0, "q"))
    print("q tap after 200 steps, mfma vs generic: rel %.3e" % e)
    assert e < 2e-4
