"""The wide form of the NAF MFMA update kernel (state_dim <= 32, action_dim in {1,2,3,4,6}, i.e. up to 21 L heads; opt-in
through set_kernel("mfma")) against the CPU oracle, at the levels of tests/test_naf.py: taps q / y / V within 1e-5 on the
first update and 2e-4 on the next two, every gradient tensor of the first update within 2e-5, targets within 1e-5, beta
powers rtol 1e-6.  Selecting "mfma" is a requirement here: a refusal fails the test."""
import numpy as np
import pytest

from oracle.naf import NAFOracle, NafDims, init_params

pytestmark = pytest.mark.gpu

LR, TAU = 1e-3, 0.01
BLOBS = ("theta", "theta_target", "adam_m", "adam_v")


def _rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _bounds(S, A):
    return -np.ones(S) * 2, np.ones(S) * 2, np.linspace(1.0, 2.0, A)


def _batch(rng, B, S, A):
    return (rng.uniform(-3, 3, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-3, 3, (B, S)),
            rng.uniform(-16, 0, B), np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def _pop(dims, B, n_agents=1, cap=2048, kernel="mfma", norm_type="input_norm"):
    from rlcontrol_amd.hip_naf import NAFPopulation
    S, A, L1, L2 = dims
    smin, smax, amax = _bounds(S, A)
    pop = NAFPopulation(n_agents, S, A, L1, L2, B, cap, TAU, smin, smax, amax, LR, seeds=list(range(3, 3 + n_agents)),
                        norm_type=norm_type)
    if kernel is not None:
        pop.set_kernel(kernel)                # no skip: a refusal is a failure
        assert pop.kernel_in_use() == kernel
    return pop


# (S, A, L1, L2), batch -- the smallest shapes at which each new piece can go wrong: the first shape past one chunk of
# eight inputs (row stride 12, one head); wide by action only (6 heads in 8 slots); wide by state only on four tiles; three
# chunks with 21 heads (head-bias rounds); the state limit with 10 heads in 12 slots; seven tiles with a padded tail; two N
# tiles per wave with unequal widths; eight tiles (127,168 B of LDS at these widths: it fits, so the widths stay at 128)
CASES = [((9, 1, 64, 48), 17), ((3, 3, 64, 48), 17), ((11, 2, 64, 48), 33), ((17, 6, 64, 48), 32), ((32, 4, 64, 48), 17),
         ((11, 3, 64, 48), 100), ((17, 6, 200, 160), 32), ((11, 3, 128, 128), 113)]


@pytest.mark.parametrize("dims,B", CASES)
def test_wide_naf_update_matches_oracle(hip_lib, dims, B):
    d = NafDims(*dims)
    th = init_params(d, 2)
    smin, smax, amax = _bounds(dims[0], dims[1])
    pop = _pop(dims, B)
    pop.enable_grad_taps(True)
    pop.set_params(0, th)
    o = NAFOracle(d, th, LR, TAU, smin, smax, amax)
    rng = np.random.RandomState(1)
    label = "%s/%d" % (dims, B)
    for it in range(3):
        s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
        pop.update_batch(0, s, a, s2, r, g)
        t = o.update(s, a, s2, r, g, taps=True)
        tol = 1e-5 if it == 0 else 2e-4
        for k in ("q", "y", "V"):
            e = _rel(pop.last_tap(0, k), t[k])
            print("%s update %d %s: rel %.3e" % (label, it, k, e))
            assert e < tol, (it, k)
        if it == 0:
            got = pop.last_tap(0, "grads")
            lay, _ = d.layout()
            for n, (off, shp) in lay.items():
                k = int(np.prod(shp))
                e = _rel(got[off:off + k], t["grads"][off:off + k])
                print("%s grads %s: rel %.3e" % (label, n, e))
                assert e < 2e-5, n
            e = _rel(pop.get_blob(0, "theta_target"), o.theta_t)
            print("%s theta_target: rel %.3e" % (label, e))
            assert e < 1e-5
            assert np.allclose(pop.get_beta_powers(0), o.pw, rtol=1e-6)
    pop.close()


def test_wide_naf_selection_is_opt_in(hip_lib):
    pop = _pop((17, 6, 64, 48), 32, kernel=None)
    assert pop.kernel_in_use() == "generic"            # a new wide population starts on the any-shape kernel
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"            # auto does not choose the wide form
    pop.close()
    pop = _pop((8, 2, 64, 48), 32, kernel=None)
    assert pop.kernel_in_use() == "mfma"               # the narrow shapes keep their default
    pop.close()


def test_wide_naf_refusals_name_the_limit(hip_lib):
    from rlcontrol_amd._lib import RlcError
    lead = "MFMA NAF kernel does not support these dimensions"
    for dims, B, why in (((33, 2, 64, 48), 32, r"state_dim <= 32"),
                         ((11, 5, 64, 48), 32, r"action_dim in \{1, 2, 3, 4, 6\}"),
                         ((17, 6, 200, 200), 100, r"\d+ bytes of LDS .* 163840")):     # HalfCheetah, 200-wide, seven tiles: 203,840 B
        pop = _pop(dims, B, kernel=None)
        with pytest.raises(RlcError, match=lead + ".*" + why):
            pop.set_kernel("mfma")
        assert pop.kernel_in_use() == "generic"
        pop.close()
    with pytest.raises(RlcError, match=r"NAF supports action_dim <= 6 \(got 7\)"):      # rlc_naf_create stops at six
        _pop((11, 7, 64, 48), 32, kernel=None)
    pop = _pop((17, 6, 64, 48), 32, kernel=None, norm_type="layer")
    with pytest.raises(RlcError, match=lead + ".*layer"):
        pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "generic"
    pop.close()


def test_wide_naf_kernel_switch_round_trip_with_optimizer_state(hip_lib):
    """generic -> mfma -> generic re-packs the weights and the optimizer state without touching a bit; one more update on
    each kernel from equal state agrees within 2e-4 (tests/test_naf.py, the kernel-switch test)"""
    dims, B = (17, 6, 64, 48), 32
    d = NafDims(*dims)
    th = init_params(d, 7)
    rng = np.random.RandomState(5)
    pops = [_pop(dims, B, kernel=None) for _ in range(2)]
    for pop in pops:
        assert pop.kernel_in_use() == "generic"
        pop.set_params(0, th)
    for _ in range(2):                                  # optimizer state that is not all zero
        batch = _batch(rng, B, dims[0], dims[1])
        for pop in pops:
            pop.update_batch(0, *batch)
    a_, b_ = pops
    before = {w: a_.get_blob(0, w) for w in BLOBS}
    pw = a_.get_beta_powers(0)
    for w in BLOBS:
        assert np.array_equal(b_.get_blob(0, w), before[w]), w
    a_.set_kernel("mfma")
    assert a_.kernel_in_use() == "mfma"
    for w in BLOBS:
        assert np.array_equal(a_.get_blob(0, w), before[w]), w
    a_.set_kernel("generic")
    assert a_.kernel_in_use() == "generic"
    for w in BLOBS:
        assert np.array_equal(a_.get_blob(0, w), before[w]), w
    assert np.array_equal(a_.get_beta_powers(0), pw)
    a_.set_kernel("mfma")
    batch = _batch(rng, B, dims[0], dims[1])
    a_.update_batch(0, *batch)                          # the wide MFMA kernel from the re-packed state
    b_.update_batch(0, *batch)                          # the any-shape kernel from the same state
    for name in ("q", "y", "V"):
        e = _rel(a_.last_tap(0, name), b_.last_tap(0, name))
        print("mfma vs generic %s: rel %.3e" % (name, e))
        assert e < 2e-4, name
    for w in BLOBS:
        e = _rel(a_.get_blob(0, w), b_.get_blob(0, w))
        print("mfma vs generic %s: rel %.3e" % (w, e))
        assert e < 2e-4, w
    for pop in pops:
        pop.close()


def test_wide_naf_replay_path_and_act(hip_lib):
    dims, B, N = (17, 6, 64, 48), 32, 2048
    S, A = dims[:2]
    d = NafDims(*dims)
    smin, smax, amax = _bounds(S, A)
    pop = _pop(dims, B, n_agents=2, cap=N)
    ths = [init_params(d, 10 + i) for i in range(2)]
    rng = np.random.RandomState(1)
    s, a, s2 = rng.uniform(-3, 3, (N, S)), rng.uniform(-2, 2, (N, A)), rng.uniform(-3, 3, (N, S))
    r, g = rng.uniform(-16, 0, N), np.where(rng.rand(N) < 0.2, 0.0, 0.99)
    for i in range(2):
        pop.set_params(i, ths[i])
        pop.replay_add_batch(i, s, a, r, s2, g)
    oracles = [NAFOracle(d, ths[i], LR, TAU, smin, smax, amax) for i in range(2)]
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(4)]).reshape(2, 2, B).astype(np.int64)
    pop.update(2, host_indices=idx)
    for i in range(2):
        for k in range(2):
            j = idx[i, k]
            t = oracles[i].update(s[j], a[j], s2[j], r[j], g[j], taps=True)
        for name in ("q", "y", "V"):
            e = _rel(pop.last_tap(i, name), t[name])
            print("replay agent %d %s: rel %.3e" % (i, name, e))
            assert e < 2e-4, (i, name)
    # acting on the tile-blocked layout: mu and the 21 entries of the L columns
    assert pop.kernel_in_use() == "mfma"
    st = rng.uniform(-3, 3, (2, S))
    mu, lc = pop.act(st, with_lcols=True)
    assert mu.shape == (2, A) and lc.shape == (2, A * (A + 1) // 2)
    for i in range(2):
        wm, wl = oracles[i].act(st[i:i + 1])
        assert _rel(mu[i], wm[0]) < 1e-5 and _rel(lc[i], wl[0]) < 1e-5, i
    pop.update(3)                                    # device sampler
    for i in range(2):
        for w in BLOBS:
            assert np.all(np.isfinite(pop.get_blob(i, w))), (i, w)
    pop.close()


def _agent_config(kernel):
    from rlcontrol_amd.utils.config import Config
    S, A = 17, 6
    cfg = Config()
    cfg.merge_config({"env_name": "synthetic-17-6", "state_dim": S, "state_min": -np.ones(S) * 5, "state_max": np.ones(S) * 5,
                      "action_dim": A, "action_min": -np.ones(A), "action_max": np.ones(A)})
    cfg.merge_config({"norm_type": "input_norm", "exploration_policy": "none", "l1_dim": 64, "l2_dim": 48,
                      "noise_scale": 0.3, "learning_rate": 1e-3, "batch_size": 32, "buffer_size": 5000, "writer": None})
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": 1})
    if kernel is not None:
        cfg.merge_config({"hip_kernel": kernel})
    return cfg


def test_wide_naf_dropin_agent_honours_hip_kernel(hip_lib):
    from rlcontrol_amd.utils.main_utils import create_agent
    plain = create_agent("NAF", _agent_config(None))
    assert plain.network_manager.population.kernel_in_use() == "generic"
    with pytest.raises(ValueError, match="hip_kernel"):
        create_agent("NAF", _agent_config("fast"))
    for kernel in ("mfma", "generic"):
        agent = create_agent("NAF", _agent_config(kernel))
        assert agent.network_manager.population.kernel_in_use() == kernel
        rng = np.random.RandomState(7)
        obs = rng.uniform(-1, 1, 17)
        agent.reset()
        act = agent.start(obs, True)
        for t in range(60):
            obs_n, r = rng.uniform(-1, 1, 17), float(rng.uniform(-1, 0))
            agent.update(obs, obs_n, r, act, False, False)
            act = agent.step(obs_n, True)
            obs = obs_n
            assert act.shape == (6,) and np.all(np.isfinite(act)) and np.all(np.abs(act) <= 1.0), (kernel, t, act)
        assert np.all(np.isfinite(agent.network_manager.population.get_blob(0, "theta"))), kernel
