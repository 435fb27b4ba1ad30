"""The layer-norm form of the DDPG MFMA update kernel (norm_type 'layer' on the hydra network at state_dim <= 8, action_dim
<= 2; opt-in through set_kernel("mfma")) against oracle.ddpg_variants.DDPGVariantOracle(VDims(..., norm=True)), with the
helpers, the generator and the bounds of tests/test_ddpg_variants.py: first update taps 1e-5, every non-empty gradient
tensor 3e-5, theta / theta_target 1e-5; later updates 2e-4.  Selecting "mfma" is a requirement here: a refusal fails
the test."""
import numpy as np
import pytest

import test_ddpg_variants as V
from oracle.ddpg_variants import DDPGVariantOracle, VDims

pytestmark = pytest.mark.gpu

_rel, _batch, _bounds, init_params = V._rel, V._batch, V._bounds, V.init_params
BLOBS = ("theta", "theta_target", "actor_m", "actor_v", "critic_m", "critic_v")
PENDULUM = (3, 1, 200, 200, 200)

# (S, A, H1, HA, HC), batch: two tiles with ragged widths and batch and HA != HC; A = 2 on whole tiles; the shipped json's
# shape (13 tiles with the split hand-off, K ending in 8); four tiles with S = 8 at the largest batch 200-wide layers fit;
# seven tiles with the padded last tile; the capacity case at seven tiles (136-wide rows at stride 136); eight tiles
SHAPES = [((3, 1, 32, 24, 40), 17), ((5, 2, 48, 64, 32), 32), (PENDULUM, 32), ((8, 2, 200, 160, 144), 64),
          ((3, 1, 64, 72, 48), 100), ((3, 1, 136, 128, 136), 97), ((3, 1, 64, 48, 72), 113)]


def _theta(d, seed=2):
    """init_params with gamma / beta moved off their trivial values by U(+-0.3) drawn from RandomState(1); returns the
    generator for the minibatches that follow, as tests/test_ddpg_variants.py draws them"""
    th = init_params(d, seed)
    rng = np.random.RandomState(1)
    for n, (off, shp) in d.layout()[0].items():
        if n[0] == "l":
            k = int(np.prod(shp))
            th[off:off + k] += rng.uniform(-0.3, 0.3, k).astype(np.float32)
    return th, rng


def _pop(dims, B, kernel="mfma", n_agents=1, cap=512, sep=False):
    pop = V._pop(dims, B, True, sep, n_agents=n_agents, cap=cap)
    if kernel is not None:
        pop.set_kernel(kernel)                # no skip: a refusal is a failure
        assert pop.kernel_in_use() == kernel
    return pop


def _oracle(d, th):
    smin, smax, amax = _bounds(d.S, d.A)
    return DDPGVariantOracle(d, th, 1e-3, 1e-2, 0.01, smin, smax, amax)


@pytest.mark.parametrize("dims,B", SHAPES)
def test_layer_mfma_update_matches_oracle(hip_lib, dims, B):
    d = VDims(*dims, norm=True)
    th, rng = _theta(d)
    lay, P = d.layout()
    pop = _pop(dims, B)
    assert pop.P == P
    pop.enable_grad_taps(True)
    pop.set_params(0, th)
    o = _oracle(d, th)
    for it in range(3):
        s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
        pop.update_batch(0, s, a, s2, r, g)
        t = o.update(s, a, s2, r, g, taps=True)
        tol = 1e-5 if it == 0 else 2e-4
        for k in ("q", "y", "a_out", "dqda"):
            e = _rel(pop.last_tap(0, k), t[k])
            print("%s B%d update %d %s: rel %.3e" % (dims, B, it, k, e))
            assert e < tol, (it, k)
        if it == 0:
            for tag in ("grads_c", "grads_a"):
                got = pop.last_tap(0, tag)
                for n, (off, shp) in lay.items():
                    k = int(np.prod(shp))
                    if np.max(np.abs(t[tag][off:off + k])) > 0:
                        e = _rel(got[off:off + k], t[tag][off:off + k])
                        print("%s B%d %s %s: rel %.3e" % (dims, B, tag, n, e))
                        assert e < 3e-5, (tag, n)
            for tag in ("grads_c", "grads_a"):              # the six gamma / beta tensors are among the non-empty ones
                both = [n for n in lay if n[0] == "l" and np.any(t[tag][lay[n][0]:lay[n][0] + lay[n][1][0]])]
                assert len(both) == 4, (tag, both)          # the trunk's pair + the critic's (grads_c) / the actor's (grads_a)
            e_t, e_tt = _rel(pop.get_blob(0, "theta"), o.theta), _rel(pop.get_blob(0, "theta_target"), o.theta_t)
            print("%s B%d theta rel %.3e theta_target rel %.3e" % (dims, B, e_t, e_tt))
            assert e_t < 1e-5 and e_tt < 1e-5
    # acting and qval read the blocked layout through the layer norms
    st = rng.uniform(-2, 2, (1, dims[0]))
    assert _rel(pop.act(st), o.act(st)) < 1e-5
    s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
    q_want = _oracle(d, o.theta.copy()).update(s, a, s2, r, g, taps=True)["q"]     # Q(s, a) at the current weights
    assert _rel(pop.qval(0, s, a), q_want) < 1e-5
    pop.close()


@pytest.mark.parametrize("dims,B", [(PENDULUM, 32), ((3, 1, 64, 72, 48), 100)])
def test_layer_mfma_optimizer_state_per_element(hip_lib, dims, B):
    """Adam's m / v, the stepped weights and the Polyak targets per element: the checks of tests/optimizer_state_checks.py
    exactly as tests/test_gpu_optimizer_state.py applies them"""
    import test_gpu_optimizer_state as OS
    from optimizer_state_cases import DDPGCase
    OS.test_optimizer_state_and_target_after_one_update(hip_lib, DDPGCase(dims, B, "mfma", norm=True))


def test_layer_mfma_replay_two_agents_and_determinism(hip_lib):
    dims, B, N = PENDULUM, 32, 512
    d = VDims(*dims, norm=True)
    rng = np.random.RandomState(3)
    data = (rng.uniform(-2, 2, (N, 3)), rng.uniform(-1, 1, (N, 1)), rng.uniform(-16, 0, N), rng.uniform(-2, 2, (N, 3)),
            np.full(N, 0.99))
    ths = [_theta(d, 30 + i)[0] for i in range(2)]
    idx = np.stack([rng.choice(N, B, replace=False) for _ in range(4)]).reshape(2, 2, B).astype(np.int64)

    def fresh():
        pop = _pop(dims, B, n_agents=2, cap=N)
        for i in range(2):
            pop.set_params(i, ths[i])
            pop.replay_add_batch(i, *data)
        return pop
    pop = fresh()
    pop.update(2, host_indices=idx)
    for i in range(2):
        o = _oracle(d, ths[i])
        for k in range(2):
            j = idx[i, k]
            t = o.update(data[0][j], data[1][j], data[3][j], data[2][j], data[4][j], taps=True)
        for name in ("q", "y", "dqda"):
            e = _rel(pop.last_tap(i, name), t[name])
            print("agent %d %s after two fused updates: rel %.3e" % (i, name, e))
            assert e < 2e-4, (i, name)
    one = [[pop.get_blob(i, w) for w in BLOBS] for i in range(2)]
    twin = fresh()
    for k in range(2):
        twin.update(1, host_indices=idx[:, k:k + 1])
    for i in range(2):
        assert not np.array_equal(one[i][0], ths[i])
        for w, x in zip(BLOBS, one[i]):
            assert np.array_equal(x, twin.get_blob(i, w)), (i, w)           # K updates in one launch == K launches
    twin.close()
    pop.update(3)                                                          # device sampler path
    for i in range(2):
        assert np.all(np.isfinite(pop.get_blob(i, "theta"))) and np.all(np.isfinite(pop.get_blob(i, "theta_target")))
    pop.close()


def test_layer_mfma_layout_round_trip(hip_lib):
    dims, B = PENDULUM, 32
    d = VDims(*dims, norm=True)
    th, rng = _theta(d)
    pops = {k: _pop(dims, B, kernel=None) for k in ("generic", "mfma")}
    for k, pop in pops.items():
        pop.set_params(0, th)
        pop.set_kernel(k)
        assert pop.kernel_in_use() == k
        assert np.array_equal(pop.get_blob(0, "theta"), th), k              # the re-pack loses no bit
        assert np.array_equal(pop.get_blob(0, "theta_target"), th), k
    o = _oracle(d, th)
    s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
    for pop in pops.values():
        pop.update_batch(0, s, a, s2, r, g)
    o.update(s, a, s2, r, g)
    e = _rel(pops["mfma"].get_blob(0, "theta"), pops["generic"].get_blob(0, "theta"))
    print("theta after one update, mfma vs generic: rel %.3e" % e)
    assert e < 1e-5
    pops["generic"].close()
    pop = pops["mfma"]
    pop.set_kernel("generic")                                               # back to row-major, optimizer state included
    assert pop.kernel_in_use() == "generic"
    for it in range(2):
        s, a, s2, r, g = _batch(rng, B, dims[0], dims[1])
        pop.update_batch(0, s, a, s2, r, g)
        t = o.update(s, a, s2, r, g, taps=True)
        for k in ("q", "y", "a_out", "dqda"):
            assert _rel(pop.last_tap(0, k), t[k]) < 2e-4, (it, k)
    assert _rel(pop.get_blob(0, "theta"), o.theta) < 2e-4
    pop.close()


def test_layer_mfma_selection_is_opt_in_and_refusals_name_the_limit(hip_lib):
    from rlcontrol_amd._lib import RlcError
    lead = "MFMA kernel does not support these dimensions"
    pop = _pop(PENDULUM, 32, kernel=None)
    assert pop.kernel_in_use() == "generic"            # a new layer-norm population starts on the any-shape kernel
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"            # auto does not choose the layer-norm form
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    with pytest.raises(RlcError):
        pop.set_split(2)                               # latency mode has no layer-norm form
    pop.set_kernel("auto")
    assert pop.kernel_in_use() == "generic"
    pop.close()
    pop = _pop(PENDULUM, 64, kernel="mfma")            # the largest batch tile count 200-wide layers fit
    pop.close()
    pop = _pop(PENDULUM, 100, kernel=None)
    with pytest.raises(RlcError, match=lead + r".*\d+ bytes of LDS .* 163840"):
        pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "generic"
    pop.close()
    pop = _pop(PENDULUM, 32, kernel=None, sep=True)
    with pytest.raises(RlcError, match=lead + r".*layer.*separate"):
        pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "generic"
    pop.close()
    pop = _pop(PENDULUM, 32, kernel=None)
    with pytest.raises(RlcError):
        pop.set_split(2)                               # ... nor on the any-shape kernel
    pop.close()


def _agent_config(kernel):
    from rlcontrol_amd.utils.config import Config
    cfg = Config()
    cfg.merge_config({"env_name": "Pendulum-v0", "state_dim": 3, "state_min": np.array([-1.0, -1.0, -8.0]),
                      "state_max": np.array([1.0, 1.0, 8.0]), "action_dim": 1, "action_min": np.array([-2.0]),
                      "action_max": np.array([2.0])})
    cfg.merge_config({"norm_type": "layer", "exploration_policy": "ou_noise", "shared_l1_dim": 200, "actor_l2_dim": 200,
                      "critic_l2_dim": 200, "actor_lr": 0.001, "critic_lr": 0.01, "batch_size": 32, "buffer_size": 5000,
                      "writer": None, "replay_sampler": "reference"})
    cfg.merge_config({"write_log": False, "write_plot": False, "random_seed": 1})
    if kernel is not None:
        cfg.merge_config({"hip_kernel": kernel})
    return cfg


def test_layer_mfma_dropin_agent_follows_the_any_shape_agent(hip_lib):
    """create_agent("DDPG") with norm_type 'layer' at the Pendulum shape with hip_kernel "mfma" and "generic", driven by
    the same seeded random transitions for 200 steps, as tests/test_gpu_ddpg_wide.py drives its pair: same acting
    stream, q tap and parameters within that test's 2e-4"""
    from rlcontrol_amd.utils.main_utils import create_agent
    plain = create_agent("DDPG", _agent_config(None))
    assert plain.network_manager.population.kernel_in_use() == "generic"
    agents = {k: create_agent("DDPG", _agent_config(k)) for k in ("mfma", "generic")}
    for k, ag in agents.items():
        assert ag.network_manager.population.kernel_in_use() == k
    rng = np.random.RandomState(7)
    obs = rng.uniform(-1, 1, 3)
    first = {k: ag.start(obs, True) for k, ag in agents.items()}
    assert np.allclose(first["mfma"], first["generic"], atol=1e-6), first
    for t in range(200):
        act = rng.uniform(-2, 2, 1)
        obs_n, r = rng.uniform(-1, 1, 3), float(rng.uniform(-1, 0))
        for ag in agents.values():
            ag.update(obs, obs_n, r, act, False, False)
            ag.step(obs_n, True)
        obs = obs_n
    pops = {k: ag.network_manager.population for k, ag in agents.items()}
    e = _rel(pops["mfma"].last_tap(0, "q"), pops["generic"].last_tap(0, "q"))
    e_th = _rel(pops["mfma"].get_blob(0, "theta"), pops["generic"].get_blob(0, "theta"))
    print("after 200 steps, mfma vs generic: q tap rel %.3e, theta rel %.3e" % (e, e_th))
    assert e < 2e-4 and e_th < 2e-4
