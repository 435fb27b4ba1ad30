"""The clamp gates of the NAF and ReverseKL / ForwardKL update kernels on the GPU ("Clamp gates").

NAF: the diagonal of L is exp(clip(d, -5, 5)) and the seed of d is gated by (-5 <= d <= 5) in naf_generic.hip and
naf_mfma_kernel.h (narrow and wide forms); naf_policy.h clamps again for act and for the exploration draw of the on-device
loop.  KL: log_std = clamp(., -20, 2), gated per action dimension on the likelihood and on the integral path of
kl_generic.hip and kl_mfma_kernel.h (action_dim 1 and 2); acting goes through sac_policy.h.

Every case, its weights and its minibatch seed come from tests/clamp_cases.py, where tests/test_clamp_cases.py asserts on
the CPU that the restatements alone put the pre-activations where the case wants them, with a margin, and that a backward
pass without the gate would miss the bar by two orders of magnitude.  Comparisons are `_held`: the device against the
float64 twin is at most max(bar, 3 x the fp32 restatement against the twin); the bars are those of tests/test_naf.py and
tests/test_kl.py.  Gradients are compared on the first update only."""
import numpy as np
import pytest
import torch

import clamp_cases as C
from oracle import kl_torch as K
from oracle.naf import NAFOracle, NafDims

pytestmark = pytest.mark.gpu

F32 = np.float32


def _np(x):
    return x.detach().numpy() if torch.is_tensor(x) else np.asarray(x)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _select(pop, kernel, must=False):
    """the kernel under test, explicitly; a refusal skips (the any-shape kernel covers the shape) unless the case exists
    for that kernel"""
    from rlcontrol_amd._lib import RlcError
    try:
        pop.set_kernel(kernel)
    except (RlcError, RuntimeError):
        pop.close()
        if must:
            raise
        pytest.skip("the %s kernel does not take this shape" % kernel)
    assert pop.kernel_in_use() == kernel


def _check_grads(label, lay, dev, g32, g64, bar_of, zero=None, leave_out=()):
    """every gradient tensor of the layout: the elements listed in zero[name] exactly 0 on the device (and on both
    restatements), the rest `_held` at bar_of(name, size); a tensor the twin has all zero is all zero on the device"""
    zero = zero or {}
    for n, (off, shp) in lay.items():
        idx = np.arange(off, off + int(np.prod(shp)))
        if n in leave_out:
            continue
        if n in zero:
            z = off + np.asarray(zero[n])
            assert not np.any(g64[z]) and not np.any(g32[z]), (label, n)
            assert not np.any(dev[z]), (label, n, dev[z][np.nonzero(dev[z])][:4])
            idx = np.setdiff1d(idx, z)
            if idx.size == 0:
                continue
        if not np.any(g64[idx]):
            assert not np.any(dev[idx]), (label, n)
            continue
        C._held("%s grad %s" % (label, n), dev[idx], g32[idx], g64[idx], bar_of(n, idx.size))


# ================================================================================================ NAF
def _naf_pop(case, kernel, must=False, **kw):
    from rlcontrol_amd.hip_naf import NAFPopulation
    smin, smax, amax = C.naf_bounds(*case["dims"][:2])
    pop = NAFPopulation(1, *case["dims"], case["B"], 512, C.NAF_TAU, smin, smax, amax, C.NAF_LR, seeds=[3],
                        norm_type="layer" if case["norm"] else "input_norm", **kw)
    _select(pop, kernel, must)
    return pop


def _naf_bar(n, size):
    return C.NAF_GRAD_BAR


def _naf_first_update(label, case, pop, theta, batch, zero=None):
    """one update on the device, the fp32 restatement and the twin from theta; taps, gradients, target, beta powers"""
    pop.enable_grad_taps(True)
    pop.set_params(0, theta)
    o32, o64 = C.naf_restatement(case, theta), C.naf_restatement(case, theta, torch.float64)
    pop.update_batch(0, *batch)
    t32, t64 = o32.update(*batch, taps=True), o64.update(*batch, taps=True)
    for k in ("q", "y", "V"):
        C._held("%s %s" % (label, k), pop.last_tap(0, k), t32[k], t64[k], C.NAF_TAP_BAR)
    _check_grads(label, C.naf_layout(case)[0], pop.last_tap(0, "grads"), np.asarray(t32["grads"], np.float64), t64["grads"],
                 _naf_bar, zero)
    C._held("%s theta_target" % label, pop.get_blob(0, "theta_target"), _np(o32.theta_t), _np(o64.theta_t), C.NAF_TARGET_BAR)
    assert np.allclose(pop.get_beta_powers(0), o32.pw, rtol=1e-6)
    return o32, o64


NAF_MIXED_RUNS = [(n, k) for n in C.NAF_MIXED for k in C.NAF_CASES[n]["kernels"]]


@pytest.mark.parametrize("name,kernel", NAF_MIXED_RUNS)
def test_naf_mixed_gate_matches_the_restatement(hip_lib, name, kernel):
    """rows below -5, inside and above 5 in one minibatch (at least 1 / 8 of the (row, column) pairs each): a gate that
    is missing, always closed or read from another row or column misses the bar on Wd_c / bd_c by 100 x or more"""
    case = C.NAF_CASES[name]
    pop = _naf_pop(case, kernel, must=len(case["kernels"]) == 1)
    batch = C.naf_batch(C.CASE_SEEDS[name], case["B"], *case["dims"][:2])
    _naf_first_update("%s/%s" % (name, kernel), case, pop, C.naf_theta(case), batch)
    pop.close()


def _gated_slices(lay, names):
    return np.concatenate([np.arange(lay[n][0], lay[n][0] + int(np.prod(lay[n][1]))) for n in names])


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
def test_naf_all_clamped_heads_stay_exactly_where_they_are(hip_lib, kernel):
    """column 0 above 5 and column 1 below -5 in every row, by more than 2: the gradient tap of every Wd_c / bd_c is
    exactly 0, and after three updates their Adam moments are exactly 0 and their parameters bit for bit what was set"""
    name = "naf_all_clamped"
    case = C.NAF_CASES[name]
    lay = C.naf_layout(case)[0]
    gated = C.NAF_GATED(case["dims"][1])
    theta = C.naf_theta(case)
    batch = C.naf_batch(C.CASE_SEEDS[name], case["B"], *case["dims"][:2])
    pop = _naf_pop(case, kernel)
    zero = {n: np.arange(int(np.prod(lay[n][1]))) for n in gated}
    _naf_first_update("%s/%s" % (name, kernel), case, pop, theta, batch, zero)
    for _ in range(2):
        pop.update_batch(0, *batch)
        assert not np.any(pop.last_tap(0, "grads")[_gated_slices(lay, gated)])
    sl = _gated_slices(lay, gated)
    assert not np.any(pop.get_blob(0, "adam_m")[sl]) and not np.any(pop.get_blob(0, "adam_v")[sl])
    assert np.array_equal(_bits(pop.get_blob(0, "theta")[sl]), _bits(theta[sl]))
    rest = np.setdiff1d(np.arange(theta.size), sl)
    assert np.all(np.isfinite(pop.get_blob(0, "theta"))) and np.any(pop.get_blob(0, "theta")[rest] != theta[rest])
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("edge,out", [(5.0, np.inf), (-5.0, -np.inf)])
def test_naf_gate_is_inclusive_at_the_edge(hip_lib, kernel, edge, out):
    """Wd_0 = 0 and bd_0 exactly on the edge: the gradient passes (tf.clip_by_value is inclusive); one fp32 step outside:
    exactly 0"""
    c = C.NAF_BOUNDARY
    case = C._naf(c["dims"], c["B"])
    off = NafDims(*c["dims"]).layout()[0]["bd0"][0]
    batch = C.naf_batch(c["seed"], c["B"], *c["dims"][:2])
    pop = _naf_pop(case, kernel)
    pop.enable_grad_taps(True)
    for bias, inside in ((F32(edge), True), (np.nextafter(F32(edge), F32(out)), False)):
        theta = C.naf_boundary_theta(bias)
        pop.set_params(0, theta)
        pop.update_batch(0, *batch)
        got = pop.last_tap(0, "grads")[off]
        t32 = C.naf_restatement(case, theta).update(*batch, taps=True)["grads"][off]
        t64 = C.naf_restatement(case, theta, torch.float64).update(*batch, taps=True)["grads"][off]
        if inside:
            assert got != 0.0 and t64 != 0.0
            C._held("naf_boundary/%s bd0 at %+.1f" % (kernel, edge), got, t32, t64, C.NAF_GRAD_BAR)
        else:
            print("naf_boundary/%s bd0 one step outside %+.1f: device %r" % (kernel, edge, got))
            assert got == 0.0 and t32 == 0.0 and t64 == 0.0
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("name", ["naf_mixed_8x2x200x200_b32", "naf_mixed_3x1x64x48_b17", "naf_all_clamped"])
def test_naf_act_clamps_the_diagonal(hip_lib, name, kernel):
    """act(with_lcols=True) on weights whose diagonal heads leave [-5, 5]: naf_policy.h, row-major and tile-blocked"""
    case = C.NAF_CASES[name]
    theta = C.naf_theta(case)
    S, A = case["dims"][:2]
    states = C.naf_batch(C.CASE_SEEDS[name], case["B"], S, A)[0]
    pop = _naf_pop(case, kernel)
    pop.set_params(0, theta)
    smin, smax, amax = C.naf_bounds(S, A)
    o = NAFOracle(NafDims(*case["dims"]), theta, C.NAF_LR, C.NAF_TAU, smin, smax, amax)
    diag_at = np.cumsum([0] + [A - c for c in range(A - 1)])            # where column c's diagonal sits in the L columns
    logd = []
    for i in range(len(states)):
        mu, lc = pop.act(states[i:i + 1], with_lcols=True)
        wm, wl = o.act(states[i:i + 1])
        assert C.rel(mu, wm) < 1e-5 and C.rel(lc, wl) < 1e-5, (i, mu, wm, lc, wl)
        d = wl[0][diag_at]
        assert np.all(d >= F32(np.exp(-5.0)) * (1 - 1e-6)) and np.all(d <= F32(np.exp(5.0)) * (1 + 1e-6))
        assert np.allclose(lc[0][diag_at], d, rtol=1e-5)                # the diagonal on its own: small entries count too
        logd.append(np.log(d.astype(np.float64)))
    logd = np.concatenate(logd)
    assert np.any(np.abs(logd - 5.0) < 1e-5) and np.any(np.abs(logd + 5.0) < 1e-5)      # both clamps were active
    pop.close()


def test_naf_exploration_draw_clamps_the_diagonal(hip_lib):
    """the on-device loop up to its first update: with the diagonal head above 5 in at least a quarter of the steps
    (tests/clamp_cases.py, on NafRolloutOracle alone) the draw is mu + sqrt(noise_scale) z / e^5; without the clamp the
    stored actions would differ from the restatement's by about sqrt(noise_scale) |z| / 148"""
    from rlcontrol_amd.device_experiment import DeviceExperiment
    from rlcontrol_amd.hip_naf import NAFPopulation
    c = C.NAF_EXPLORE
    seed, total = C.CASE_SEEDS["naf_explore"], c["B"] + 2
    pop = NAFPopulation(1, *c["dims"], c["B"], 4096, 0.01, c["smin"], c["smax"], c["amax"], [c["lr"]], seeds=[seed])
    pop.set_params(0, C.naf_explore_theta(), init_target=True)
    env = {"environment": "Pendulum-v0", "TotalMilSteps": total / 1e6, "EpisodeSteps": c["limit"],
           "EvalIntervalMilSteps": 0.001, "EvalEpisodes": 1}
    assert int(env["TotalMilSteps"] * 1000000) == total
    exp = DeviceExperiment(pop, env, gamma=0.99, warmup_steps=0, noise_scale=c["noise"])
    exp.advance(1000)
    orc = C.naf_explore_oracle(seed).run()
    pre = c["B"] + 1
    assert pop.replay_size(0) == len(orc.replay) >= pre
    s, act, _, _, _ = pop.replay_gather(0, np.arange(pre))
    os_ = np.array([t[0] for t in orc.replay[:pre]])
    oa = np.array([t[1] for t in orc.replay[:pre]])
    print("naf_explore: states %.3e, actions %.3e" % (np.max(np.abs(s - os_)), np.max(np.abs(act - oa))))
    assert np.allclose(s, os_, atol=2e-6) and np.allclose(act, oa, atol=1e-5)
    pop.close()


# ================================================================================================ ReverseKL / ForwardKL
KL_RUN_MODES = [(k, o, "non_sac") for k, o in C.KL_MODES] + [("reverse", "intg", "sac")]
KL_TAPS = ("q", "v", "q_pi", "logp", "intgrl_q")


def _kl_pop(case, kind, optim, qup, kernel, must=False, dims=None, B=None):
    from rlcontrol_amd.hip_kl import KLPopulation
    pop = KLPopulation(kind, 1, *(dims or case["dims"]), B or case["B"], 2048, C.KL_TAU, C.KL_AMAX, C.KL_PI_LR, C.KL_QV_LR,
                       C.KL_ALPHA, seeds=[5], n_param=case["n_param"] or 64, optim_type=optim, q_update_type=qup,
                       l_param=case["l_param"], action_max=C.kl_action_max(case))
    _select(pop, kernel, must)
    return pop


def _kl_bar(case):
    def bar(n, size):
        if size == 1:
            return C.KL_GRAD1_BAR
        # above one action dimension the sparse grid's weights cancel: tests/test_kl.py holds the policy tensors to 3e-4
        return C.KL_GRAD1_BAR if (case["dims"][1] > 1 and n[0] == "p") else C.KL_GRAD_BAR
    return bar


def _kl_first_update(label, case, pop, theta, batch, kind, optim, qup, zero=None, leave_out=(), taps=KL_TAPS, loss=True):
    pop.enable_grad_taps(True)
    pop.set_params(0, theta)
    o32 = C.kl_restatement(case, theta, kind, optim, qup)
    o64 = C.kl_restatement(case, theta, kind, optim, qup, dtype=torch.float64)
    pop.update_batch(0, *batch[:5], eps=batch[5])
    t32, t64 = o32.update(*batch, taps=True), o64.update(*batch, taps=True)
    for k in taps:
        if k in t64:
            C._held("%s %s" % (label, k), pop.last_tap(0, k), t32[k], t64[k], C.KL_TAP_BAR)
    if loss:
        C._held("%s loss" % label, pop.last_tap(0, "loss"), t32["loss"], t64["loss"], C.KL_LOSS_BAR)
    lay = K.KlDims(*case["dims"]).layout()[0]
    _check_grads(label, lay, pop.last_tap(0, "grads"), np.asarray(t32["grads"], np.float64), t64["grads"], _kl_bar(case), zero,
                 leave_out)
    return o32, o64, t32, t64


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("kind,optim,qup", KL_RUN_MODES)
@pytest.mark.parametrize("name", C.KL_MIXED)
def test_kl_mixed_upper_gate_matches_the_restatement(hip_lib, name, kind, optim, qup, kernel):
    """rows inside and rows above log_std = 2 in one minibatch (at least 1 / 8 each): the gate of the likelihood path
    (ll, hard_ll) and of the integral path (intg, hard_intg, ForwardKL)"""
    case = C.KL_CASES[name]
    theta, batch = C.kl_theta(case), C.kl_case_batch(case, C.CASE_SEEDS[name])
    pop = _kl_pop(case, kind, optim, qup, kernel)
    label = "%s/%s/%s/%s/%s" % (name, kind, optim, qup, kernel)
    o32, o64, _, _ = _kl_first_update(label, case, pop, theta, batch, kind, optim, qup)
    C._held(label + " adam_m", pop.get_blob(0, "adam_m"), _np(o32.m), _np(o64.m), C.KL_GRAD_BAR)
    C._held(label + " adam_v", pop.get_blob(0, "adam_v"), _np(o32.v), _np(o64.v), C.KL_GRAD_BAR)
    vo = K.KlDims(*case["dims"]).layout()[0]["vW1"][0]
    C._held(label + " theta_target[V]", pop.get_blob(0, "theta_target")[vo:], _np(o32.theta_t)[vo:], _np(o64.theta_t)[vo:],
            C.KL_TAP_BAR)
    pop.close()


def _kl_zero(case, dims_above):
    """element indices of pWs [L2A, A] (row-major) and pbs [A] that belong to the action dimensions in dims_above"""
    L2A, A = case["dims"][3], case["dims"][1]
    return {"pWs": np.concatenate([np.arange(j, L2A * A, A) for j in dims_above]), "pbs": np.asarray(dims_above)}


def _kl_head_stays(pop, lay, theta, zero):
    sl = np.concatenate([lay[n][0] + zero[n] for n in ("pWs", "pbs")])
    assert not np.any(pop.get_blob(0, "adam_m")[sl]) and not np.any(pop.get_blob(0, "adam_v")[sl])
    assert np.array_equal(_bits(pop.get_blob(0, "theta")[sl]), _bits(theta[sl]))
    assert np.all(np.isfinite(pop.get_blob(0, "theta")))


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("kind,optim", C.KL_MODES)
def test_kl_all_above_head_stays_exactly_where_it_is(hip_lib, kind, optim, kernel):
    """every row above log_std = 2: the gradient tap of pWs / pbs is exactly 0; after three updates their Adam moments are
    exactly 0 and their parameters bit for bit what was set; the mean head and the trunk are at the bars"""
    name = "kl_all_above"
    case = C.KL_CASES[name]
    lay = K.KlDims(*case["dims"]).layout()[0]
    theta, batch = C.kl_theta(case), C.kl_case_batch(case, C.CASE_SEEDS[name])
    pop = _kl_pop(case, kind, optim, "non_sac", kernel)
    zero = _kl_zero(case, [0])
    _kl_first_update("%s/%s/%s/%s" % (name, kind, optim, kernel), case, pop, theta, batch, kind, optim, "non_sac", zero)
    for _ in range(2):
        pop.update_batch(0, *batch[:5], eps=batch[5])
        assert not np.any(pop.last_tap(0, "grads")[lay["pWs"][0] + zero["pWs"]]) and pop.last_tap(0, "grads")[lay["pbs"][0]] == 0.0
    assert pop.get_step(0) == 3
    _kl_head_stays(pop, lay, theta, zero)
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("kind,optim", C.KL_MODES)
def test_kl_all_below_gate_closes_and_nothing_overflows(hip_lib, kind, optim, kernel):
    """Every raw log_std below -20 by more than 1.  The pWs / pbs gradient tap is exactly 0, q, v and the Q / V gradient
    tensors are at the bars, every tap is finite wherever the restatement's is.

    No policy-gradient parity here: with std = e^-20 the draw mean + std eps equals mean in fp32, z - mean is below one
    ulp of mean and 1 / var = e^40 turns that rounding into the gradient; ForwardKL's loss is 8e16 there, and ReverseKL's
    integral has an all-zero policy gradient because the quadrature misses the spike.  The first update takes eps = 0, where
    z = mean in every precision and the log density (which the V target reads) is well conditioned; the second takes
    standard normal draws and is checked for the closed gate and for finiteness only."""
    name = "kl_all_below"
    case = C.KL_CASES[name]
    lay = K.KlDims(*case["dims"]).layout()[0]
    theta, batch = C.kl_theta(case), C.kl_case_batch(case, C.CASE_SEEDS[name])
    assert not np.any(batch[5])
    pop = _kl_pop(case, kind, optim, "non_sac", kernel)
    label = "%s/%s/%s/%s" % (name, kind, optim, kernel)
    policy = [n for n in lay if n[0] == "p" and n not in C.KL_GATED]
    o32, _, t32, _ = _kl_first_update(label, case, pop, theta, batch, kind, optim, "non_sac", _kl_zero(case, [0]), leave_out=policy,
                                      taps=("q", "v"), loss=False)
    gated = np.concatenate([lay[n][0] + np.arange(int(np.prod(lay[n][1]))) for n in C.KL_GATED])

    def finite_where_the_restatement_is(t):
        for k in KL_TAPS + ("loss", "grads"):
            if k in t:
                ok = np.isfinite(t[k])
                assert np.all(np.isfinite(pop.last_tap(0, k)[ok])), (label, k)
    finite_where_the_restatement_is(t32)
    noisy = C.kl_batch(C.CASE_SEEDS[name] + 100, case["B"], case["dims"][0], 1)
    noisy = noisy[:5] + (np.random.RandomState(C.CASE_SEEDS[name]).randn(case["B"], 1),)
    pop.update_batch(0, *noisy[:5], eps=noisy[5])
    finite_where_the_restatement_is(o32.update(*noisy, taps=True))
    assert not np.any(pop.last_tap(0, "grads")[gated])
    pop.close()


@pytest.mark.parametrize("kernel", ["generic", "mfma"])
@pytest.mark.parametrize("kind,optim", C.KL_BOUNDARY["modes"])
@pytest.mark.parametrize("edge,out", [(2.0, np.inf), (-20.0, -np.inf)])
def test_kl_gate_is_inclusive_at_the_edge(hip_lib, kind, optim, edge, out, kernel):
    """pWs = 0 and pbs exactly on the edge: the gradient passes (torch.clamp is inclusive) -- at the bar at +2, with the
    restatement's sign at -20 (no parity at the lower clamp); one fp32 step outside: exactly 0"""
    c = C.KL_BOUNDARY
    case = C._kl(c["dims"], c["B"], 0.0, (edge,), ("edge",), n_param=c["n_param"])
    off = K.KlDims(*c["dims"]).layout()[0]["pbs"][0]
    batch = C.kl_batch(c["seed"], c["B"], c["dims"][0], 1, c["eps_width"][edge])
    pop = _kl_pop(case, kind, optim, "non_sac", kernel)
    pop.enable_grad_taps(True)
    label = "kl_boundary/%s/%s/%s pbs" % (kind, optim, kernel)
    for bias, inside in ((F32(edge), True), (np.nextafter(F32(edge), F32(out)), False)):
        theta = C.kl_boundary_theta(bias)
        pop.set_params(0, theta)
        pop.update_batch(0, *batch[:5], eps=batch[5])
        got = pop.last_tap(0, "grads")[off]
        t32 = C.kl_restatement(case, theta, kind, optim).update(*batch, taps=True)["grads"][off]
        t64 = C.kl_restatement(case, theta, kind, optim, dtype=torch.float64).update(*batch, taps=True)["grads"][off]
        if not inside:
            print("%s one step outside %+.1f: device %r" % (label, edge, got))
            assert got == 0.0 and t32 == 0.0 and t64 == 0.0
        elif edge > 0:
            assert got != 0.0 and t64 != 0.0
            C._held("%s at %+.1f" % (label, edge), got, t32, t64, C.KL_GRAD1_BAR)
        else:
            print("%s at %+.1f: device %.6e, restatement %.6e, twin %.6e" % (label, edge, got, t32, t64))
            assert got != 0.0 and np.isfinite(got) and np.sign(got) == np.sign(t32) == np.sign(t64)
    pop.close()


KL_ACTION2 = [n for n in C.KL_CASES if n.startswith("kl_action2")]


@pytest.mark.parametrize("kind,optim", C.KL_MODES)
@pytest.mark.parametrize("name", KL_ACTION2)
def test_kl_action2_gate_is_per_dimension(hip_lib, name, kind, optim):
    """two action dimensions, one above log_std = 2 in every row and the other inside in every row (both assignments): the
    column of pWs and the entry of pbs of the clamped dimension are exactly 0, the other column is at the bars -- a gate
    read from dimension 0 for both fails one of the two assignments"""
    case = C.KL_CASES[name]
    above = [j for j, w in enumerate(case["want"]) if w == "all-above"]
    assert len(above) == 1
    theta, batch = C.kl_theta(case), C.kl_case_batch(case, C.CASE_SEEDS[name])
    kernel = case["kernels"][0]
    pop = _kl_pop(case, kind, optim, "non_sac", kernel, must=True)
    assert pop.n_nodes == len(C.kl_restatement(case, theta, kind, optim).weights)
    _kl_first_update("%s/%s/%s" % (name, kind, optim), case, pop, theta, batch, kind, optim, "non_sac", _kl_zero(case, above))
    pop.close()


KL_ACT = [("kl_mixed_upper_s1", "generic"), ("kl_mixed_upper_s1", "mfma"), ("kl_all_above", "generic"), ("kl_all_above", "mfma"),
          ("kl_all_below", "generic"), ("kl_all_below", "mfma"), ("kl_action2_generic_0above", "generic"),
          ("kl_action2_mfma_1above", "mfma")]


@pytest.mark.parametrize("name,kernel", KL_ACT)
def test_kl_act_clamps_log_std(hip_lib, name, kernel):
    """the mean action and the sampled action with injected eps (sac_policy.h with clamp_ls = 1; above one action dimension
    the reference's sqrt(std) scale) on weights whose log_std head leaves [-20, 2]"""
    case = C.KL_CASES[name]
    S, A = case["dims"][:2]
    theta = C.kl_theta(case)
    pop = _kl_pop(case, "reverse", "intg", "non_sac", kernel, must=A > 1)
    pop.set_params(0, theta)
    o = C.kl_restatement(case, theta, "reverse", "intg")
    states = C.kl_case_batch(case, C.CASE_SEEDS[name])[0][:8]
    eps = np.random.RandomState(C.CASE_SEEDS[name] + 7).randn(len(states), A)
    for i in range(len(states)):
        st, e = states[i:i + 1], eps[i:i + 1]
        assert C.rel(pop.act(st), o.act(st)) < 1e-5, i
        got, want = pop.act(st, sample=True, eps=e), o.act(st, eps=e)
        assert C.rel(got, want) < 1e-4, (i, got, want)
    pop.close()


def test_kl_latency_mode_gates_like_one_workgroup(hip_lib):
    """kl_mixed_upper's first shape with the node passes dealt over 8 workgroups against the one-workgroup run: the
    comparison of tests/test_kl.py::test_kl_latency_mode_equals_one_workgroup after one update from equal parameters"""
    name = "kl_mixed_upper_s1"
    case = C.KL_CASES[name]
    theta, batch = C.kl_theta(case), C.kl_case_batch(case, C.CASE_SEEDS[name])
    lay = K.KlDims(*case["dims"]).layout()[0]
    pops = []
    for split in (1, 8):
        pop = _kl_pop(case, "reverse", "intg", "non_sac", "mfma")
        pop.enable_grad_taps(True)
        pop.set_params(0, theta)
        pop.set_split(split)
        pop.update_batch(0, *batch[:5], eps=batch[5])
        pops.append(pop)
    one, many = pops
    assert np.array_equal(one.last_tap(0, "intgrl_q"), many.last_tap(0, "intgrl_q"))
    for k in ("q", "v", "q_pi", "logp", "loss"):
        assert C.rel(many.last_tap(0, k), one.last_tap(0, k)) < 1e-5, k
    g1, g8 = one.last_tap(0, "grads"), many.last_tap(0, "grads")
    for n in C.KL_GATED:
        off, shp = lay[n]
        k = int(np.prod(shp))
        print("kl_split %s: %.3e" % (n, C.rel(g8[off:off + k], g1[off:off + k])))
        assert C.rel(g8[off:off + k], g1[off:off + k]) < 1e-5, n
    for blob in ("theta", "theta_target", "adam_m", "adam_v"):
        x, y = one.get_blob(0, blob).astype(np.float64), many.get_blob(0, blob).astype(np.float64)
        assert np.max(np.abs(x - y)) <= 3e-5 * np.max(np.abs(x)) + 1e-9, blob
    for pop in pops:
        pop.close()
