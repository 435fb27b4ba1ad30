"""CPU: the inputs of tests/test_gpu_clamp_gates.py meet their conditions on the restatements alone (tests/clamp_cases.py),
the three restatements pass the gradient AT a clamp edge and stop it one fp32 step outside, and oracle/kl_torch.py's dtype
argument leaves its float32 arithmetic bit for bit what it was."""
import hashlib

import numpy as np
import pytest
import torch

import clamp_cases as C
from oracle import kl_torch as K
from oracle.naf import NafDims

F32 = np.float32


# ------------------------------------------------------------------------------------------ the search and its record
def test_every_case_has_a_recorded_seed():
    assert sorted(C.CASE_SEEDS) == sorted(list(C.NAF_CASES) + list(C.KL_CASES) + ["naf_explore"])
    assert set(C.NAF_MIXED) | set(C.KL_MIXED) <= set(C.CASE_SEEDS) and len(C.NAF_MIXED) == 6 and len(C.KL_MIXED) == 2


@pytest.mark.parametrize("name", sorted(C.CASE_SEEDS))
def test_recorded_seed_is_the_first_that_meets_the_conditions(name):
    """find_seed walks the case's short list and returns the first seed whose minibatch meets (a) to (e) on the
    restatements (a seed it returns has an empty list of failures); at most half of the list may be left out before it"""
    seeds = C.seed_list(name)
    found = C.find_seed(name)
    assert found is not None, "no seed of %r meets the conditions" % (seeds,)
    assert found == C.CASE_SEEDS[name]
    assert seeds.index(found) <= len(seeds) // 2, (found, seeds)


@pytest.mark.parametrize("name", ["naf_mixed_3x1x64x48_b17", "naf_mixed_layer_5x3x32x40_b9", "kl_mixed_upper_s1"])
def test_conditions_reject_what_they_are_there_to_reject(name):
    """the same case with its recipe undone (weights as initialised) fails the share condition, and the sensitivity of a
    minibatch that never leaves the open interval is zero: the search can say no"""
    naf = name in C.NAF_CASES
    case = dict((C.NAF_CASES if naf else C.KL_CASES)[name])
    if naf:
        case.update(scale=1.0, shift=(0.0,) * case["dims"][1])
        out = C.naf_failures(case, C.CASE_SEEDS[name])
        ratio = C.case_sensitivity(case, C.CASE_SEEDS[name])
    else:
        case.update(ws_scale=30.0, pbs=(0.0,))
        out = C.kl_failures(case, C.CASE_SEEDS[name])
        ratio = C.case_sensitivity(case, C.CASE_SEEDS[name])
    assert any(f.split(":")[0].endswith("b") for f in out), out
    assert ratio < 1e-3, ratio


@pytest.mark.parametrize("name", C.NAF_MIXED + C.KL_MIXED)
def test_mixed_cases_tell_a_missing_gate_from_the_true_backward(name):
    """condition (d), stated on its own and printed: how many bars a gate-less backward misses the true one by"""
    ratio = C.case_sensitivity((C.NAF_CASES if name in C.NAF_CASES else C.KL_CASES)[name], C.CASE_SEEDS[name])
    print("%s: a gate-less backward misses by %.3g bars" % (name, ratio))
    assert ratio >= C.SENSITIVITY


def test_gate_removed_keeps_the_forward_and_passes_the_gradient():
    x = torch.tensor([-7.0, -5.0, 0.5, 5.0, 7.0], dtype=torch.float64, requires_grad=True)
    with C.gate_removed():
        y = torch.clamp(x, -5.0, 5.0)
    assert torch.equal(y.detach(), torch.tensor([-5.0, -5.0, 0.5, 5.0, 5.0], dtype=torch.float64))
    y.sum().backward()
    assert torch.equal(x.grad, torch.ones(5, dtype=torch.float64))
    assert torch.clamp(torch.tensor(9.0), -5.0, 5.0).item() == 5.0            # and the real one is back


# ------------------------------------------------------------------------------------------ boundary semantics
def test_torch_clamp_is_inclusive_at_both_edges():
    """tf.clip_by_value (the reference's NAF) and torch.clamp (its KL agents) pass the gradient at equality"""
    x = torch.tensor([-5.0, float(np.nextafter(F32(-5.0), F32(-np.inf))), 5.0, float(np.nextafter(F32(5.0), F32(np.inf)))],
                     requires_grad=True)
    torch.clamp(x, -5.0, 5.0).sum().backward()
    assert x.grad.tolist() == [1.0, 0.0, 1.0, 0.0]


def _naf_bias_gradient(kind, bias):
    c = C.NAF_BOUNDARY
    case = C._naf(c["dims"], c["B"])
    theta = C.naf_boundary_theta(bias)
    assert theta[NafDims(*c["dims"]).layout()[0]["bd0"][0]] == F32(bias)
    batch = C.naf_batch(c["seed"], c["B"], *c["dims"][:2])
    t = C.naf_restatement(case, theta, torch.float32 if kind == "c" else torch.float64).update(*batch, taps=True)
    return t["grads"][NafDims(*c["dims"]).layout()[0]["bd0"][0]]


@pytest.mark.parametrize("kind", ["c", "torch"])
@pytest.mark.parametrize("edge,out", [(5.0, np.inf), (-5.0, -np.inf)])
def test_naf_restatements_gate_inclusively(kind, edge, out):
    """oracle/naf_oracle.c (fp32) and TorchNAF (float64): bias exactly on the edge -> the gradient passes; one fp32 step
    outside -> exactly zero"""
    on = _naf_bias_gradient(kind, F32(edge))
    off = _naf_bias_gradient(kind, np.nextafter(F32(edge), F32(out)))
    print("NAF %s bd0 gradient at %+.1f: %.6e, one step outside: %.1e" % (kind, edge, on, off))
    assert on != 0.0 and np.isfinite(on) and off == 0.0


def _kl_bias_gradient(kind, optim, bias, edge, dtype=torch.float32):
    c = C.KL_BOUNDARY
    d = K.KlDims(*c["dims"])
    theta = C.kl_boundary_theta(bias)
    o = K.KLOracle(kind, d, theta, C.KL_PI_LR, C.KL_QV_LR, C.KL_ALPHA, C.KL_TAU, C.KL_AMAX, c["n_param"], optim, dtype=dtype)
    t = o.update(*C.kl_batch(c["seed"], c["B"], c["dims"][0], 1, c["eps_width"][edge]), taps=True)
    return t["grads"][d.layout()[0]["pbs"][0]]


@pytest.mark.parametrize("kind,optim", C.KL_BOUNDARY["modes"])
@pytest.mark.parametrize("edge,out", [(2.0, np.inf), (-20.0, -np.inf)])
def test_kl_restatement_gates_inclusively(kind, optim, edge, out):
    on = _kl_bias_gradient(kind, optim, F32(edge), edge)
    off = _kl_bias_gradient(kind, optim, np.nextafter(F32(edge), F32(out)), edge)
    print("KL %s/%s pbs gradient at %+.1f: %.6e, one step outside: %.1e" % (kind, optim, edge, on, off))
    assert on != 0.0 and np.isfinite(on) and off == 0.0


# ------------------------------------------------------------------------------------------ oracle/kl_torch.py dtype
MODES = ([("reverse", o, q) for o in K.OPTIM_TYPES for q in K.Q_UPDATE_TYPES] + [("forward", "intg", q) for q in K.Q_UPDATE_TYPES])
# sha256 (first 16 hex digits) over every tap of one update and theta, theta_target, adam_m, adam_v after it, recorded
# from oracle/kl_torch.py as it was before the dtype argument
FLOAT32_DIGESTS = dict(zip(MODES, ("b36e82cb3e2e21b6", "84de3ca33e2f1927", "34c371eb9e575a83", "ccd032fe3e680b46", "e72eccac904e4720",
                                   "30a0d55d936b5d61", "f5e8ba471ade97ed", "74045317c7c42a6d", "ce5817362ba73379", "f6b879c36b636189")))


def _one_update(kind, optim, qup, **kw):
    dims, B = (3, 1, 16, 16, 16, 16), 8
    d = K.KlDims(*dims)
    rng = np.random.RandomState(11)
    th = K.init_params(d, 5)
    lay, _ = d.layout()
    for name in ("pWm", "pWs", "qW3", "vW3"):
        off, shp = lay[name]
        th[off:off + int(np.prod(shp))] *= 30.0
    o = K.KLOracle(kind, d, th, 1e-3, 1e-2, 0.3, 0.01, 2.0, 9, optim, qup, **kw)
    s, a, s2 = rng.uniform(-2, 2, (B, 3)), rng.uniform(-2, 2, (B, 1)), rng.uniform(-2, 2, (B, 3))
    r, g, eps = rng.uniform(-16, 0, B), np.where(rng.rand(B) < 0.2, 0.0, 0.99), rng.randn(B, 1)
    return o, o.update(s, a, s2, r, g, eps, taps=True)


@pytest.mark.parametrize("kind,optim,qup", MODES)
def test_kl_torch_float32_is_bit_for_bit_what_it_was(kind, optim, qup):
    for kw in ({}, {"dtype": torch.float32}):
        o, t = _one_update(kind, optim, qup, **kw)
        h = hashlib.sha256()
        for k in sorted(t):
            assert t[k].dtype == np.float32, k
            h.update(t[k].tobytes())
        for x in (o.theta, o.theta_t, o.m, o.v):
            assert x.dtype == torch.float32
            h.update(x.numpy().tobytes())
        assert h.hexdigest()[:16] == FLOAT32_DIGESTS[(kind, optim, qup)]


@pytest.mark.parametrize("kind,optim,qup", MODES)
def test_kl_torch_float64_twin_follows_the_float32_run(kind, optim, qup):
    o32, t32 = _one_update(kind, optim, qup)
    o64, t64 = _one_update(kind, optim, qup, dtype=torch.float64)
    assert o64.theta.dtype == o64.m.dtype == o64.nodes.dtype == o64.weights.dtype == torch.float64
    assert torch.equal(o64.nodes, o32.nodes.double()) and torch.equal(o64.weights, o32.weights.double())   # rounded first
    for k in t64:
        assert t64[k].dtype == np.float64 and t64[k].shape == t32[k].shape, k
        assert C.rel(t32[k], t64[k]) < (1e-5 if k != "grads" else 3e-4), k
    st = np.random.RandomState(0).uniform(-2, 2, (4, 3))
    assert C.rel(o32.act(st), o64.act(st)) < 1e-5
