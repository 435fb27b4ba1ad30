"""Inputs shared by tests/test_clamp_cases.py (CPU) and tests/test_gpu_clamp_gates.py: the weight recipes that drive the
NAF diagonal heads past clip(., -5, 5) and the KL log_std head past clamp(., -20, 2), the conditions those inputs meet on
the restatements alone, the search for a minibatch seed that meets them, and the seeds it found.

Conditions ("Clamp gates"):
  (a) margin       every gated pre-activation is at least MARGIN from both clamp edges (boundary cases sit on an edge
                   exactly, by construction, and are not searched)
  (b) share        mixed cases: at least SHARE of the gated elements in each region the case is about
  (c) ReLU kinks   no hidden pre-activation of a differentiated network within KINK of zero
  (d) sensitivity  mixed cases: the float64 twin with the gate removed (x + (clamp(x) - x).detach(): same forward,
                   straight-through backward) differs from the true twin by at least SENSITIVITY x the bar on every
                   gated tensor
  (e) squash       KL: every draw z of the minibatch keeps 1 - tanh(z)^2 >= SQUASH_FLOOR, so that the squash correction
                   log(1 - tanh(z)^2 + 1e-6) is well conditioned in fp32
"""
import contextlib
from unittest import mock

import numpy as np
import torch

from oracle import kl_torch as K
from oracle.naf import NAFOracle, NafDims, init_params as naf_init_params
from oracle.naf_variants import NafVariantOracle, init_params as naf_variant_init, layout as naf_variant_layout
from torch_ref_naf import TorchNAF

MARGIN, SHARE, KINK, SENSITIVITY = 1e-3, 1.0 / 8.0, 1.5e-6, 100.0
SEED_LIST = (1, 2, 3, 4, 5, 6, 7, 8)       # a case may leave out at most the first half of it

# the bars the agents already carry (tests/test_naf.py, tests/test_kl.py)
NAF_TAP_BAR, NAF_GRAD_BAR, NAF_TARGET_BAR = 1e-5, 2e-5, 1e-5
KL_TAP_BAR, KL_GRAD_BAR, KL_GRAD1_BAR, KL_LOSS_BAR = 1e-5, 5e-5, 3e-4, 1e-4

NAF_LO, NAF_HI = -5.0, 5.0
KL_LO, KL_HI = K.LOG_STD_MIN, K.LOG_STD_MAX


def rel(x, y):
    x, y = np.asarray(x, np.float64).ravel(), np.asarray(y, np.float64).ravel()
    return float(np.max(np.abs(x - y)) / (np.max(np.abs(y)) + 1e-30))


def _held(label, dev, ref32, twin, bar):
    """device against the twin <= max(bar, 3 x the fp32 restatement against the twin)  (tests/test_gpu_ae.py)"""
    e_dev, e_ref = rel(dev, twin), rel(ref32, twin)
    bound = max(bar, 3.0 * e_ref)
    print("%s: device %.3e, restatement %.3e, bound %.3e" % (label, e_dev, e_ref, bound))
    assert e_dev <= bound, (label, e_dev, e_ref, bound)
    return e_dev


@contextlib.contextmanager
def gate_removed():
    """every torch.clamp of the restatements (the gates are their only ones) keeps its forward value and passes the
    gradient straight through"""
    real = torch.clamp

    def straight_through(x, lo, hi):
        return x + (real(x, lo, hi) - x).detach()
    with mock.patch.object(torch, "clamp", straight_through):
        yield


def regions(pre, lo, hi):
    """shares (below, inside, above) of the elements of pre, and the distance of the nearest one from an edge"""
    pre = np.asarray(pre, np.float64)
    n = float(pre.size)
    return (np.sum(pre < lo) / n, np.sum((pre >= lo) & (pre <= hi)) / n, np.sum(pre > hi) / n,
            float(min(np.min(np.abs(pre - lo)), np.min(np.abs(pre - hi)))))


def _region_failures(pre, lo, hi, want):
    """conditions (a) and (b) on one set of gated pre-activations; want: shares that must reach SHARE (a subset of
    'below', 'inside', 'above') or a single region written 'all-below' / 'all-inside' / 'all-above'"""
    below, inside, above, nearest = regions(pre, lo, hi)
    share = {"below": below, "inside": inside, "above": above}
    out = []
    if nearest < MARGIN:
        out.append("a: a pre-activation %.3e from a clamp edge" % nearest)
    if isinstance(want, str):
        if share[want[4:]] != 1.0:
            out.append("b: not every element %s (%.2f / %.2f / %.2f)" % (want[4:], below, inside, above))
    else:
        for k in want:
            if share[k] < SHARE:
                out.append("b: share %s %.3f" % (k, share[k]))
    return out


# ================================================================================================ NAF
NAF_LR, NAF_TAU = 1e-3, 0.01
NAF_INIT_SEED = 2
NAF_GATED = lambda A: ["%s%d" % (w, c) for c in range(A) for w in ("Wd", "bd")]


def naf_bounds(S, A):
    return -np.ones(S) * 2, np.ones(S) * 2, np.linspace(1.0, 2.0, A)


def naf_batch(seed, B, S, A):
    """the minibatch of tests/test_naf.py, from RandomState(seed)"""
    rng = np.random.RandomState(seed)
    return (rng.uniform(-3, 3, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-3, 3, (B, S)),
            rng.uniform(-16, 0, B), np.where(rng.rand(B) < 0.2, 0.0, 0.99))


def _naf(dims, B, scale=1.0, shift=None, norm=False, want=("below", "inside", "above"), kernels=("generic", "mfma")):
    return dict(dims=dims, B=B, scale=float(scale), shift=tuple(shift) if shift is not None else (0.0,) * dims[1], norm=norm,
                want=want, kernels=kernels)


# Recipe of a case: from init_params(dims, NAF_INIT_SEED) every Wd_c is multiplied by `scale` and every bd_c set to
# shift[c].  The diagonal heads read h1 >= 0, so a one-column head needs a bias shift to reach below -5 as well.
NAF_CASES = {
    "naf_mixed_8x2x200x200_b32": _naf((8, 2, 200, 200), 32, 40.0),
    "naf_mixed_8x2x200x200_b97": _naf((8, 2, 200, 200), 97, 40.0, kernels=("mfma",)),          # tail of four
    "naf_mixed_3x1x64x48_b17": _naf((3, 1, 64, 48), 17, 40.0, (-10.0,)),
    "naf_mixed_5x3x32x40_b9": _naf((5, 3, 32, 40), 9, 20.0, kernels=("generic",)),
    "naf_mixed_wide_3x3x64x48_b17": _naf((3, 3, 64, 48), 17, 40.0, kernels=("mfma",)),         # the wide MFMA form
    "naf_mixed_layer_5x3x32x40_b9": _naf((5, 3, 32, 40), 9, 20.0, norm=True, kernels=("generic",)),
    # every element outside, by more than 2: column 0 above, column 1 below; weights as initialised
    "naf_all_clamped": _naf((8, 2, 64, 48), 17, 1.0, (8.0, -8.0), want=None),
}
NAF_MIXED = [k for k in NAF_CASES if k.startswith("naf_mixed")]
NAF_BOUNDARY = dict(dims=(3, 1, 16, 16), B=8, seed=1)


def naf_layout(case):
    return naf_variant_layout(case["dims"], case["norm"])


def naf_theta(case):
    dims, lay = case["dims"], naf_layout(case)[0]
    if case["norm"]:
        th = naf_variant_init(dims, NAF_INIT_SEED, True)
        rng = np.random.RandomState(NAF_INIT_SEED + 100)       # gammas / betas off their 1 / 0 defaults (tests/test_naf.py)
        for n, (off, shp) in lay.items():
            if n.startswith("L"):
                th[off:off + shp[0]] += rng.uniform(-0.2, 0.2, shp[0]).astype(np.float32)
    else:
        th = naf_init_params(NafDims(*dims), NAF_INIT_SEED)
    for c in range(dims[1]):
        off, shp = lay["Wd%d" % c]
        th[off:off + shp[0]] *= np.float32(case["scale"])
        th[lay["bd%d" % c][0]] = case["shift"][c]
    return th


def naf_boundary_theta(bias):
    """Wd_0 = 0 and bd_0 = bias: the diagonal pre-activation is the bias itself in every row, on every implementation"""
    d = NafDims(*NAF_BOUNDARY["dims"])
    th, lay = naf_init_params(d, NAF_INIT_SEED), d.layout()[0]
    off, shp = lay["Wd0"]
    th[off:off + shp[0]] = 0.0
    th[lay["bd0"][0]] = np.float32(bias)
    return th


def naf_restatement(case, theta, dtype=torch.float32):
    """fp32: the oracle the kernels are held to (oracle/naf_oracle.c, naf_variants.py under layer norm); float64: its
    twin (TorchNAF, naf_variants.py in float64).  Both return update(...) taps with a flat `grads`."""
    smin, smax, amax = naf_bounds(*case["dims"][:2])
    if case["norm"]:
        return NafVariantOracle(case["dims"], theta, NAF_LR, NAF_TAU, smin, smax, amax, norm_type="layer", dtype=dtype)
    if dtype == torch.float32:
        return NAFOracle(NafDims(*case["dims"]), theta, NAF_LR, NAF_TAU, smin, smax, amax)
    return _FlatTorchNAF(case["dims"], theta, NAF_LR, NAF_TAU, smin, smax, amax)


class _FlatTorchNAF(TorchNAF):
    """TorchNAF with the taps of the other restatements: grads as one flat blob in the layout's order"""

    def update(self, s, a, s2, r, gam, taps=True):
        t = TorchNAF.update(self, s, a, s2, r, gam)
        t["grads"] = np.concatenate([t["grads"][n].reshape(-1) for n in self.names])
        return t

    @property
    def theta_t(self):
        return self.blob(True)


def naf_preacts(case, theta, s):
    """(diagonal pre-activations [B, A] in front of clip(., -5, 5), the smallest |hidden pre-activation| in front of a
    ReLU) of the online network on the fp32 restatement (oracle/naf_variants.py's forward, taken apart)"""
    smin, smax, amax = naf_bounds(*case["dims"][:2])
    o = NafVariantOracle(case["dims"], theta, NAF_LR, NAF_TAU, smin, smax, amax,
                         norm_type="layer" if case["norm"] else "input_norm")
    S, A = case["dims"][:2]

    def pre_relu(P, tag, z):
        if o.norm:
            mean = z.mean(-1, keepdim=True)
            var = ((z - mean) ** 2).mean(-1, keepdim=True)
            z = (z - mean) / torch.sqrt(var + 1e-12) * P["L%sg" % tag] + P["L%sb" % tag]
        return z
    with torch.no_grad():
        P = o._views(o.theta)
        x = o._clip(o._t(s, (-1, S)))
        z1 = pre_relu(P, "1", x @ P["W1"] + P["b1"])
        h1 = torch.relu(z1)
        za = pre_relu(P, "a2", h1 @ P["Wa2"] + P["ba2"])
        zv = pre_relu(P, "v2", h1 @ P["Wv2"] + P["bv2"])
        diag = torch.cat([h1 @ P["Wd%d" % c] + P["bd%d" % c] for c in range(A)], 1)
        kink = min(z.abs().min().item() for z in (z1, za, zv))
    return diag.numpy().astype(np.float64), kink


def naf_sensitivity(case, theta, batch):
    """condition (d): over the gated tensors, the smallest (twin without the gate against the true twin) / bar"""
    true = naf_restatement(case, theta, torch.float64).update(*batch, taps=True)["grads"]
    with gate_removed():
        loose = naf_restatement(case, theta, torch.float64).update(*batch, taps=True)["grads"]
    lay = naf_layout(case)[0]
    worst = float("inf")
    for n in NAF_GATED(case["dims"][1]):
        off, shp = lay[n]
        sl = slice(off, off + int(np.prod(shp)))
        worst = min(worst, rel(loose[sl], true[sl]) / NAF_GRAD_BAR)
    return worst


def naf_failures(case, seed):
    """conditions (a) to (d) for the minibatch of RandomState(seed); [] when all hold"""
    S, A = case["dims"][:2]
    theta, batch = naf_theta(case), naf_batch(seed, case["B"], S, A)
    diag, kink = naf_preacts(case, theta, batch[0])
    out = []
    if case["want"] is None:                                       # naf_all_clamped: column 0 above, column 1 below, by > 2
        if not (np.all(diag[:, 0] > NAF_HI + 2.0) and np.all(diag[:, 1] < NAF_LO - 2.0)):
            out.append("b: an element within 2 of the open interval")
    else:
        out += _region_failures(diag, NAF_LO, NAF_HI, case["want"])
    if kink < KINK:
        out.append("c: a hidden pre-activation %.3e from zero" % kink)
    if case["want"] is not None and not out:
        ratio = case_sensitivity(case, seed)
        if ratio < SENSITIVITY:
            out.append("d: the gate moves a gated tensor by %.1f bars only" % ratio)
    return out


# ---- the exploration draw of the on-device loop (naf_policy.h clamps the diagonal again)
NAF_EXPLORE = dict(dims=(3, 1, 32, 32), B=16, init_seed=40, scale=60.0, shift=2.0, noise=1.0, lr=1e-3, seed_list=(8, 9, 10, 11),
                   smin=[-1, -1, -8], smax=[1, 1, 8], amax=[2.0], limit=25)


def naf_explore_theta():
    c = NAF_EXPLORE
    d = NafDims(*c["dims"])
    th, lay = naf_init_params(d, c["init_seed"]), d.layout()[0]
    off, shp = lay["Wd0"]
    th[off:off + shp[0]] *= np.float32(c["scale"])
    th[lay["bd0"][0]] = c["shift"]
    return th


def naf_explore_oracle(seed):
    """NafRolloutOracle of one agent, run just past its first update (B + 2 training steps, no evaluation in between)"""
    from oracle.rollout import NafRolloutOracle
    c = NAF_EXPLORE
    total = c["B"] + 2
    return NafRolloutOracle(NafDims(*c["dims"]), naf_explore_theta(), c["lr"], 0.01, c["smin"], c["smax"], c["amax"], c["noise"],
                            seed, c["B"], 4096, 0.99, 0, c["limit"], total, 1000, 1)


def naf_explore_failures(seed):
    """on the restatement alone: at least a quarter of the first B + 1 training states have the diagonal pre-activation
    above 5 and every one of them keeps MARGIN from both edges.  Above 5 the draw is mu + sqrt(noise_scale) z / e^5; without
    the clamp it would be nearer mu by about sqrt(noise_scale) |z| / 148, hundreds of times the 1e-5 the draws are held to"""
    c = NAF_EXPLORE
    orc = naf_explore_oracle(seed).run()
    pre = c["B"] + 1
    states = np.array([t[0] for t in orc.replay[:pre]])
    diag = _explore_diag(naf_explore_theta(), states, (c["smin"], c["smax"]))
    below, inside, above, nearest = regions(diag, NAF_LO, NAF_HI)
    out = []
    if nearest < MARGIN:
        out.append("a: a pre-activation %.3e from a clamp edge" % nearest)
    if above < 0.25:
        out.append("b: share above %.3f" % above)
    return out


def _explore_diag(theta, states, bounds):
    d = NafDims(*NAF_EXPLORE["dims"])
    lay = d.layout()[0]
    S, A, L1, L2 = d.t
    f = np.float32
    x = np.clip(np.asarray(states, np.float32), np.asarray(bounds[0], f), np.asarray(bounds[1], f))
    W1 = theta[lay["W1"][0]:lay["W1"][0] + S * L1].reshape(S, L1)
    b1 = theta[lay["b1"][0]:lay["b1"][0] + L1]
    h1 = np.maximum(x @ W1 + b1, 0)
    Wd = theta[lay["Wd0"][0]:lay["Wd0"][0] + L1]
    return (h1 @ Wd + theta[lay["bd0"][0]]).astype(np.float64)


# ================================================================================================ ReverseKL / ForwardKL
KL_PI_LR, KL_QV_LR, KL_ALPHA, KL_TAU, KL_AMAX = 1e-3, 1e-2, 0.3, 0.01, 2.0
KL_INIT_SEED = 1
KL_MODES = [("reverse", "intg"), ("reverse", "hard_intg"), ("reverse", "ll"), ("reverse", "hard_ll"), ("forward", "intg")]
KL_GATED = ("pWs", "pbs")
# (e) conditioning of the squash correction: tanh(z) carries about one fp32 ulp (6e-8) of rounding, so 1 - tanh(z)^2 about
# 2e-7; with 1 - tanh(z)^2 >= SQUASH_FLOOR the log moves by 2e-5 at the most, 4e-6 of a log density of 5 or more
KL_EPS_WIDTH, SQUASH_FLOOR = 0.35, 0.01


def _kl(dims, B, ws_scale, pbs, want, n_param=0, l_param=None, kernels=("generic", "mfma"), eps_width=KL_EPS_WIDTH):
    return dict(dims=dims, B=B, n_param=n_param, l_param=l_param, ws_scale=float(ws_scale), pbs=tuple(pbs), want=tuple(want),
                kernels=kernels, eps_width=eps_width)


_S1, _S2 = (5, 1, 64, 48, 40, 56), (3, 1, 128, 128, 128, 128)
_A2G, _A2M = (3, 2, 48, 40, 44, 36), (3, 2, 64, 64, 64, 64)        # tests/test_kl.py MULTI, tests/test_kl_mfma_action2.py SHAPES
# Recipe of a case: from init_params(dims, KL_INIT_SEED), pWm, qW3 and vW3 are multiplied by 30 (tests/test_kl.py's
# _lively), pWs by ws_scale, and pbs[j] is set.  want[j]: the regions dimension j of the raw log_std must reach.
KL_CASES = {
    "kl_mixed_upper_s1": _kl(_S1, 17, 300.0, (3.0,), (("inside", "above"),), n_param=9),
    "kl_mixed_upper_s2": _kl(_S2, 100, 300.0, (1.5,), (("inside", "above"),), n_param=33),
    "kl_all_above": _kl(_S1, 17, 30.0, (5.0,), ("all-above",), n_param=9),
    # eps = 0: with std = e^-20 the draw mean + std eps is mean itself in fp32 whatever eps is, and 1 / var = e^40 turns
    # the rounding of z - mean into the log density; at eps = 0 it is mean in float64 as well
    "kl_all_below": _kl(_S1, 17, 30.0, (-25.0,), ("all-below",), n_param=9, eps_width=0.0),
    "kl_action2_generic_0above": _kl(_A2G, 12, 30.0, (5.0, 0.0), ("all-above", "all-inside"), l_param=5, kernels=("generic",)),
    "kl_action2_generic_1above": _kl(_A2G, 12, 30.0, (0.0, 5.0), ("all-inside", "all-above"), l_param=5, kernels=("generic",)),
    "kl_action2_mfma_0above": _kl(_A2M, 32, 30.0, (5.0, 0.0), ("all-above", "all-inside"), l_param=6, kernels=("mfma",)),
    "kl_action2_mfma_1above": _kl(_A2M, 32, 30.0, (0.0, 5.0), ("all-inside", "all-above"), l_param=6, kernels=("mfma",)),
}
KL_MIXED = [k for k, c in KL_CASES.items() if not isinstance(c["want"][0], str)]
KL_BOUNDARY = dict(dims=(3, 1, 16, 16, 16, 16), B=8, n_param=9, seed=3, modes=[("reverse", "ll"), ("forward", "intg")],
                   # at -20 the draw is mean itself in fp32 whatever eps is (see kl_all_below); eps = 0 makes it so everywhere.
                   # ReverseKL's integral is no mode for that edge: its quadrature misses the spike and the gradient is 0
                   eps_width={2.0: KL_EPS_WIDTH, -20.0: 0.0})


def kl_theta(case):
    d = K.KlDims(*case["dims"])
    th, lay = K.init_params(d, KL_INIT_SEED), d.layout()[0]
    for name, scale in (("pWm", 30.0), ("pWs", case["ws_scale"]), ("qW3", 30.0), ("vW3", 30.0)):
        off, shp = lay[name]
        th[off:off + int(np.prod(shp))] *= np.float32(scale)
    off = lay["pbs"][0]
    th[off:off + len(case["pbs"])] = np.asarray(case["pbs"], np.float32)
    return th


def kl_boundary_theta(bias):
    """pWs = 0 and pbs = bias: the raw log_std is the bias itself in every row, on every implementation"""
    d = K.KlDims(*KL_BOUNDARY["dims"])
    th, lay = K.init_params(d, KL_INIT_SEED), d.layout()[0]
    for name in ("pWm", "qW3", "vW3"):
        off, shp = lay[name]
        th[off:off + int(np.prod(shp))] *= np.float32(30.0)
    off, shp = lay["pWs"]
    th[off:off + int(np.prod(shp))] = 0.0
    th[lay["pbs"][0]] = np.float32(bias)
    return th


def kl_batch(seed, B, S, A, eps_width=KL_EPS_WIDTH):
    """the minibatch of tests/test_kl.py (s, a, s2, r, gamma, eps), from RandomState(seed), but for the draw: eps is uniform
    in +-eps_width.  At the upper clamp std = e^2, and a standard normal eps would put z = mean + std eps at 10 and beyond,
    where tanh(z) rounds to 1 and log(1 - tanh(z)^2 + 1e-6) is rounding noise (condition e)."""
    rng = np.random.RandomState(seed)
    return (rng.uniform(-2, 2, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-2, 2, (B, S)),
            rng.uniform(-16, 0, B), np.where(rng.rand(B) < 0.2, 0.0, 0.99), rng.uniform(-1, 1, (B, A)) * eps_width)


def kl_case_batch(case, seed):
    return kl_batch(seed, case["B"], case["dims"][0], case["dims"][1], case["eps_width"])


def kl_action_max(case):
    A = case["dims"][1]
    return np.full(A, KL_AMAX) if A > 1 else None


def kl_restatement(case, theta, kind, optim, qup="non_sac", dtype=torch.float32):
    return K.KLOracle(kind, K.KlDims(*case["dims"]), theta, KL_PI_LR, KL_QV_LR, KL_ALPHA, KL_TAU, KL_AMAX, case["n_param"], optim,
                      qup, l_param=case["l_param"], action_max=kl_action_max(case), dtype=dtype)


def kl_preacts(dims, theta, s, a):
    """(raw log_std [B, A] in front of clamp(., -20, 2), the smallest |hidden pre-activation| of pi, Q(s, a) and V) on
    the fp32 restatement (oracle/kl_torch.py's _pi, taken apart; _near_relu_kink of tests/test_kl.py)"""
    d = K.KlDims(*dims)
    lay = d.layout()[0]
    with torch.no_grad():
        p = K._views(torch.tensor(np.asarray(theta, np.float32)), lay)
        s = torch.tensor(np.asarray(s, np.float32))
        xq = torch.cat([s, torch.tensor(np.asarray(a, np.float32))], 1)
        kink = float("inf")
        for pre, x in (("p", s), ("q", xq), ("v", s)):
            z1 = x @ p[pre + "W1"] + p[pre + "b1"]
            z2 = torch.relu(z1) @ p[pre + "W2"] + p[pre + "b2"]
            kink = min(kink, z1.abs().min().item(), z2.abs().min().item())
            if pre == "p":
                raw = torch.relu(z2) @ p["pWs"] + p["pbs"]
    return raw.numpy().astype(np.float64), kink


def kl_sensitivity(case, theta, batch):
    """condition (d): over the five modes and the gated tensors, the smallest (twin without the gate against the true
    twin) / bar"""
    lay = K.KlDims(*case["dims"]).layout()[0]
    worst = float("inf")
    for kind, optim in KL_MODES:
        true = kl_restatement(case, theta, kind, optim, dtype=torch.float64).update(*batch, taps=True)["grads"]
        with gate_removed():
            loose = kl_restatement(case, theta, kind, optim, dtype=torch.float64).update(*batch, taps=True)["grads"]
        for n in KL_GATED:
            off, shp = lay[n]
            k = int(np.prod(shp))
            worst = min(worst, rel(loose[off:off + k], true[off:off + k]) / (KL_GRAD_BAR if k > 1 else KL_GRAD1_BAR))
    return worst


def kl_failures(case, seed):
    """conditions (a) to (d) for the minibatch of RandomState(seed); [] when all hold"""
    S, A = case["dims"][:2]
    theta, batch = kl_theta(case), kl_case_batch(case, seed)
    raw, kink = kl_preacts(case["dims"], theta, batch[0], batch[1])
    out = []
    for j in range(A):
        out += ["dim %d %s" % (j, f) for f in _region_failures(raw[:, j], KL_LO, KL_HI, case["want"][j])]
    if case["want"][0] == "all-below" and np.max(raw) >= KL_LO - 1.0:
        out.append("b: a row within 1 of the lower edge")
    if kink < KINK:
        out.append("c: a hidden pre-activation %.3e from zero" % kink)
    z = kl_restatement(case, theta, "reverse", "ll").update(*batch, taps=True)["z"]
    squash = float(np.min(1.0 - np.tanh(z.astype(np.float64)) ** 2))
    if squash < SQUASH_FLOOR:
        out.append("e: 1 - tanh(z)^2 down to %.3e" % squash)
    if not isinstance(case["want"][0], str) and not out:
        ratio = case_sensitivity(case, seed)
        if ratio < SENSITIVITY:
            out.append("d: the gate moves a gated tensor by %.1f bars only" % ratio)
    return out


# ================================================================================================ the search, its record
_SENSITIVITY = {}


def case_sensitivity(case, seed):
    """condition (d) of one case dict and minibatch seed, computed once"""
    key = (repr(sorted(case.items())), seed)
    if key not in _SENSITIVITY:
        if "scale" in case:
            _SENSITIVITY[key] = naf_sensitivity(case, naf_theta(case), naf_batch(seed, case["B"], *case["dims"][:2]))
        else:
            _SENSITIVITY[key] = kl_sensitivity(case, kl_theta(case), kl_case_batch(case, seed))
    return _SENSITIVITY[key]


def failures(name, seed):
    if name == "naf_explore":
        return naf_explore_failures(seed)
    return naf_failures(NAF_CASES[name], seed) if name in NAF_CASES else kl_failures(KL_CASES[name], seed)


def seed_list(name):
    return NAF_EXPLORE["seed_list"] if name == "naf_explore" else SEED_LIST


def find_seed(name, seeds=None):
    """the first seed of the case's list whose minibatch meets every condition on the restatements; None if there is none"""
    for seed in (seed_list(name) if seeds is None else seeds):
        if not failures(name, seed):
            return seed
    return None


# what find_seed(name) returns (tests/test_clamp_cases.py re-runs the search)
CASE_SEEDS = {
    "naf_mixed_8x2x200x200_b32": 1, "naf_mixed_8x2x200x200_b97": 1, "naf_mixed_3x1x64x48_b17": 1, "naf_mixed_5x3x32x40_b9": 1,
    "naf_mixed_wide_3x3x64x48_b17": 3,      # seeds 1 and 2: a column with no row outside (d), too few rows inside (b)
    "naf_mixed_layer_5x3x32x40_b9": 1, "naf_all_clamped": 1, "naf_explore": 8,
    "kl_mixed_upper_s1": 1, "kl_mixed_upper_s2": 1, "kl_all_above": 1, "kl_all_below": 1,
    "kl_action2_generic_0above": 1, "kl_action2_generic_1above": 1, "kl_action2_mfma_0above": 1, "kl_action2_mfma_1above": 1,
}
