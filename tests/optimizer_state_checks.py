"""Checks of the second half of an update: Adam's m / v, the parameters after the step, the Polyak average into the target.

Pure numpy.  Every function takes the state BEFORE one update, the state AFTER it and (check a, e) the oracle's state
after the same update from the same start plus its gradient taps; none knows whether a state came from a HIP kernel or
from an oracle.  A state is a dict
    theta, theta_target   [P] float32
    m, v                  {slot: [P] float32}    slot "actor" / "critic" (DDPG's two optimizers) or "adam"
    pw                    beta powers BEFORE they are advanced past this state (float32; TF-style Adam), or the one-element
                          integer step count (the KL agents' torch-style Adam)
and a Spec says which optimizer owns which range (read from oracle/ddpg_oracle.c:238-290, ddpg_variants_oracle.c:243-280,
sac_oracle.c:319-324, naf_oracle.c:244-252, the three *_variants.py and kl_torch.py:263-269).

  a  m', v' against the oracle, per tensor, as absolute bounds that FOLLOW from the gradient tolerance tol_g the parity
     tests hold (relative to the tensor's max|g|), both sides starting from bit-identical m, v:
        |m' - m'_o| <= (1-b1) * tol_g * max|g|                     + 2 ulp(m')
        |v' - v'_o| <= (1-b2) * (2 tol_g + tol_g^2) * max|g|^2     + 2 ulp(v')
  b  theta' against the plain Adam formula in float64 on the result's OWN m', v', the old theta and the beta powers from
     before the update: theta' = theta - alpha m' / (sqrt(v') + 1e-8), alpha = lr sqrt(1-b2^t) / (1-b1^t) (torch's form
     for the KL agents: theta - (lr / (1-b1^t)) m' / (sqrt(v') / sqrt(1-b2^t) + 1e-8)); a range two optimizers own (DDPG's
     shared first layer: the critic's step, then the actor's) subtracts both steps.  EVERY element, in units of
        ulp_f32(theta) + 2^-23 * sum |step|
  c  theta_target' against tt + tau (theta' - tt) in float64 on the result's own theta'.  EVERY element, in units of
        ulp_f32(max(|tt|, |theta'|))
     -- pins tau, pins that the average reads the weights AFTER the step, covers every tile.
  d  ranges of a slot that no optimizer owns keep their bits in m and v; ranges the Polyak average does not move keep
     their bits in the target.
  e  beta powers equal the oracle's at rtol 1e-6 (the step count exactly).

ulp_f32(x) is the float32 spacing at max(|x|, FLT_MIN): the oracles and the kernels flush denormals, so a result below
FLT_MIN may come out as zero.

The two unit bounds are measured on the ORACLES (tests/test_optimizer_state_checks.py runs checks b and c on the oracles'
own before / after states, every case of tests/test_gpu_optimizer_state.py, target started apart, two warm-up updates):
  ADAM_UNITS   = 4 x the oracles' largest count = 4 x 2.36 = 9.44.  Measured 2.36 (DDPG, separate networks,
                 (12,3,128,128,128)/100), 2.30 (DDPG (3,1,200,200,200)/97), 2.14 (SAC), 1.14 (NAF), 1.58 (KL).  The
                 factor: the kernels use the hardware rcp and sqrt, about 1 ulp each, where the oracle divides with
                 correct rounding.
  POLYAK_UNITS = 2 x the larger count of the two algebraic forms the oracles use, tt += tau (th - tt) and
                 (1-tau) tt + tau th, both evaluated in numpy float32 on those states = 2 x 1.15 = 2.30.  Measured 1.15
                 ((1-tau) tt + tau th; SAC (3,1,128,128,128,128)/32) and 0.52 (tt += tau (th - tt): DDPG, NAF).
Largest values seen on an MI355X over the 48 single-update cases and the three population cases: Adam 2.65 units (DDPG wide,
(17,6,200,200,200)/32; 2.63 separate networks, 2.60 latency mode; SAC 2.30, NAF 1.42, KL 1.90), Polyak 1.15 units (SAC; 0.50
for DDPG and NAF), m' at most 0.58 and v' at most 0.40 of their bounds.
For scale: a Polyak average that read the weights before the step is about 170 units away at |w| = 0.5.
"""
from collections import OrderedDict, namedtuple

import numpy as np

B1, B2, ADAM_EPS = 0.9, 0.999, 1e-8
FLT_MIN = np.float32(1.17549435e-38)

# measured on the CPU oracles (DDPG, its variants, SAC, NAF, their layer-norm variants, the KL agents; every case of the
# GPU file): the largest Adam count and the larger of the two Polyak forms' counts.  The CPU tests assert that a fresh
# measurement on the C oracles (plain scalar loops: the same bits everywhere) stays at or below these, so the GPU bounds
# below cannot drift from what they were derived from.
ORACLE_ADAM_UNITS = 2.36
ORACLE_POLYAK_UNITS = 1.15
ADAM_UNITS = 4 * ORACLE_ADAM_UNITS
POLYAK_UNITS = 2 * ORACLE_POLYAK_UNITS

# owner of a range: slot = which m / v blob, pw = indices of (b1^t, b2^t) in the beta powers, grads = name of the
# gradient tap.  Listed in the order the steps are taken.
Opt = namedtuple("Opt", "name slot ranges lr pw grads")
Spec = namedtuple("Spec", "layout P opts polyak tau adam tol_g")      # tol_g(tensor name, element count)


class CheckFailed(AssertionError):
    def __init__(self, failures):
        self.failures = failures                      # [(check letter, message)]
        self.checks = sorted(set(c for c, _ in failures))
        AssertionError.__init__(self, "; ".join("check %s: %s" % f for f in failures))


def ulp32(x):
    a = np.maximum(np.abs(np.asarray(x, np.float64)), float(FLT_MIN)).astype(np.float32)
    return np.spacing(a).astype(np.float64)


def _f64(x):
    return np.asarray(x, np.float32).astype(np.float64)


def _mask(P, ranges):
    k = np.zeros(P, bool)
    for lo, hi in ranges:
        k[lo:hi] = True
    return k


def _tensors(spec, ranges):
    """the layout's tensors that lie inside `ranges`"""
    own = _mask(spec.P, ranges)
    for name, (off, shp) in spec.layout.items():
        n = int(np.prod(shp))
        if own[off:off + n].all():
            yield name, off, n
        else:
            assert not own[off:off + n].any(), name   # an optimizer owns whole tensors


def bias_corrections(spec, opt, pw):
    """(1 - b1^t, 1 - b2^t) of the update that starts from beta powers / step count `pw`"""
    if spec.adam == "torch":
        t = int(np.asarray(pw).reshape(-1)[0]) + 1
        return 1.0 - B1 ** t, 1.0 - B2 ** t
    p = _f64(pw)
    return 1.0 - p[opt.pw[0]], 1.0 - p[opt.pw[1]]


def adam_steps(spec, before, after):
    """float64 steps of every optimizer on the result's own m', v': [(opt, mask, step [P])]"""
    out = []
    for opt in spec.opts:
        bc1, bc2 = bias_corrections(spec, opt, before["pw"])
        lr = float(np.float32(opt.lr))
        m, v = _f64(after["m"][opt.slot]), _f64(after["v"][opt.slot])
        if spec.adam == "torch":
            step = (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + ADAM_EPS)
        else:
            step = (lr * np.sqrt(bc2) / bc1) * m / (np.sqrt(v) + ADAM_EPS)
        k = _mask(spec.P, opt.ranges)
        out.append((opt, k, np.where(k, step, 0.0)))
    return out


def moment_deviation(spec, before, after, oracle_after, grads):
    """check a: [(opt, tensor, 'm' | 'v', largest deviation, bound at that element's tensor)] and the failures"""
    rows, fails = [], []
    for opt in spec.opts:
        g = _f64(grads[opt.grads])
        for name, off, n in _tensors(spec, opt.ranges):
            sl = slice(off, off + n)
            gmax = float(np.max(np.abs(g[sl])))
            tol = spec.tol_g(name, n)
            for which, lead in (("m", (1 - B1) * tol * gmax), ("v", (1 - B2) * (2 * tol + tol * tol) * gmax * gmax)):
                got, want = _f64(after[which][opt.slot][sl]), _f64(oracle_after[which][opt.slot][sl])
                bound = lead + 2 * ulp32(want)
                dev = np.abs(got - want)
                i = int(np.argmax(dev - bound))
                rows.append((opt.name, name, which, float(dev[i]), float(bound[i])))
                if not np.all(dev <= bound):
                    fails.append(("a", "%s %s' of %s: |dev| %.3e > bound %.3e at element %d (%d elements over)"
                                  % (opt.name, which, name, dev[i], bound[i], i, int(np.sum(dev > bound)))))
    return rows, fails


def adam_units(spec, before, after):
    """check b: the per-element count |theta' - expected| / (ulp(theta) + 2^-23 sum|step|)"""
    th = _f64(before["theta"])
    steps = adam_steps(spec, before, after)
    total = sum(s for _, _, s in steps)
    mag = sum(np.abs(s) for _, _, s in steps)
    # the same order as the kernels and the oracles: one step after the other (in float64 the order does not matter)
    return np.abs(_f64(after["theta"]) - (th - total)) / (ulp32(th) + 2.0 ** -23 * mag)


def polyak_units(spec, before, after):
    """check c over the ranges the average moves"""
    tt, th = _f64(before["theta_target"]), _f64(after["theta"])
    tau = float(np.float32(spec.tau))
    want = tt + tau * (th - tt)
    units = np.abs(_f64(after["theta_target"]) - want) / ulp32(np.maximum(np.abs(tt), np.abs(th)))
    return np.where(_mask(spec.P, spec.polyak), units, 0.0)


def polyak_forms_units(spec, before, after):
    """the two forms the oracles use, evaluated in numpy float32 from `before`'s target and `after`'s weights: the larger
    of their largest counts (what POLYAK_UNITS is derived from)"""
    tt, th, tau = np.asarray(before["theta_target"], np.float32), np.asarray(after["theta"], np.float32), np.float32(spec.tau)
    worst = 0.0
    for form in (tt + tau * (th - tt), (np.float32(1) - tau) * tt + tau * th):
        worst = max(worst, float(np.max(polyak_units(spec, before, dict(after, theta_target=form)))))
    return worst


def unowned_failures(spec, before, after):
    fails = []
    for slot in before["m"]:
        free = ~_mask(spec.P, [r for o in spec.opts if o.slot == slot for r in o.ranges])
        for which in ("m", "v"):
            x, y = np.asarray(before[which][slot], np.float32), np.asarray(after[which][slot], np.float32)
            bad = free & (x.view(np.uint32) != y.view(np.uint32))
            if bad.any():
                fails.append(("d", "%s %s changed in a range its optimizer does not own: %d elements, first %d"
                              % (slot, which, int(bad.sum()), int(np.argmax(bad)))))
    free = ~_mask(spec.P, spec.polyak)
    x, y = np.asarray(before["theta_target"], np.float32), np.asarray(after["theta_target"], np.float32)
    bad = free & (x.view(np.uint32) != y.view(np.uint32))
    if bad.any():
        fails.append(("d", "theta_target changed where the average does not move it: %d elements, first %d"
                      % (int(bad.sum()), int(np.argmax(bad)))))
    return fails


def _where(spec, i):
    for name, (off, shp) in spec.layout.items():
        if off <= i < off + int(np.prod(shp)):
            return "%s[%d]" % (name, i - off)
    return str(i)


def check_update(spec, before, after, oracle_after=None, grads=None, label="", adam_bound=ADAM_UNITS,
                 polyak_bound=POLYAK_UNITS, quiet=False):
    """checks b, c, d always; a and e when the oracle's after-state and gradient taps are given.  Prints every measured
    quantity, raises CheckFailed naming every check that failed, returns the measurements."""
    fails, out = [], {}
    if oracle_after is not None:
        rows, f = moment_deviation(spec, before, after, oracle_after, grads)
        fails += f
        for which in ("m", "v"):
            r = max((r for r in rows if r[2] == which), key=lambda r: r[3] / r[4] if r[4] > 0 else float(r[3] > 0))
            out[which] = (r[3], r[4])
            if not quiet:
                print("%s %s': largest deviation/bound %.3e / %.3e (%s %s)" % (label, which, r[3], r[4], r[0], r[1]))
    u = adam_units(spec, before, after)
    i = int(np.argmax(u))
    out["adam_units"] = float(u[i])
    if not quiet:
        print("%s Adam: %.2f units at %s (bound %.2f)" % (label, u[i], _where(spec, i), adam_bound))
    if not u[i] <= adam_bound:
        fails.append(("b", "theta' is %.2f units from the Adam formula at %s (%d elements over %.2f)"
                      % (u[i], _where(spec, i), int(np.sum(u > adam_bound)), adam_bound)))
    u = polyak_units(spec, before, after)
    i = int(np.argmax(u))
    out["polyak_units"] = float(u[i])
    if not quiet:
        print("%s Polyak: %.2f units at %s (bound %.2f)" % (label, u[i], _where(spec, i), polyak_bound))
    if not u[i] <= polyak_bound:
        fails.append(("c", "theta_target' is %.2f units from tt + tau (theta' - tt) at %s (%d elements over %.2f)"
                      % (u[i], _where(spec, i), int(np.sum(u > polyak_bound)), polyak_bound)))
    fails += unowned_failures(spec, before, after)
    if oracle_after is not None:
        got, want = np.asarray(after["pw"]), np.asarray(oracle_after["pw"])
        ok = np.array_equal(got, want) if spec.adam == "torch" else np.allclose(got, want, rtol=1e-6, atol=0)
        if not quiet:
            print("%s beta powers %s (oracle %s)" % (label, got, want))
        if not ok:
            fails.append(("e", "beta powers %s, oracle %s" % (got, want)))
    if fails:
        raise CheckFailed(fails)
    return out


# ------------------------------------------------------------------------------------------ specs
def ddpg_spec(layout, P, actor_lr, critic_lr, tau, separate=False, tol_g=1e-5):
    """Adam_c: the first layer (with its layer norm) unless the networks are separate, and the critic block; then Adam_a:
    everything before the critic block (oracle/ddpg_oracle.c:239-240,288; ddpg_variants_oracle.c:243-244,277).  Beta
    powers: actor's, then critic's.  Polyak over every tensor."""
    critic0 = layout["Wc1" if separate else "Wc2"][0]
    c_ranges = [(critic0, P)] if separate else [(0, layout["Wa2"][0]), (critic0, P)]
    opts = [Opt("critic", "critic", c_ranges, critic_lr, (2, 3), "grads_c"),
            Opt("actor", "actor", [(0, critic0)], actor_lr, (0, 1), "grads_a")]
    return Spec(layout, P, opts, [(0, P)], tau, "tf", lambda name, n: tol_g)


def sac_spec(layout, P, pi_lr, qv_lr, tau, tol_g=2e-5):
    """pi-Adam on the policy block, value-Adam on qf and vf, one m / v blob; Polyak over every tensor
    (oracle/sac_oracle.c:319-324)"""
    pi_end = layout["qW1"][0]
    opts = [Opt("pi", "adam", [(0, pi_end)], pi_lr, (0, 1), "grads"), Opt("qv", "adam", [(pi_end, P)], qv_lr, (2, 3), "grads")]
    return Spec(layout, P, opts, [(0, P)], tau, "tf", lambda name, n: tol_g)


def naf_spec(layout, P, lr, tau, tol_g=2e-5):
    """one Adam and the Polyak average over every tensor (oracle/naf_oracle.c:244-252)"""
    return Spec(layout, P, [Opt("adam", "adam", [(0, P)], lr, (0, 1), "grads")], [(0, P)], tau, "tf", lambda name, n: tol_g)


def kl_spec(layout, P, pi_lr, qv_lr, tau, action_dim=1):
    """torch's Adam, one step count: q, v at qf_vf_lr, pi at pi_lr; the average moves the V block only
    (oracle/kl_torch.py:263-269).  tol_g: the gradient levels of tests/test_kl.py and tests/test_kl_mfma_action2.py: 5e-5;
    3e-4 for a one-element tensor (a cancelling sum over the batch measured against itself) and, on the sparse grid of
    action_dim > 1 (weights of both signs), for the policy's tensors."""
    pi_end, v0 = layout["qW1"][0], layout["vW1"][0]
    opts = [Opt("qv", "adam", [(pi_end, P)], qv_lr, None, "grads"), Opt("pi", "adam", [(0, pi_end)], pi_lr, None, "grads")]
    tol = lambda name, n: 3e-4 if (n == 1 or (action_dim > 1 and name[0] == "p")) else 5e-5
    return Spec(layout, P, opts, [(v0, P)], tau, "torch", tol)


# ------------------------------------------------------------------------------------------ oracle <-> state
_SLOTS = OrderedDict((("actor", ("m_a", "v_a")), ("critic", ("m_c", "v_c")), ("adam", ("m", "v"))))


def _np(x):
    return (x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)).astype(np.float32).copy()


def oracle_state(o):
    """the state of an oracle object (numpy attributes, or torch attributes for the variant and KL oracles)"""
    st = {"theta": _np(o.theta), "theta_target": _np(o.theta_t), "m": {}, "v": {}}
    for slot, (mn, vn) in _SLOTS.items():
        if hasattr(o, mn):
            st["m"][slot], st["v"][slot] = _np(getattr(o, mn)), _np(getattr(o, vn))
    st["pw"] = np.asarray(o.pw, np.float32).copy() if hasattr(o, "pw") else np.array([o.step], np.int64)
    return st


def load_oracle(o, st):
    """copy a state into a fresh oracle's arrays"""
    def put(name, value):
        old = getattr(o, name)
        if hasattr(old, "detach"):
            import torch
            setattr(o, name, torch.tensor(np.asarray(value, np.float32).copy()).to(old.dtype))
        else:
            setattr(o, name, np.asarray(value, np.float32).copy())
    put("theta", st["theta"])
    put("theta_t", st["theta_target"])
    for slot, (mn, vn) in _SLOTS.items():
        if hasattr(o, mn):
            put(mn, st["m"][slot])
            put(vn, st["v"][slot])
    if hasattr(o, "pw"):
        o.pw = np.asarray(st["pw"], np.float32).copy()
    else:
        o.step = int(np.asarray(st["pw"]).reshape(-1)[0])
