"""The cases of tests/test_gpu_optimizer_state.py, shared with the CPU run of the oracles through the same checker
(tests/test_optimizer_state_checks.py): for each case the initial weights, a fresh oracle, the HIP population, the
ownership spec and the minibatches.  The shapes are ones the existing parity tests already run on the named kernel."""
import numpy as np

import optimizer_state_checks as C

TAU = 0.01


def _bounds(S, A):
    return -np.ones(S) * 2, np.ones(S) * 2, np.linspace(1.0, 2.0, A)


def _seeds(seeds, first, n_agents):
    """a pop()'s per-agent Philox keys: the caller's, or the family's usual run first, first + 1, ..."""
    return list(seeds) if seeds is not None else list(range(first, first + n_agents))


class Case(object):
    """kernel: 'generic' or 'mfma' (the wide forms are opt-in through the same name); split: latency mode's workgroups"""
    SLOTS = {"adam": ("adam_m", "adam_v")}
    GRADS = ("grads",)
    EPS = False

    def __init__(self, dims, B, kernel, **kw):
        self.dims, self.B, self.kernel = tuple(dims), int(B), kernel
        self.split = kw.pop("split", 0)
        self.seed = kw.pop("seed", 1)             # minibatch seed of the schedules that search for one (tests/mfma_unit_cases.py)
        self.kw = kw
        self.S, self.A = self.dims[0], self.dims[1]

    @property
    def id(self):
        extra = "".join("-%s" % (k if v is True else "%s%s" % (k, v)) for k, v in sorted(self.kw.items()) if v)
        return "%s-%s-%s-B%d%s%s" % (self.NAME, self.kernel, "x".join(map(str, self.dims)), self.B, extra,
                                     "-split%d" % self.split if self.split else "")

    def batch(self, rng):
        B, S, A = self.B, self.S, self.A
        out = (rng.uniform(-2, 2, (B, S)), rng.uniform(-2, 2, (B, A)), rng.uniform(-2, 2, (B, S)), rng.uniform(-16, 0, B),
               np.where(rng.rand(B) < 0.2, 0.0, 0.99))
        return out + ((rng.randn(B, A),) if self.EPS else ())

    def replay(self, rng, N):
        """(s, a, r, s2, g) in replay_add_batch's order"""
        S, A = self.S, self.A
        return (rng.uniform(-2, 2, (N, S)), rng.uniform(-2, 2, (N, A)), rng.uniform(-16, 0, N), rng.uniform(-2, 2, (N, S)),
                np.where(rng.rand(N) < 0.2, 0.0, 0.99))

    def from_replay(self, data, idx, eps=None):
        """the minibatch `idx` of replay() in update()'s order"""
        s, a, r, s2, g = data
        return (s[idx], a[idx], s2[idx], r[idx], g[idx]) + ((eps,) if self.EPS else ())

    def target_apart(self, theta, rng):
        return (theta + rng.uniform(-0.05, 0.05, theta.size)).astype(np.float32)

    def select_kernel(self, pop):
        pop.set_kernel(self.kernel)               # no skip: a refusal is a failure
        assert pop.kernel_in_use() == self.kernel
        if self.split:
            pop.set_split(self.split)
        return pop

    def pop_state(self, pop, agent=0):
        st = {"theta": pop.get_blob(agent, "theta"), "theta_target": pop.get_blob(agent, "theta_target"), "m": {}, "v": {}}
        for slot, (mn, vn) in self.SLOTS.items():
            st["m"][slot], st["v"][slot] = pop.get_blob(agent, mn), pop.get_blob(agent, vn)
        st["pw"] = self.pop_powers(pop, agent)
        return st

    def pop_powers(self, pop, agent):
        return pop.get_beta_powers(agent)

    def pop_grads(self, pop, agent=0):
        return {k: pop.last_tap(agent, k) for k in self.GRADS}

    def grads(self, taps):
        return {k: np.asarray(taps[k], np.float32) for k in self.GRADS}


class DDPGCase(Case):
    """kw: norm (layer norm), sep (separate networks)"""
    NAME = "ddpg"
    SLOTS = {"actor": ("actor_m", "actor_v"), "critic": ("critic_m", "critic_v")}
    GRADS = ("grads_c", "grads_a")
    LR = (1e-3, 1e-2)

    def _vd(self):
        from oracle.ddpg_variants import VDims
        return VDims(*self.dims, norm=bool(self.kw.get("norm")), separate=bool(self.kw.get("sep")))

    def theta0(self, seed=3):
        from oracle.ddpg_variants import init_params
        d = self._vd()
        th = init_params(d, seed)
        rng = np.random.RandomState(seed + 50)
        for n, (off, shp) in d.layout()[0].items():       # layer-norm gamma / beta off their trivial initial values
            if n[0] == "l":
                th[off:off + shp[0]] += rng.uniform(-0.3, 0.3, shp[0]).astype(np.float32)
        return th

    def oracle(self, theta, lr=None):
        from oracle.ddpg_variants import DDPGVariantOracle     # without norm / sep: oracle/ddpg_oracle.c bit for bit
        lr = lr or self.LR
        smin, smax, amax = _bounds(self.S, self.A)
        return DDPGVariantOracle(self._vd(), theta, lr[0], lr[1], TAU, smin, smax, amax)

    def spec(self, lr=None):
        lr = lr or self.LR
        lay, P = self._vd().layout()
        return C.ddpg_spec(lay, P, lr[0], lr[1], TAU, separate=bool(self.kw.get("sep")))

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        from rlcontrol_amd.hip_ddpg import DDPGPopulation
        lr = lr or self.LR
        smin, smax, amax = _bounds(self.S, self.A)
        S, A, H1, HA, HC = self.dims
        pop = DDPGPopulation(n_agents, S, A, H1, HA, HC, self.B, cap, TAU, smin, smax, -amax, amax, lr[0], lr[1],
                             seeds=_seeds(seeds, 10, n_agents), norm_type="layer" if self.kw.get("norm") else "input_norm",
                             separate_networks=bool(self.kw.get("sep")))
        return self.select_kernel(pop)


class SACCase(Case):
    NAME = "sac"
    EPS = True
    LR = (1e-2, 1e-1)
    HYPER = (0.5, TAU, -1.0, 1.0, 2.0)         # entropy scale, tau, state_min[0], state_max[0], action_max[0]

    def theta0(self, seed=1):
        from oracle.sac_variants import init_params, layout
        norm = bool(self.kw.get("norm"))
        lay, _ = layout(self.dims, norm)
        th = init_params(self.dims, seed, norm)
        for name, f in (("pWs", 0.02), ("pWm", 0.3)):       # the well-conditioned regime of tests/test_sac.py
            off, shp = lay[name]
            th[off:off + int(np.prod(shp))] *= f
        rng = np.random.RandomState(seed + 76)
        for name, (off, shp) in lay.items():
            if name[1] == "L":
                th[off:off + shp[0]] = rng.uniform(0.5, 1.5, shp[0]) if name.endswith("g") else rng.uniform(-0.3, 0.3, shp[0])
        return th

    def oracle(self, theta, lr=None):
        lr = lr or self.LR
        if self.kw.get("norm"):
            from oracle.sac_variants import SacVariantOracle
            return SacVariantOracle(self.dims, theta, lr[0], lr[1], *self.HYPER)
        from oracle.sac import SACOracle, SacDims
        return SACOracle(SacDims(*self.dims), theta, lr[0], lr[1], *self.HYPER)

    def spec(self, lr=None):
        from oracle.sac_variants import layout
        lr = lr or self.LR
        lay, P = layout(self.dims, bool(self.kw.get("norm")))
        return C.sac_spec(lay, P, lr[0], lr[1], TAU)

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        from rlcontrol_amd.hip_sac import SACPopulation
        lr = lr or self.LR
        al, tau, smin0, smax0, amax0 = self.HYPER
        S, A, L1A, L2A, L1C, L2C = self.dims
        pop = SACPopulation(n_agents, S, A, L1A, L2A, L1C, L2C, self.B, cap, tau, smin0, smax0, amax0, lr[0], lr[1], al,
                            seeds=_seeds(seeds, 5, n_agents), norm_type="layer" if self.kw.get("norm") else "input_norm")
        return self.select_kernel(pop)


class NAFCase(Case):
    NAME = "naf"
    LR = (1e-3,)

    def theta0(self, seed=2):
        from oracle.naf_variants import init_params, layout
        norm = bool(self.kw.get("norm"))
        th = init_params(self.dims, seed, norm)
        rng = np.random.RandomState(seed + 100)
        for n, (off, shp) in layout(self.dims, norm)[0].items():
            if n.startswith("L"):
                th[off:off + shp[0]] += rng.uniform(-0.2, 0.2, shp[0]).astype(np.float32)
        return th

    def oracle(self, theta, lr=None):
        lr = lr or self.LR
        smin, smax, amax = _bounds(self.S, self.A)
        if self.kw.get("norm"):
            from oracle.naf_variants import NafVariantOracle
            return NafVariantOracle(self.dims, theta, lr[0], TAU, smin, smax, amax)
        from oracle.naf import NAFOracle, NafDims
        return NAFOracle(NafDims(*self.dims), theta, lr[0], TAU, smin, smax, amax)

    def spec(self, lr=None):
        from oracle.naf_variants import layout
        lr = lr or self.LR
        lay, P = layout(self.dims, bool(self.kw.get("norm")))
        return C.naf_spec(lay, P, lr[0], TAU)

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        from rlcontrol_amd.hip_naf import NAFPopulation
        lr = lr or self.LR
        smin, smax, amax = _bounds(self.S, self.A)
        pop = NAFPopulation(n_agents, *self.dims, self.B, cap, TAU, smin, smax, amax, lr[0],
                            seeds=_seeds(seeds, 3, n_agents), norm_type="layer" if self.kw.get("norm") else "input_norm")
        return self.select_kernel(pop)


class KLCase(Case):
    """kw: kind ('reverse' / 'forward'), n_param (the line rule, action_dim 1) or l_param (the sparse grid)"""
    NAME = "kl"
    EPS = True
    LR = (1e-3, 1e-2)
    ALPHA, AMAX0 = 0.3, 2.0

    def theta0(self, seed=1):
        from oracle import kl_torch as K
        d = K.KlDims(*self.dims)
        lay, _ = d.layout()
        th = K.init_params(d, seed)
        for name in ("pWm", "pWs", "qW3", "vW3"):           # tests/test_kl_mfma_action2.py: every path carries signal
            off, shp = lay[name]
            th[off:off + int(np.prod(shp))] *= 30.0
        return th

    def oracle(self, theta, lr=None):
        from oracle import kl_torch as K
        lr = lr or self.LR
        return K.KLOracle(self.kw["kind"], K.KlDims(*self.dims), theta, lr[0], lr[1], self.ALPHA, TAU, self.AMAX0,
                          self.kw.get("n_param", 0), l_param=self.kw.get("l_param"),
                          action_max=np.full(self.A, self.AMAX0) if self.A > 1 else None)

    def spec(self, lr=None):
        from oracle import kl_torch as K
        lr = lr or self.LR
        lay, P = K.KlDims(*self.dims).layout()
        return C.kl_spec(lay, P, lr[0], lr[1], TAU, action_dim=self.A)

    def pop(self, n_agents=1, lr=None, cap=512, seeds=None):
        from rlcontrol_amd.hip_kl import KLPopulation
        lr = lr or self.LR
        S, A, L1A, L2A, L1C, L2C = self.dims
        pop = KLPopulation(self.kw["kind"], n_agents, S, A, L1A, L2A, L1C, L2C, self.B, cap, TAU, self.AMAX0, lr[0], lr[1],
                           self.ALPHA, seeds=_seeds(seeds, 5, n_agents), n_param=self.kw.get("n_param", 64),
                           l_param=self.kw.get("l_param"), action_max=np.full(A, self.AMAX0) if A > 1 else None)
        return self.select_kernel(pop)

    def pop_powers(self, pop, agent):
        return np.array([pop.get_step(agent)], np.int64)


def _both(cls, shapes, **kw):
    return [cls(d, B, k, **kw) for d, B in shapes for k in ("generic", "mfma")]


def _mfma(cls, shapes, **kw):
    return [cls(d, B, "mfma", **kw) for d, B in shapes]


def single_update_cases():
    from test_ddpg_variants import SHAPES as DDPG_LN_SHAPES
    from test_gpu_naf_wide import CASES as NAF_WIDE
    from test_gpu_sac_wide import CASES as SAC_WIDE
    from test_kl_mfma_action2 import SHAPES as KL_A2
    from test_naf import CASES as NAF_CASES, LN_CASES as NAF_LN
    from test_sac import CASES as SAC_CASES, LN_CASES as SAC_LN
    cases = _both(DDPGCase, [((8, 2, 64, 48, 40), 17), ((1, 1, 16, 16, 16), 5), ((3, 1, 200, 200, 200), 97),
                             ((8, 2, 200, 160, 144), 101), ((3, 1, 128, 128, 128), 128)])
    cases += _mfma(DDPGCase, [((9, 1, 64, 48, 40), 17), ((17, 6, 200, 200, 200), 32), ((32, 6, 128, 128, 128), 128)])
    cases += _both(DDPGCase, [((8, 2, 64, 48, 40), 17)], sep=True) + _mfma(DDPGCase, [((12, 3, 128, 128, 128), 100)], sep=True)
    # layer norm runs on the any-shape kernel only (the MFMA kernels refuse it)
    cases += [DDPGCase(d, B, "generic", norm=True, sep=sep) for d, B in DDPG_LN_SHAPES for sep in (False, True)]
    cases += [DDPGCase((3, 1, 200, 200, 200), 100, "mfma", split=4)]
    wide = lambda table: [c for c in table if c[0][:2] in ((17, 6), (32, 4)) and c[0][2] == 64]
    cases += _both(SACCase, SAC_CASES[:2] + [((3, 2, 128, 96, 112, 128), 100)]) + _mfma(SACCase, wide(SAC_WIDE))
    cases += [SACCase(*SAC_LN[1], kernel="generic", norm=True)]
    cases += _both(NAFCase, NAF_CASES[:2] + [((8, 1, 128, 96), 100)])
    cases += _mfma(NAFCase, wide(NAF_WIDE) + [((11, 3, 128, 128), 113)])
    cases += [NAFCase(*NAF_LN[0], kernel="generic", norm=True)]
    for kind in ("reverse", "forward"):
        cases += _both(KLCase, [((5, 1, 64, 48, 40, 56), 17)], kind=kind, n_param=9)
        cases += _mfma(KLCase, [KL_A2[0][:2]], kind=kind, l_param=KL_A2[0][2])
    return cases


def population_cases():
    """three agents with their own learning rates in one launch; agent 2 is checked"""
    return [(DDPGCase((8, 2, 64, 48, 40), 17, "mfma"), [[1e-3, 5e-4, 3e-3], [1e-2, 5e-2, 2e-2]]),
            (SACCase((8, 2, 64, 48, 40, 56), 17, "mfma"), [[1e-2, 3e-3, 2e-2], [1e-1, 3e-2, 5e-2]]),
            (NAFCase((3, 1, 64, 48), 17, "mfma"), [[1e-3, 5e-4, 3e-3]])]


def tap_cases():
    """one case for each kernel family: taps on and off must leave the same state"""
    return ([DDPGCase((8, 2, 64, 48, 40), 17, "generic"), DDPGCase((8, 2, 64, 48, 40), 17, "mfma"),
             DDPGCase((3, 1, 200, 200, 200), 97, "mfma"), DDPGCase((9, 1, 64, 48, 40), 17, "mfma"),
             DDPGCase((3, 1, 200, 200, 200), 100, "mfma", split=4)] +
            [SACCase((8, 2, 64, 48, 40, 56), 17, k) for k in ("generic", "mfma")] + [SACCase((17, 6, 64, 48, 40, 56), 32, "mfma")] +
            [NAFCase((3, 1, 64, 48), 17, k) for k in ("generic", "mfma")] + [NAFCase((17, 6, 64, 48), 32, "mfma")])
