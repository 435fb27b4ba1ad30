"""The case table of the minibatch front end: "pick B logical indices, map them through the ring, gather (s, a, r, s',
gamma), clip the states", of which every fused update kernel is a call site (the shared body: rlc_common.h; the DDPG
MFMA kernel alone keeps it typed out and is held to the same table).  One entry
for each call site and for each form of one that changes its indexing or its block size, on the smallest shape the
parity tests already run on that kernel.  Shared by tests/test_front_end_cases.py (CPU: the table can fail) and
tests/test_gpu_minibatch_front_end.py (GPU: properties P1 to P5, every one bit-exact between two runs of the same kernel,
and P6, the same run against recorded bits).

What the table fixes for every entry: NA = 3 agents with their own Philox keys, initial weights and replay contents,
K = 3 updates, two rings with cap = n (n = 3 B, the last size of the sampler's dense regime, and n = 3 B + 1, the first
of the sparse one, where candidates collide often), the per-agent ring shifts of the rotated population, the injected
draws, and the host indices of the two upload routes.  No GPU import happens at module level."""
import numpy as np

from oracle import philox

NA, K = 3, 3
SEEDS = (5, 6, 7)
REGIMES = ("dense", "sparse")
PINNED_ENTRIES = 1024          # rlc_h_update_begin: DDPG's indices go through pinned host memory up to this many


def f32(x):
    """float32-representable doubles: the ring and the staging minibatch then hold the same bits as the host arrays"""
    return np.asarray(x, np.float32).astype(np.float64)


class FrontEnd(object):
    """case: a Case of tests/optimizer_state_cases.py (or its WireFitting / OptimalQ / ActorExpert subclass);
    copy: the kernel source file whose front-end call site the case runs; form: what of that call site the case adds"""

    def __init__(self, number, case, copy, form=""):
        self.number, self.case, self.copy, self.form = number, case, copy, form
        self.B, self.S, self.A = case.B, case.S, case.A
        self.seeds = SEEDS
        self._memo = {}

    @property
    def id(self):
        return "%s:%s%s" % (self.copy, self.case.id, "-" + self.form if self.form else "")

    # ---- rings ---------------------------------------------------------------------------------------------------------
    def n(self, regime):
        return {"dense": 3 * self.B, "sparse": 3 * self.B + 1}[regime]

    def shifts(self, n):
        """junk rows added ahead of the n real ones: ring.start of the rotated population.  1: (nearly) no sampled row
        lies past the wrap; n - 1: (nearly) every one does; n - (B + 3): a start inside the ring with both sides in
        every minibatch and the larger share, (n - B - 3) / n = about two thirds, past the wrap (a start of B + 3 itself
        would leave (B + 3) / n, about a third, past it: short of the half that tests/test_front_end_cases.py asks of
        this agent)."""
        return (1, n - 1, n - (self.B + 3))

    def replay(self, agent, n):
        """agent's n rows in replay_add_batch's order, from a generator state of its own"""
        if ("replay", agent, n) not in self._memo:
            s, a, r, s2, g = self.case.replay(np.random.RandomState(7000 + 100 * self.number + 10 * agent + n % 2), n)
            self._memo["replay", agent, n] = (f32(s), f32(a), r, f32(s2), g)
        return self._memo["replay", agent, n]

    def junk(self, agent, count):
        """rows that evict nothing real and must never be gathered: far outside the data, a different value per field"""
        c = float(agent + 1)
        return (np.full((count, self.S), 70.0 + c), np.full((count, self.A), -50.0 - c), np.full(count, -1.0e6 * c),
                np.full((count, self.S), -90.0 - c), np.full(count, 0.5))

    def theta0(self, agent):
        if ("theta0", agent) not in self._memo:
            self._memo["theta0", agent] = self.case.theta0(seed=40 + agent)
        return self._memo["theta0", agent]

    # ---- minibatches ---------------------------------------------------------------------------------------------------
    def sampler_indices(self, n, first_call=0, calls=K):
        """[NA][calls][B]: what the device sampler draws for calls first_call, first_call + 1, ... (oracle/philox.py)"""
        return np.stack([np.stack([philox.sample_distinct(n, self.B, seed, first_call + k) for k in range(calls)])
                         for seed in self.seeds]).astype(np.int64)

    def sampler_rounds(self, n, agent):
        """redraw rounds of agent's K calls"""
        return [philox.sample_distinct_rounds(n, self.B, self.seeds[agent], k)[1] for k in range(K)]

    def wrapped_share(self, n, agent):
        """share of agent's K * B sampled logical indices whose physical slot start + idx lies past the end of the ring"""
        idx = self.sampler_indices(n)[agent]
        return float(np.mean(self.shifts(n)[agent] + idx >= n))

    def draws(self, n_updates, stream=0):
        """the injected draws of update(): eps for SoftActorCritic and the KL agents, u and eps for ActorExpert"""
        rng = np.random.RandomState(9000 + 100 * self.number + stream)
        if self.case.NAME == "ae":
            ns = self.case.dims[6]
            u = np.minimum(rng.random_sample((NA, n_updates, self.B, ns)).astype(np.float32), np.float32(1.0 - 2.0 ** -24))
            return {"u": u, "eps": rng.standard_normal((NA, n_updates, self.B, ns, self.A)).astype(np.float32)}
        if self.case.EPS:
            return {"eps": rng.standard_normal((NA, n_updates, self.B, self.A)).astype(np.float32)}
        return {}

    @staticmethod
    def cut(draws, agents=slice(None), updates=slice(None)):
        return {k: np.ascontiguousarray(v[agents, updates]) for k, v in draws.items()}

    def routes_updates(self):
        """K': the smallest number of updates whose indices no longer fit the pinned buffer, NA * K' * B > 1024"""
        return PINNED_ENTRIES // (NA * self.B) + 1

    def random_indices(self, n, n_updates, stream=0):
        """[NA][n_updates][B] distinct rows per minibatch, not the sampler's"""
        rng = np.random.RandomState(8000 + 100 * self.number + stream)
        return np.stack([rng.choice(n, self.B, replace=False) for _ in range(NA * n_updates)]).reshape(
            NA, n_updates, self.B).astype(np.int64)


def cases():
    from optimizer_state_cases import DDPGCase, KLCase, NAFCase, SACCase
    from test_ddpg_variants import SHAPES as DDPG_LN
    from test_kl import HEADLINE as KL_HEADLINE
    from test_kl_mfma_action2 import SHAPES as KL_A2
    from test_naf import LN_CASES as NAF_LN
    from test_sac import LN_CASES as SAC_LN
    import ae_cases
    import test_gpu_ae
    import test_gpu_optq
    import test_gpu_wf

    small, full, packed = ((8, 2, 64, 48, 40), 17), ((3, 1, 128, 128, 128), 128), ((3, 1, 200, 200, 200), 100)
    rows = [(DDPGCase(*small, kernel="generic"), "ddpg_generic.hip", ""),
            (DDPGCase(*small, kernel="mfma"), "ddpg_mfma_kernel.h", ""),
            (DDPGCase(*full, kernel="generic"), "ddpg_generic.hip", "max_batch"),
            (DDPGCase(*full, kernel="mfma"), "ddpg_mfma_kernel.h", "max_batch"),
            (DDPGCase(*packed, kernel="mfma"), "ddpg_mfma_kernel.h", "packed_pair_tail4"),
            (DDPGCase((9, 1, 64, 48, 40), 17, "mfma"), "ddpg_mfma_kernel.h", "wide"),
            (DDPGCase(*small, kernel="generic", sep=True), "ddpg_generic.hip", ""),
            (DDPGCase(*small, kernel="mfma", sep=True), "ddpg_mfma_kernel.h", ""),
            (DDPGCase(*DDPG_LN[0], kernel="generic", norm=True), "ddpg_generic.hip", ""),
            (DDPGCase((3, 1, 32, 24, 40), 17, "mfma", norm=True), "ddpg_ln_mfma_kernel.h", ""),
            (DDPGCase(*packed, kernel="mfma", split=4), "ddpg_split_kernel.h", ""),
            (SACCase((8, 2, 64, 48, 40, 56), 17, "generic"), "sac_generic.hip", ""),
            (SACCase((8, 2, 64, 48, 40, 56), 17, "mfma"), "sac_mfma_kernel.h", ""),
            (SACCase((17, 6, 64, 48, 40, 56), 32, "mfma"), "sac_mfma_kernel.h", "wide"),
            (SACCase(*SAC_LN[1], kernel="generic", norm=True), "sac_generic.hip", ""),
            (NAFCase((3, 1, 64, 48), 17, "generic"), "naf_generic.hip", ""),
            (NAFCase((3, 1, 64, 48), 17, "mfma"), "naf_mfma_kernel.h", ""),
            (NAFCase((17, 6, 64, 48), 32, "mfma"), "naf_mfma_kernel.h", "wide"),
            (NAFCase(*NAF_LN[0], kernel="generic", norm=True), "naf_generic.hip", "")]
    for kind in ("reverse", "forward"):
        rows += [(KLCase((5, 1, 64, 48, 40, 56), 17, "generic", kind=kind, n_param=9), "kl_generic.hip", ""),
                 (KLCase((5, 1, 64, 48, 40, 56), 17, "mfma", kind=kind, n_param=9), "kl_mfma_kernel.h", "")]
    rows += [(KLCase(*KL_A2[0][:2], kernel="mfma", kind="reverse", l_param=KL_A2[0][2]), "kl_mfma_kernel.h", "action2"),
             (KLCase(KL_HEADLINE, 32, "mfma", kind="forward", n_param=64, split=2), "kl_mfma_kernel.h", "latency"),
             (test_gpu_optq.OptQCase(*test_gpu_optq.UPDATE_CASES[0][:4]), "optq_generic.hip", ""),
             (test_gpu_wf.WFCase((5, 2, 48, 64, 33), 32), "wf_generic.hip", ""),
             (test_gpu_ae.AECase(*ae_cases.SHAPES[1]), "ae_generic.hip", "")]
    return [FrontEnd(i, case, copy, form) for i, (case, copy, form) in enumerate(rows)]


COPIES = ("ddpg_generic.hip", "ddpg_mfma_kernel.h", "ddpg_ln_mfma_kernel.h", "ddpg_split_kernel.h", "sac_generic.hip",
          "sac_mfma_kernel.h", "naf_generic.hip", "naf_mfma_kernel.h", "kl_generic.hip", "kl_mfma_kernel.h",
          "optq_generic.hip", "wf_generic.hip", "ae_generic.hip")
