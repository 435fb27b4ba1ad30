"""The minibatch front end of every fused update kernel, pinned bit for bit: "pick B logical indices, map them through the
ring, gather (s, a, r, s', gamma), clip the states".  Picking the indices and locating a row are one shared body in
rlc_common.h; twelve kernels are a call site of it and ddpg_mfma_kernel.h keeps the block typed out (DESIGN.md 4;
tests/front_end_cases.py names all thirteen and holds them to the same properties).  P1 to P5 each compare two
runs of the SAME kernel that must see the same minibatch rows in the same order, P6 compares a run with recorded bits, so
every assertion is an equality and no tolerance appears anywhere.

"State" of an agent: theta, theta_target, every Adam m / v blob of the family, the beta powers (the KL agents: the step
counter) and the family's cheap taps of the last update.

P1  rotation invariance: a ring that wrapped (ring.start = shift_i, junk rows evicted) gives the state of the ring that
    did not, under the device sampler and under host indices, at n = 3 B (dense sampler) and n = 3 B + 1 (sparse).
P2  the fused sampler is oracle/philox.py: update(K) with the device sampler equals update(K, host_indices = the
    restatement's indices); with injected draws this also pins where the draws lie behind the index block.
P3  both upload routes of host indices: K' updates in one launch (more than 1024 indices) equal K' launches of one.
P4  the sample counter: K fused sampler calls leave it at K, host-index updates leave it at 0.
P5  agents are isolated: agent i of three equals a one-agent population with its seed, rows and weights; update_batch(2)
    leaves agents 0 and 1 untouched and gives agent 2 what update(1, host_indices) on the same rows gives it.
P6  the recorded bits: a front end that is wrong the same way in both runs of a pair passes P1 to P5, so the state of
    P1's rotated, device-sampled run (K = 3, three agents) is hashed per agent and must equal the digest in
    tests/golden/front_end_digests.json, recorded by tests/helpers/front_end_digests.py from the build of the commit
    before the thirteen copies were merged.  It makes no run of its own: the lab already holds that one.

The runs of one table entry are shared by the properties that need them (the module-scoped `lab`)."""
import hashlib
import json
import os

import numpy as np
import pytest

import front_end_cases as T
from front_end_cases import K, NA

pytestmark = pytest.mark.gpu


def _population(fe, n, rotated, agents):
    """agents: the table's agent numbers this population holds, in order.  Straight: the n rows into an empty ring
    (ring.start = 0).  Rotated: shift_i junk rows first, then the same n rows: the junk is evicted, ring.start = shift_i,
    the logical content is the same."""
    pop = fe.case.pop(n_agents=len(agents), cap=n, seeds=[fe.seeds[i] for i in agents])
    try:
        shifts = fe.shifts(n)
        for j, i in enumerate(agents):
            pop.set_params(j, fe.theta0(i))
            if rotated:
                pop.replay_add_batch(j, *fe.junk(i, shifts[i]))
            pop.replay_add_batch(j, *fe.replay(i, n))
            assert pop.replay_size(j) == n
    except Exception:
        pop.close()
        raise
    return pop


def _state(fe, pop, j):
    st = fe.case.pop_state(pop, j)
    flat = {"theta": st["theta"], "theta_target": st["theta_target"], "powers": np.asarray(st["pw"])}
    for which in ("m", "v"):
        for slot, blob in st[which].items():
            flat["%s[%s]" % (which, slot)] = blob
    for tap in pop.TAP:
        if not tap.startswith("grads") and tap != "intgrl_q":        # the cheap taps: written with the gradient taps off
            flat["tap " + tap] = pop.last_tap(j, tap)
    return flat


def _same(x, y, label):
    assert set(x) == set(y), label
    differ = ["%s (%d of %d elements)" % (k, int(np.sum(x[k] != y[k])) if x[k].shape == y[k].shape else -1, x[k].size)
              for k in sorted(x) if not np.array_equal(x[k], y[k])]
    assert not differ, "%s: not bit-identical: %s" % (label, ", ".join(differ))


def _ran(fe, state, agent, label):
    """the updates ran (as test_gradient_taps_do_not_change_the_state asserts it) and left numbers"""
    assert np.all(np.isfinite(state["theta"])), label
    assert not np.array_equal(state["theta"], fe.theta0(agent)), label


class Lab(object):
    """the runs of one table entry, each made once: K updates of a straight or rotated population under the device
    sampler or under the restatement's indices, then the state, the whole ring in logical order and the next sample"""

    def __init__(self, fe):
        self.fe, self.runs = fe, {}

    def run(self, regime, rotated, source, agents=tuple(range(NA))):
        key = (regime, rotated, source, agents)
        if key not in self.runs:
            fe, n = self.fe, self.fe.n(regime)
            draws = fe.cut(fe.draws(K), agents=list(agents))
            pop = _population(fe, n, rotated, agents)
            try:
                if source == "sampler":
                    pop.update(K, **draws)
                else:
                    pop.update(K, host_indices=fe.sampler_indices(n)[list(agents)], **draws)
                out = {"state": [_state(fe, pop, j) for j in range(len(agents))],
                       "ring": [pop.replay_gather(j, np.arange(n)) for j in range(len(agents))]}
                out["next"] = [pop.replay_sample_indices(j, fe.B) for j in range(len(agents))]     # advances the counter: last
            finally:
                pop.close()
            for j, i in enumerate(agents):
                _ran(fe, out["state"][j], i, (key, i))
            self.runs[key] = out
        return self.runs[key]


@pytest.fixture(scope="module", params=T.cases(), ids=lambda fe: fe.id)
def lab(request, hip_lib):
    lab = Lab(request.param)
    yield lab
    lab.runs.clear()


@pytest.mark.parametrize("regime", T.REGIMES)
def test_p1_rotation_invariance(lab, regime):
    fe = lab.fe
    n = fe.n(regime)
    for source in ("sampler", "host"):
        straight, rotated = lab.run(regime, False, source), lab.run(regime, True, source)
        for i in range(NA):
            label = "%s %s %s agent %d (shift %d)" % (fe.id, regime, source, i, fe.shifts(n)[i])
            _same(straight["state"][i], rotated["state"][i], label)
            want = fe.replay(i, n)
            for field, a, b, w in zip(("s", "a", "r", "s2", "gamma"), straight["ring"][i], rotated["ring"][i], want):
                assert np.array_equal(a, b), (label, field)
                assert np.array_equal(a, np.asarray(w).reshape(a.shape)), (label, field)     # and both hold the rows added
    print("%s %s: %d agents, ring.start %s against 0: state and ring bit-identical under both sources"
          % (fe.id, regime, NA, fe.shifts(n)))


@pytest.mark.parametrize("regime", T.REGIMES)
def test_p2_fused_sampler_is_the_philox_restatement(lab, regime):
    fe = lab.fe
    sampler, host = lab.run(regime, True, "sampler"), lab.run(regime, True, "host")
    for i in range(NA):
        _same(sampler["state"][i], host["state"][i], "%s %s agent %d (seed %d)" % (fe.id, regime, i, fe.seeds[i]))
    print("%s %s: device sampler == host indices of oracle/philox.py, redraw rounds per agent %s"
          % (fe.id, regime, [fe.sampler_rounds(fe.n(regime), i) for i in range(NA)]))


def test_p3_both_host_index_routes(lab):
    fe = lab.fe
    n, kp = fe.n("sparse"), fe.routes_updates()
    idx, draws = fe.random_indices(n, kp), fe.draws(kp, 1)
    assert idx.size > T.PINNED_ENTRIES >= idx[:, :1].size
    agents = tuple(range(NA))
    one, many = _population(fe, n, True, agents), None
    try:
        many = _population(fe, n, True, agents)
        one.update(kp, host_indices=idx, **draws)                         # one launch, past the pinned buffer
        for k in range(kp):                                               # K' launches, each within it
            many.update(1, host_indices=idx[:, k:k + 1], **fe.cut(draws, updates=slice(k, k + 1)))
        for i in range(NA):
            a, b = _state(fe, one, i), _state(fe, many, i)
            _ran(fe, a, i, (fe.id, i))
            _same(a, b, "%s agent %d: %d updates in one launch against %d launches" % (fe.id, i, kp, kp))
    finally:
        one.close()
        if many is not None:
            many.close()
    print("%s: %d indices in one launch == %d launches of %d" % (fe.id, idx.size, kp, idx[:, :1].size))


@pytest.mark.parametrize("regime", T.REGIMES)
def test_p4_sample_counter(lab, regime):
    fe = lab.fe
    n = fe.n(regime)
    after_sampler, after_host = lab.run(regime, True, "sampler"), lab.run(regime, True, "host")
    call_k, call_0 = fe.sampler_indices(n, K, 1)[:, 0], fe.sampler_indices(n, 0, 1)[:, 0]
    for i in range(NA):
        assert np.array_equal(after_sampler["next"][i], call_k[i]), (fe.id, regime, i, "K fused sampler calls: the next is call K")
        assert np.array_equal(after_host["next"][i], call_0[i]), (fe.id, regime, i, "host indices leave the counter alone")
        assert not np.array_equal(call_k[i], call_0[i])


@pytest.mark.parametrize("regime", T.REGIMES)
def test_p5_agent_equals_a_population_of_one(lab, regime):
    fe = lab.fe
    three = lab.run(regime, True, "sampler")
    for i in range(NA):
        alone = lab.run(regime, True, "sampler", agents=(i,))
        _same(three["state"][i], alone["state"][0], "%s %s agent %d of %d against a population of one" % (fe.id, regime, i, NA))
        assert np.array_equal(three["next"][i], alone["next"][0]), (fe.id, regime, i)


def test_p5_update_batch_touches_one_agent(lab):
    fe = lab.fe
    n, agent = fe.n("sparse"), 2
    idx, draws = fe.random_indices(n, 2, 2), fe.draws(2, 2)
    agents = tuple(range(NA))
    pop, twin = _population(fe, n, True, agents), None
    try:
        twin = _population(fe, n, True, agents)
        for p in (pop, twin):                                             # a first update: m, v and the taps of every agent non-zero
            p.update(1, host_indices=idx[:, :1], **fe.cut(draws, updates=slice(0, 1)))
        before = [_state(fe, pop, i) for i in range(NA)]
        j = idx[agent, 1]
        s, a, r, s2, g = fe.replay(agent, n)                              # float32-representable: staging holds the ring's bits
        pop.update_batch(agent, s[j], a[j], s2[j], r[j], g[j], **{k: v[agent, 1] for k, v in draws.items()})
        twin.update(1, host_indices=idx[:, 1:2], **fe.cut(draws, updates=slice(1, 2)))
        after = [_state(fe, pop, i) for i in range(NA)]
        want = _state(fe, twin, agent)
    finally:
        pop.close()
        if twin is not None:
            twin.close()
    for i in range(NA):
        _ran(fe, before[i], i, (fe.id, i))
        if i != agent:
            _same(before[i], after[i], "%s agent %d across update_batch(%d)" % (fe.id, i, agent))
    assert not np.array_equal(after[agent]["theta"], before[agent]["theta"])
    _same(after[agent], want, "%s agent %d: update_batch against update(1, host_indices) on the same rows" % (fe.id, agent))


def state_digest(state):
    """sha256 over the sorted keys of one agent's _state: for each key its name, dtype, shape and raw bytes"""
    h = hashlib.sha256()
    for k in sorted(state):
        v = np.ascontiguousarray(state[k])
        h.update(("%s|%s|%s|" % (k, v.dtype.str, v.shape)).encode())
        h.update(v.tobytes())
    return h.hexdigest()


def digest_key(fe, regime, agent):
    return "%s %s agent %d" % (fe.id, regime, agent)


def lab_digests(lab):
    """{digest_key: digest} of P1's rotated device-sampler run in both regimes"""
    return {digest_key(lab.fe, regime, i): state_digest(lab.run(regime, True, "sampler")["state"][i])
            for regime in T.REGIMES for i in range(NA)}


@pytest.mark.parametrize("regime", T.REGIMES)
def test_p6_state_has_the_recorded_bits(lab, golden_dir, regime):
    fe = lab.fe
    with open(os.path.join(golden_dir, "front_end_digests.json")) as f:     # a missing file or key fails
        want = json.load(f)["digests"]
    got = lab_digests(lab)
    for i in range(NA):
        key = digest_key(fe, regime, i)
        assert got[key] == want[key], key
