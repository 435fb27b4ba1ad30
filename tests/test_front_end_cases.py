"""The table of tests/front_end_cases.py can fail: on the CPU restatement of the sampler alone (oracle/philox.py) every
entry reaches the regime switch from both sides, runs the redraw path of the sparse regime for every agent, hands every
update and every agent its own rows, and puts the sampled rows of two of the three agents mostly past the wrap of the
rotated ring.  These are conditions on the table, not measurements of a kernel: where one fails, the table changes (a
seed, a shift), never the condition."""
import numpy as np
import pytest

import front_end_cases as T

CASES = T.cases()


def test_every_front_end_copy_has_a_case():
    assert sorted({fe.copy for fe in CASES}) == sorted(T.COPIES) and len(T.COPIES) == 13
    assert len({fe.id for fe in CASES}) == len(CASES)
    forms = {(fe.copy, fe.form) for fe in CASES}
    for want in (("ddpg_mfma_kernel.h", "wide"), ("sac_mfma_kernel.h", "wide"), ("naf_mfma_kernel.h", "wide"),
                 ("ddpg_mfma_kernel.h", "max_batch"), ("ddpg_generic.hip", "max_batch"), ("kl_mfma_kernel.h", "action2"),
                 ("kl_mfma_kernel.h", "latency"), ("ddpg_mfma_kernel.h", "packed_pair_tail4")):
        assert want in forms, want
    assert any(fe.B == 128 and fe.n("dense") == 384 for fe in CASES)       # the dense pool of 3 * RLC_MAX_BATCH ints, full


@pytest.mark.parametrize("fe", CASES, ids=lambda fe: fe.id)
def test_table_conditions(fe):
    B = fe.B
    assert T.NA == 3 and T.K == 3 and len(set(fe.seeds)) == T.NA
    assert 3 * B >= fe.n("dense") and 3 * B < fe.n("sparse")                 # the two sides of rlc_sample_distinct's switch
    thetas = [fe.theta0(i) for i in range(T.NA)]
    for i in range(T.NA):
        for j in range(i):
            assert not np.array_equal(thetas[i], thetas[j]), (i, j)
    for regime in T.REGIMES:
        n = fe.n(regime)
        idx = fe.sampler_indices(n)
        assert idx.shape == (T.NA, T.K, B) and idx.min() >= 0 and idx.max() < n
        shifts = fe.shifts(n)
        rows = [fe.replay(i, n) for i in range(T.NA)]
        for i in range(T.NA):
            rounds = fe.sampler_rounds(n, i)
            share = fe.wrapped_share(n, i)
            print("%s %s n %d agent %d (seed %d, shift %d): redraw rounds %s, %.0f %% of the sampled rows past the wrap"
                  % (fe.id, regime, n, i, fe.seeds[i], shifts[i], rounds, 100.0 * share))
            assert all(len(set(idx[i, k])) == B for k in range(T.K))
            if regime == "sparse":
                assert max(rounds) >= 1, (i, rounds)         # the flag / redraw path of the fused sampler runs
            else:
                assert rounds == [0] * T.K
            for k in range(T.K):                             # every update its own rows (as sets and in order) ...
                for k2 in range(k):
                    assert set(idx[i, k]) != set(idx[i, k2]), (i, k, k2)
            for j in range(i):                               # ... and every agent: another agent's rows or order shows
                for k in range(T.K):
                    assert set(idx[i, k]) != set(idx[j, k]), (i, j, k)
                assert not np.array_equal(rows[i][0], rows[j][0]) and not np.array_equal(rows[i][2], rows[j][2])
            assert shifts[i] % n != 0, (i, shifts[i])
            assert 0 < shifts[i] < n
        # which agent covers which side of the wrap: agent 0 (shift 1) the near side, almost no sampled row wraps;
        # agent 1 (shift n - 1) the far side, almost every one wraps; agent 2 (shift n - B - 3) both sides in one
        # minibatch, most of them past the wrap.  The half-rule holds for agents 1 and 2.
        assert fe.wrapped_share(n, 0) < 0.5
        assert fe.wrapped_share(n, 1) >= 0.5 and fe.wrapped_share(n, 2) >= 0.5
        both = shifts[2] + idx[2] >= n
        assert all(both[k].any() and not both[k].all() for k in range(T.K))   # agent 2: a straddling minibatch every update
    # the two upload routes of host indices
    kp = fe.routes_updates()
    assert T.NA * kp * B > T.PINNED_ENTRIES >= T.NA * (kp - 1) * B and T.NA * B <= T.PINNED_ENTRIES
    ridx = fe.random_indices(fe.n("sparse"), kp)
    assert ridx.shape == (T.NA, kp, B) and ridx.max() < fe.n("sparse")
    assert all(len(set(ridx[i, k])) == B for i in range(T.NA) for k in range(kp))
    for d in (fe.draws(T.K), fe.draws(kp, 1)):
        assert set(d) == ({"u", "eps"} if fe.case.NAME == "ae" else {"eps"} if fe.case.EPS else set())
        assert all(v.dtype == np.float32 and v.shape[0] == T.NA for v in d.values())
        assert "u" not in d or (d["u"].min() >= 0.0 and d["u"].max() < 1.0)
