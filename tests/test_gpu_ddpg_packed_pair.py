"""The fused forward pairs of the DDPG MFMA kernel at thirteen N tiles: the ragged 13th tile of the actor's and the
critic's second layers packed into ONE 16-column MFMA tile (widths 193..200: at most 8 real columns in the tile;
mfma_blocks.h, fwd_gemm2's PACK) against the unpacked path (widths 201..208), and the phase merges of the update
(TD target in the dq phase, one end-of-update barrier).

Parity against the oracle with the helpers and the 1e-5 bar of tests/test_gpu_ddpg.py.  Where the MFMA kernel does not
take a shape the case asserts the refusal and the limit it names (the kernel takes widths that are multiples of four,
and a 13-tile width above 200 has a 264-float activation row: seven batch tiles of those are more LDS than a workgroup
gets), so that a change of those limits shows up here.

The digests of tests/golden/ddpg_packed_pair_digests.json were recorded from the build of the commit BEFORE the packed
tile and the phase merges went in (tests/helpers/packed_pair_digests.py writes the file): the kernel's results after
them are the same bits.
"""
import hashlib
import json
import os

import numpy as np
import pytest

from test_gpu_ddpg import AMAX, SMAX, SMIN, _batch, _cos, _make, _oracle, _rel

pytestmark = pytest.mark.gpu

PACKED_WIDTHS = (193, 196, 200)          # 13 tiles, 1..8 real columns in the last
UNPACKED_WIDTHS = (201, 204, 208)        # 13 tiles, 9..16 real columns in the last
NETS = ((3, 1), (8, 2))
CASES = [(S, A, w, B) for (S, A) in NETS for w in PACKED_WIDTHS + UNPACKED_WIDTHS for B in (17, 32, 100)]
CASES += [(S, A, 200, 112) for (S, A) in NETS]                 # seven padded tiles, no tail-of-four unit
DIGEST_CASES = [(3, 1, 200, 100), (3, 1, 200, 32), (8, 2, 200, 100), (8, 2, 200, 32)]


def _refusal(width, B):
    """the limit rlc_ddpg_set_kernel names for a shape outside the MFMA kernel's range, or None (ddpg_mfma.hip)"""
    if width % 4:
        return "multiples of 4"
    if width > 200 and B > 64:           # LDH 264 x 112 rows
        return r"\d+ bytes of LDS"
    return None


def _pop_or_refusal(S, A, width, B, **kw):
    from rlcontrol_amd._lib import RlcError
    dims = (S, A, width, width, width)
    pop, smin, smax, amax = _make(dims, B, **kw)
    why = _refusal(width, B)
    if why is not None:
        with pytest.raises(RlcError, match=why):
            pop.set_kernel("mfma")
        pop.close()
        return None
    pop.set_kernel("mfma")
    assert pop.kernel_in_use() == "mfma"
    return dims, pop, smin, smax, amax


@pytest.mark.parametrize("S,A,width,B", CASES)
def test_single_update_taps_and_gradients(hip_lib, S, A, width, B):
    from oracle.ddpg import Dims, init_params
    made = _pop_or_refusal(S, A, width, B)
    if made is None:
        return
    dims, pop, smin, smax, amax = made
    pop.enable_grad_taps(True)
    th = init_params(Dims(*dims), 3)
    pop.set_params(0, th)
    o = _oracle(dims, th, (1e-3, 1e-2), smin, smax, amax)
    s, a, s2, r, g = _batch(np.random.RandomState(11), B, S, A)
    pop.update_batch(0, s, a, s2, r, g)
    taps = o.update(s, a, s2, r, g, taps=True)
    for name in ("q", "y", "a_out", "dqda"):
        assert _rel(pop.last_tap(0, name), taps[name]) < 1e-5, name
    lay, P = Dims(*dims).layout()
    for which in ("grads_c", "grads_a"):
        got, want = pop.last_tap(0, which), taps[which]
        assert _cos(got, want) > 1 - 1e-9, which
        for name, (off, shp) in lay.items():
            n = int(np.prod(shp))
            if np.any(want[off:off + n]):
                assert _rel(got[off:off + n], want[off:off + n]) < 1e-5, (which, name)
            else:
                assert not np.any(got[off:off + n]), (which, name)
    assert _rel(pop.get_blob(0, "theta_target"), o.theta_t) < 1e-5
    assert np.allclose(pop.get_beta_powers(0), o.pw, rtol=1e-6)
    pop.close()


@pytest.mark.parametrize("S,A,width,B", CASES)
def test_ten_updates_from_host_indices(hip_lib, S, A, width, B):
    """ten updates from the replay with host-drawn indices: the first within 1e-5 of the oracle, the trajectory within the
    2e-4 that tests/test_gpu_ddpg.py gives rounding differences compounding through Adam"""
    from oracle.ddpg import Dims, init_params
    N = 1024
    made = _pop_or_refusal(S, A, width, B, cap=N)
    if made is None:
        return
    dims, pop, smin, smax, amax = made
    th = init_params(Dims(*dims), 0)
    pop.set_params(0, th)
    rng = np.random.RandomState(7)
    s, a, s2, r, g = _batch(rng, N, S, A)
    pop.replay_add_batch(0, s, a, r, s2, g)
    o = _oracle(dims, th, (1e-3, 1e-2), smin, smax, amax)
    for it in range(10):
        idx = rng.choice(N, B, replace=False).astype(np.int64)
        pop.update(1, host_indices=idx)
        # the oracle sees what the device gathers: states clipped on the way in by both
        taps = o.update(s[idx], a[idx], s2[idx], r[idx], g[idx], taps=True)
        tol = 1e-5 if it == 0 else 2e-4
        for name in ("q", "y", "a_out", "dqda"):
            assert _rel(pop.last_tap(0, name), taps[name]) < tol, (it, name)
    assert _rel(pop.get_blob(0, "theta_target"), o.theta_t) < 1e-4
    pop.close()


def _sampled_population(S, A, width, B, N=3000):
    """one agent on the MFMA kernel with a seeded replay, ready for device-sampled updates"""
    from oracle.ddpg import Dims, init_params
    dims = (S, A, width, width, width)
    pop, _, _, _ = _make(dims, B, cap=N, seeds=[4242])
    pop.set_kernel("mfma")
    pop.set_params(0, init_params(Dims(*dims), 5))
    rng = np.random.RandomState(3)
    pop.replay_add_batch(0, rng.randn(N, S), rng.randn(N, A), rng.randn(N), rng.randn(N, S), np.full(N, 0.99))
    return pop


STATE = ("theta", "theta_target", "actor_m", "actor_v", "critic_m", "critic_v")


@pytest.mark.parametrize("S,A,width,B", DIGEST_CASES)
def test_three_updates_in_one_launch_equal_three_launches(hip_lib, S, A, width, B):
    """device-sampled updates: bit-identical parameters, Adam m / v, targets, taps and beta powers either way, and the
    sampler's stream in the same place afterwards (the next draw is the same index set)"""
    got = []
    for launches in ((3,), (1, 1, 1)):
        pop = _sampled_population(S, A, width, B)
        for k in launches:
            pop.update(k)
        state = [pop.get_blob(0, w) for w in STATE] + [pop.last_tap(0, t) for t in ("q", "y", "a_out", "dqda")]
        state += [pop.get_beta_powers(0), pop.replay_sample_indices(0, B)]
        got.append(state)
        pop.close()
    for x, y in zip(*got):
        assert np.array_equal(x, y)


def state_digests(S, A, width, B):
    """sha256 of the raw float32 bytes of theta, theta_target, the four taps and the beta powers after five
    device-sampled updates (three in one launch, then two)"""
    pop = _sampled_population(S, A, width, B)
    pop.update(3)
    pop.update(2)
    out = {}
    for name in ("theta", "theta_target"):
        out[name] = pop.get_blob(0, name)
    for name in ("q", "y", "a_out", "dqda"):
        out[name] = pop.last_tap(0, name)
    out["beta_powers"] = pop.get_beta_powers(0)
    pop.close()
    return {k: hashlib.sha256(np.ascontiguousarray(v, np.float32).tobytes()).hexdigest() for k, v in out.items()}


def digest_key(S, A, width, B):
    return "S%d_A%d_H%d_B%d" % (S, A, width, B)


@pytest.mark.parametrize("S,A,width,B", DIGEST_CASES)
def test_state_after_five_updates_has_the_recorded_bits(hip_lib, golden_dir, S, A, width, B):
    with open(os.path.join(golden_dir, "ddpg_packed_pair_digests.json")) as f:
        want = json.load(f)["digests"][digest_key(S, A, width, B)]
    assert state_digests(S, A, width, B) == want
