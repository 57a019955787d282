"""CPU tests of oracle/noise_ref.py, the numpy restatement of the step's N(0,1) generator (lo_mix64 / lo_randn in
lunaris_orion_amd/csrc/lo_train.hip) and of its stream of call seeds (lunaris_orion_amd/vae.py).  The GPU tests
(tests/test_train_ops_gpu.py) compare the kernel with this restatement element by element; here the restatement itself is shown
to be what it should stand for: standard normal, uncorrelated between elements, forwards and ranks, in step with vae.lcg_advance."""
import math

import numpy as np
import pytest

from oracle import noise_ref as N


@pytest.fixture(scope="module")
def vectors():
    """{(torch seed, rank): [the restatement's float64 vectors of forwards 1..4]}, STAT_N samples each."""
    return {(ts, r): [N.randn(s, 0, N.STAT_N) for s in N.call_seeds(ts, r, N.STAT_CALLS)] for ts in N.STAT_TORCH_SEEDS for r in N.STAT_RANKS}


def test_mix64_matches_a_plain_integer_restatement():
    def mix(x):
        x = (x + 0x9E3779B97F4A7C15) & N.M64
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & N.M64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & N.M64
        return x ^ (x >> 31)
    xs = [0, 1, 2, 0xFFFFFFFFFFFFFFFF, 0x8000000000000000, 0x123456789ABCDEF0, N.EDGE_SEED]
    got = N.mix64(np.array(xs, dtype=np.uint64))
    assert [int(g) for g in got] == [mix(x) for x in xs]
    seed = 0xDEADBEEFCAFEF00D
    h = N.hash_words(seed, 5, 3)
    assert [int(v) for v in h] == [mix(seed ^ mix(i)) for i in (5, 6, 7)]


def test_stream_of_call_seeds_is_the_models():
    """first seed from (torch seed, rank), one LCG step per forward: the constants and the order of lunaris_orion_amd/vae.py, and
    the position a resumed run re-enters at (lcg_advance by the checkpointed count, then the step of the forward itself)."""
    from lunaris_orion_amd import vae as V
    assert (N.LCG_A, N.LCG_C, N.M64) == (V._LCG_A, V._LCG_C, V._M64)
    for ts in N.STAT_TORCH_SEEDS:
        for rank in N.STAT_RANKS:
            f = N.first_seed(ts, rank)
            assert f == (ts * 0x9E3779B97F4A7C15 + 0x5EED + 0xD1B54A32D192ED03 * rank) % (1 << 64)
            seeds = N.call_seeds(ts, rank, 6)
            assert len(set(seeds)) == 6
            for k, s in enumerate(seeds, start=1):
                assert s == V.lcg_advance(f, k) == N.lcg(V.lcg_advance(f, k - 1))
        assert N.first_seed(ts, 0) != N.first_seed(ts, 1)
    assert N.call_seed(0, 0, 1) == N.EDGE_SEED


def test_uniforms_are_formed_in_float32_like_the_kernel():
    """u1 = (float(k1) + 0.5f) * 2^-24 with the sum rounded to float32: exact below 2^23, an integer (ties to even) from 2^23 on."""
    seed = N.EDGE_SEED
    k1, k2 = N.counters(seed, 0, 1 << 16)
    u1, u2 = N.uniforms(seed, 0, 1 << 16)
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    small = k1 < (1 << 23)
    assert small.any() and (~small).any()
    assert np.array_equal(u1[small].astype(np.float64), (k1[small].astype(np.float64) + 0.5) / 2.0 ** 24)
    big = k1[~small].astype(np.int64)
    even = big + (big & 1)                                  # k + 0.5 is a tie: to the even neighbour
    assert np.array_equal(u1[~small].astype(np.float64), even.astype(np.float64) / 2.0 ** 24)
    assert np.array_equal(u2.astype(np.float64), k2.astype(np.float64) / 2.0 ** 24)
    assert u1.min() > 0.0 and u1.max() <= 1.0 and u2.min() >= 0.0 and u2.max() < 1.0


def test_edge_points_are_what_they_are_recorded_as():
    k1, _ = N.counters(N.EDGE_SEED, N.EDGE_INDEX_K1_ZERO, 1)
    u1, _ = N.uniforms(N.EDGE_SEED, N.EDGE_INDEX_K1_ZERO, 1)
    assert int(k1[0]) == 0 and float(u1[0]) == 2.0 ** -25
    x = N.randn(N.EDGE_SEED, N.EDGE_INDEX_K1_ZERO, 1)[0]
    assert math.isfinite(x) and abs(x) <= N.MAX_ABS and abs(x) > 0.4        # radius 5.887 times cos(2 pi 0.7628)
    k1, _ = N.counters(N.EDGE_SEED, N.EDGE_INDEX_U1_ONE, 1)
    u1, _ = N.uniforms(N.EDGE_SEED, N.EDGE_INDEX_U1_ONE, 1)
    assert int(k1[0]) == (1 << 24) - 1 and float(u1[0]) == 1.0
    assert N.randn(N.EDGE_SEED, N.EDGE_INDEX_U1_ONE, 1)[0] == 0.0            # +-0
    assert abs(N.MAX_ABS - 5.887) < 1e-3


def test_first_argument_is_an_offset_into_the_same_sequence():
    a = N.randn(N.EDGE_SEED, 0, 20000)
    assert np.array_equal(N.randn(N.EDGE_SEED, 12345, 4099), a[12345:12345 + 4099])


@pytest.mark.parametrize("torch_seed", N.STAT_TORCH_SEEDS)
@pytest.mark.parametrize("rank", N.STAT_RANKS)
def test_every_vector_is_standard_normal(vectors, torch_seed, rank):
    for k, x in enumerate(vectors[(torch_seed, rank)], start=1):
        st = N.statistics(x)
        print(f"torch seed {torch_seed} rank {rank} forward {k}: " + " ".join(f"{a}={b:.3e}" for a, b in st.items()))
        N.assert_standard_normal(st, (torch_seed, rank, k))


@pytest.mark.parametrize("torch_seed", N.STAT_TORCH_SEEDS)
def test_forwards_and_ranks_are_uncorrelated(vectors, torch_seed):
    for rank in N.STAT_RANKS:
        v = vectors[(torch_seed, rank)]
        for k in range(1, len(v)):
            N.assert_uncorrelated(v[k], v[k - 1], (torch_seed, rank, "forward", k + 1, "with the one before"))
    for k, (a, b) in enumerate(zip(vectors[(torch_seed, 0)], vectors[(torch_seed, 1)]), start=1):
        N.assert_uncorrelated(a, b, (torch_seed, "rank 0 with rank 1 at forward", k))
