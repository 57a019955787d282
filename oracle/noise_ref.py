"""Reparameterisation noise of the native VAE step, regenerated on the CPU.  TEST INFRASTRUCTURE ONLY (see vae_ref.py).

The reference draws ``eps = torch.randn_like(std)`` (lunar_generate.py:259-261) from torch's global generator.  The native step,
when it is not handed ``eps``, draws it inside the head-reduce kernel from a counter generator (lunaris_orion_amd/csrc/lo_train.hip:
``lo_mix64``, ``lo_randn``): sample i of a forward is a function of (call seed, i) alone.  This file restates

  * the integer part bit for bit: ``h = mix64(seed ^ mix64(i))``, ``k1 = h >> 40``, ``k2 = (h >> 8) & 0xFFFFFF``;
  * the two uniforms in float32 exactly as the kernel forms them: ``u1 = (float(k1) + 0.5f) * 2^-24`` -- for ``k1 >= 2^23`` the sum
    is rounded to an integer (ties to even), so ``k1 = 2^24 - 1`` gives ``u1 == 1.0`` and the sample +-0 -- and
    ``u2 = float(k2) * 2^-24`` (exact);
  * Box-Muller's cosine branch in float64: ``sqrt(-2 ln u1) cos(2 pi u2)``.  The kernel evaluates it with ``__logf`` / ``__cosf``
    in float32; that difference is what tests/test_train_ops_gpu.py measures and bounds;
  * the stream of call seeds (lunaris_orion_amd/vae.py, ``LunarisCoreVAE._native_forward``): a first seed from
    (``torch.initial_seed()``, rank), then one step of a 64-bit LCG per forward; forward number k (from 1) runs on ``call_seed(.., k)``.

The smallest ``u1`` is 2^-25 (``k1 = 0``), so no sample exceeds ``sqrt(-2 ln 2^-25)`` = 5.887 in magnitude.
"""
from __future__ import annotations

import math

import numpy as np

M64 = (1 << 64) - 1
LCG_A, LCG_C = 6364136223846793005, 1442695040888963407
MAX_ABS = math.sqrt(-2.0 * math.log(2.0 ** -25))


def mix64(x: np.ndarray) -> np.ndarray:
    """lo_mix64 on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def hash_words(seed: int, first: int, n: int) -> np.ndarray:
    """h of lo_randn for elements first .. first + n - 1 (uint64)."""
    idx = np.arange(n, dtype=np.uint64) + np.uint64(first)
    return mix64(np.uint64(seed & M64) ^ mix64(idx))


def counters(seed: int, first: int, n: int):
    """(k1, k2): the two 24-bit counters the uniforms are made of (uint32)."""
    h = hash_words(seed, first, n)
    return (h >> np.uint64(40)).astype(np.uint32), ((h >> np.uint64(8)) & np.uint64(0xFFFFFF)).astype(np.uint32)


def uniforms(seed: int, first: int, n: int):
    """(u1, u2) as float32 arrays, every operation rounded to float32 like the kernel's: u1 in (0, 1], u2 in [0, 1)."""
    k1, k2 = counters(seed, first, n)
    c = np.float32(1.0 / 16777216.0)
    u1 = (k1.astype(np.float32) + np.float32(0.5)) * c
    u2 = k2.astype(np.float32) * c
    assert u1.dtype == np.float32 and u2.dtype == np.float32
    return u1, u2


def randn(seed: int, first: int, n: int) -> np.ndarray:
    """The samples of elements first .. first + n - 1 for call seed `seed`, float64."""
    u1, u2 = uniforms(seed, first, n)
    return np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(2.0 * np.pi * u2.astype(np.float64))


# ---- what "standard normal and uncorrelated" means for a vector of n = 2^20 samples ------------------------------------------
# Standard errors at n = 2^20: mean 1 / sqrt(n) = 9.8e-4, variance sqrt(2 / n) = 1.4e-3, skewness sqrt(6 / n) = 2.4e-3, excess
# kurtosis sqrt(24 / n) = 4.8e-3, a correlation coefficient 1 / sqrt(n) = 9.8e-4, the Kolmogorov-Smirnov distance about 0.87 / sqrt(n)
# = 8.5e-4 (99.9 % point 1.95 / sqrt(n) = 1.9e-3).  The limits are 4-5 of those; a variance off by 1 %, a u2 that repeats u1's bits
# or one seed reused for two calls misses them by orders of magnitude.
STAT_N = 1 << 20
LIMITS = {"mean": 5e-3, "var": 7e-3, "skew": 2e-2, "kurt": 2e-2, "corr": 5e-3, "ks": 3e-3, "tail_rel": 0.10}
TAIL_3SIGMA = 2.0 * 0.5 * math.erfc(3.0 / math.sqrt(2.0))          # P(|x| > 3) = 2.6998e-3


def corr(a: np.ndarray, b: np.ndarray) -> float:
    a = a.astype(np.float64) - a.mean(dtype=np.float64)
    b = b.astype(np.float64) - b.mean(dtype=np.float64)
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def ks_distance(x: np.ndarray) -> float:
    """sup |F_n - Phi| of the sample x against the standard normal distribution function (float64 erf)."""
    import torch
    s = np.sort(x.astype(np.float64))
    n = s.size
    phi = (0.5 * (1.0 + torch.erf(torch.from_numpy(s) / math.sqrt(2.0)))).numpy()
    i = np.arange(1, n + 1, dtype=np.float64)
    return float(max((i / n - phi).max(), (phi - (i - 1) / n).max()))


def statistics(x: np.ndarray) -> dict:
    """Moments, serial correlations, KS distance, extremes of one vector (any float dtype; computed in float64)."""
    x = x.astype(np.float64)
    m = x.mean()
    d = x - m
    var = (d * d).mean()
    sd = math.sqrt(var)
    return {"mean": float(m), "var": float(var), "skew": float((d ** 3).mean() / sd ** 3), "kurt": float((d ** 4).mean() / var ** 2 - 3.0),
            "lag1": corr(x[:-1], x[1:]), "lag512": corr(x[:-512], x[512:]), "ks": ks_distance(x), "max_abs": float(np.abs(x).max()),
            "tail": float((np.abs(x) > 3.0).mean())}


def assert_standard_normal(st: dict, what: str) -> None:
    """The conditions every vector of STAT_N samples meets (restatement and device alike)."""
    assert abs(st["mean"]) <= LIMITS["mean"], (what, "mean", st)
    assert abs(st["var"] - 1.0) <= LIMITS["var"], (what, "variance", st)
    assert abs(st["skew"]) <= LIMITS["skew"], (what, "skewness", st)
    assert abs(st["kurt"]) <= LIMITS["kurt"], (what, "excess kurtosis", st)
    assert abs(st["lag1"]) <= LIMITS["corr"] and abs(st["lag512"]) <= LIMITS["corr"], (what, "serial correlation", st)
    assert st["ks"] <= LIMITS["ks"], (what, "KS distance", st)
    assert st["max_abs"] <= MAX_ABS, (what, "hard maximum", st)
    assert abs(st["tail"] - TAIL_3SIGMA) <= LIMITS["tail_rel"] * TAIL_3SIGMA, (what, "fraction beyond 3 sigma", st)


def assert_uncorrelated(a: np.ndarray, b: np.ndarray, what: str) -> None:
    c = corr(a, b)
    assert abs(c) <= LIMITS["corr"], (what, "correlation", c)


# the streams every statistics test draws from: torch seeds x ranks x the first four forwards = 32 vectors
STAT_TORCH_SEEDS, STAT_RANKS, STAT_CALLS = (0, 1, 42, 12345), (0, 1), 4

# Edge points of the generator, found by hashing indices 0 .. 2^25 of the first call seed of (torch seed 0, rank 0) on the CPU
# (tests/test_noise_ref.py re-verifies them): k1 == 0 is the smallest u1 = 2^-25, the sample of largest radius the generator has;
# k1 == 2^24 - 1 rounds to u1 == 1.0 in float32, radius exactly 0.
EDGE_SEED = 0xEF8D2B8DC280C3F8
EDGE_INDEX_K1_ZERO = 25342557
EDGE_INDEX_U1_ONE = 10086891


def first_seed(torch_seed: int, rank: int = 0) -> int:
    """The stream's state before its first forward."""
    return (torch_seed * 0x9E3779B97F4A7C15 + 0x5EED + 0xD1B54A32D192ED03 * rank) & M64


def lcg(seed: int) -> int:
    return (seed * LCG_A + LCG_C) & M64


def call_seed(torch_seed: int, rank: int, call: int) -> int:
    """Seed of forward number `call` (1 = the first) of the stream of (torch seed, rank)."""
    assert call >= 1
    s = first_seed(torch_seed, rank)
    for _ in range(call):
        s = lcg(s)
    return s


def call_seeds(torch_seed: int, rank: int, calls: int):
    return [call_seed(torch_seed, rank, k) for k in range(1, calls + 1)]
