"""The exploration noise of salp_collect's in-kernel policy, on the CPU.

csrc/salp_random.h sr_policy_noise is the function the rollout kernels call
(salp_kernels.hip policy_noise); the oracle library compiles the same header
(oracle.policy_noise, oracle.policy_noise_from_words).  Pinned here:

* sm_log (csrc/salp_math.h), which sits under this noise and the simulator's
  disturbance noise, against mpmath;
* the mapping (noise_seed, global env id, lifetime step counter) -> Philox
  counter and key, written out from sp_draw's definition (csrc/salp_philox.h);
* the Box-Muller arithmetic against mpmath, and at the edge words;
* the distribution of 2^18 draws over consecutive env ids and steps.

tests/test_gpu_collect_policy.py ties the rollout kernels' output to these
functions bit for bit.
"""
import itertools
import math

import mpmath
import numpy as np
import pytest

from log_samples import log_samples
from oracle import oracle

mpmath.mp.prec = 160

LOG_ROW = 23                      # salp_math_selftest's sm_log row (include/salp.h)
STREAM_POLICY = 7                 # SP_STREAM_POLICY
TWO_PI = 6.283185307179586        # the kernel's constant
M32 = 0xFFFFFFFF


def sp_draw_words(seed, env_id, ctr, stream=STREAM_POLICY, group=0):
    """sp_draw (csrc/salp_philox.h) restated: Philox4x32-10 on the counter
    (ctr low, ctr high, env id low, env id bits 32..47 | group << 16) with the
    key (seed low ^ 0x6C8E9CF5 stream, seed high ^ stream)."""
    counter = (ctr & M32, (ctr >> 32) & M32, env_id & M32, ((env_id >> 32) & 0xFFFF) | (group << 16))
    key = ((seed & M32) ^ ((0x6C8E9CF5 * stream) & M32), ((seed >> 32) & M32) ^ stream)
    return oracle.philox(counter, key)


def _sm_log(x):
    x = np.ascontiguousarray(x, np.float64)
    return oracle.math_selftest(x, np.ones_like(x))[LOG_ROW]


# ------------------------------------------------------------------ sm_log
def test_sm_log_within_one_ulp_of_mpmath():
    x = log_samples()
    got = _sm_log(x)
    pos = np.isfinite(x) & (x > 0)
    assert pos.sum() > 25000
    exact = [mpmath.log(mpmath.mpf(float(v))) for v in x[pos]]
    ex64 = np.array([float(e) for e in exact])
    err = np.array([float(abs(mpmath.mpf(float(g)) - e)) for g, e in zip(got[pos], exact)])
    ulps = err / np.spacing(np.abs(ex64))
    nz = ex64 != 0.0
    print(f"sm_log: worst error {ulps[nz].max():.3f} ulp over {int(nz.sum())} arguments")
    assert np.all(ulps[nz] <= 1.0), (x[pos][nz][np.argmax(ulps[nz])], float(ulps[nz].max()))
    # the value Box-Muller's u = 1 (word 0xFFFFFFFF) needs: exactly +0, so that the radius is 0
    one = _sm_log([1.0])
    assert one[0] == 0.0 and not np.signbit(one[0])
    assert np.all(got[pos & (x == 1.0)] == 0.0)
    # fdlibm's special cases
    sp = _sm_log([0.0, -0.0, np.inf, np.nan, -1.0, -np.inf, -5e-324])
    assert sp[0] == -np.inf and sp[1] == -np.inf and sp[2] == np.inf and np.all(np.isnan(sp[3:]))


# ----------------------------------------------------------------- mapping
ENV_IDS = (0, 5, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 5, 2 ** 47 + 3)
SEEDS = (0, 99, 100, 2 ** 32 + 99, 2 ** 63 + 99, 2 ** 64 - 1)
STEPS = (0, 1, 7, 8, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 5)


def test_noise_is_box_muller_on_the_draw_of_seed_global_id_and_step_counter():
    """policy_noise(seed, env, step) is policy_noise_from_words on the Philox
    words of sp_draw(seed, env, step, stream 7, group 0): env ids on both
    sides of 2^32, seeds that differ only in the high word, steps up to
    2^32 + 5.  No two of the triples share their words or their noise."""
    seen = {}
    for seed in SEEDS:
        got = oracle.policy_noise(seed, ENV_IDS, STEPS)
        assert got.shape == (len(ENV_IDS), len(STEPS), 3) and got.dtype == np.float32
        words = np.array([[sp_draw_words(seed, e, s) for s in STEPS] for e in ENV_IDS], np.uint32)
        want = oracle.policy_noise_from_words(words.reshape(-1, 4)).reshape(got.shape)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), seed
        for i, e in enumerate(ENV_IDS):
            for j, s in enumerate(STEPS):
                seen[(seed, e, s)] = (tuple(words[i, j]), got[i, j].tobytes())
    assert len({w for w, _ in seen.values()}) == len(seen)
    assert len({z for _, z in seen.values()}) == len(seen)
    # a draw alone equals its place in a batch
    one = oracle.policy_noise(2 ** 32 + 99, [2 ** 32 + 1], [2 ** 32 + 5])
    assert one.tobytes() == seen[(2 ** 32 + 99, 2 ** 32 + 1, 2 ** 32 + 5)][1]


# ---------------------------------------------------------------- accuracy
def _exact_normals(words):
    """mpmath values of the three normals at the kernel's own inputs:
    u = (w + 1) 2^-32 exactly and the kernel's rounded angle
    fl(6.283185307179586 * (w 2^-32)), a plain float product."""
    out = []
    for w0, w1, w2, w3 in words:
        u1, u3 = mpmath.mpf(int(w0) + 1) / 2 ** 32, mpmath.mpf(int(w2) + 1) / 2 ** 32
        a1, a3 = mpmath.mpf(TWO_PI * (int(w1) * 2.0 ** -32)), mpmath.mpf(TWO_PI * (int(w3) * 2.0 ** -32))
        r1, r3 = mpmath.sqrt(-2 * mpmath.log(u1)), mpmath.sqrt(-2 * mpmath.log(u3))
        out.append((r1 * mpmath.cos(a1), r1 * mpmath.sin(a1), r3 * mpmath.cos(a3)))
    return out


def _ulp(exact, mant_bits, emin):
    """Spacing of the format (mant_bits of precision, smallest exponent emin) at |exact|."""
    if exact == 0:
        return mpmath.mpf(2) ** emin
    e = int(mpmath.floor(mpmath.log(abs(exact), 2)))
    return mpmath.mpf(2) ** max(e - (mant_bits - 1), emin)


def _noise_error_over_bound(words, z):
    worst = 0.0
    for zs, exacts in zip(z, _exact_normals(words)):
        for got, ex in zip(zs, exacts):
            bound = 0.5 * _ulp(ex, 24, -149) + 4 * _ulp(ex, 53, -1074)
            worst = max(worst, float(abs(mpmath.mpf(float(got)) - ex) / bound))
    return worst


def test_noise_within_half_a_float32_ulp_and_four_float64_ulps_of_mpmath():
    """|z - exact| <= 0.5 ulp32(exact) + 4 ulp64(exact).

    The float64 part, counted in ulps of each intermediate (a value with
    mantissa m in [1, 2) and an error of e ulps has the relative error
    e 2^-52 / m):
    * sm_log <= 1 ulp (test_sm_log_within_one_ulp_of_mpmath); -2 * log is exact;
    * sqrt halves the relative error: 1 ulp of rad^2 is at most 0.71 ulp of
      rad (m_rad / m_sq <= sqrt 2), and sqrt rounds once, 0.5: rad <= 1.21 ulp;
    * sin / cos <= 1 ulp at the rounded angle (tests/test_math.py);
    * the product carries 1.21 m_p / m_rad + 1 m_p / m_c ulps of itself, with
      m_p = m_rad m_c when that is below 2 (then <= 1.21 m_c + m_rad <= 3.42)
      and half of it otherwise (<= 2.21), and rounds once, 0.5: <= 3.92 ulp64;
    * one rounding to float32, 0.5 ulp32."""
    rng = np.random.default_rng(3)
    words = rng.integers(0, 2 ** 32, (1500, 4), dtype=np.uint64).astype(np.uint32)
    # the noise of real keys too
    words = np.concatenate([words, np.array([sp_draw_words(99, e, s) for e in range(16) for s in range(16)], np.uint32)])
    z = oracle.policy_noise_from_words(words)
    worst = _noise_error_over_bound(words, z)
    print(f"policy noise: worst error / bound {worst:.3f} over {len(words)} draws")
    assert worst <= 1.0


EDGE = (0, 1, 0x3FFFFFFF, 0x40000000, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF)


def test_noise_at_the_edge_words():
    """Every edge word in every position (the radii, words 0 and 2; the
    angles, words 1 and 3): finite, inside the largest radius, an exact zero
    radius at u = 1, and the axis at angle 0."""
    words = np.array(list(itertools.product(EDGE, repeat=4)), np.uint32)
    z = oracle.policy_noise_from_words(words)
    assert np.isfinite(z).all()
    # the largest radius sqrt(-2 ln 2^-32), as the float32 next to it (a draw on the axis rounds to that)
    rmax = math.sqrt(64 * math.log(2))
    assert np.all(np.abs(z).astype(np.float64) <= float(np.float32(rmax)))
    assert abs(float(np.float32(rmax)) - rmax) <= 0.5 * float(np.spacing(np.float32(rmax)))
    w0, w1 = words[:, 0], words[:, 1]
    u1 = w0 == 0xFFFFFFFF
    assert u1.any() and np.all(z[u1, 0] == 0.0) and np.all(z[u1, 1] == 0.0)
    ax = w1 == 0
    rad = np.sqrt(-2.0 * _sm_log((w0[ax].astype(np.float64) + 1.0) * 2.0 ** -32))
    assert np.all(z[ax, 1] == 0.0) and np.array_equal(z[ax, 0], rad.astype(np.float32))
    assert z[ax, 0].max() == np.float32(rmax)          # word 0 = 0: the largest radius is reached
    assert _noise_error_over_bound(words[::7], z[::7]) <= 1.0


# ------------------------------------------------------------ distribution
GRID = 512
N_DRAWS = GRID * GRID                     # 2^18
DIST_SEED = 2 ** 32 + 99
DIST_ENV0, DIST_STEP0 = 2 ** 32 - 256, 0  # 512 consecutive global ids across 2^32, the first 512 steps


def _corr(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    a, b = a - a.mean(), b - b.mean()
    return float((a * b).sum() / math.sqrt((a * a).sum() * (b * b).sum()))


def _ks_normal(x):
    x = np.sort(np.asarray(x, np.float64).ravel())
    cdf = 0.5 * (1.0 + np.array([math.erf(v) for v in x / math.sqrt(2.0)]))
    n = len(x)
    return float(max((np.arange(1, n + 1) / n - cdf).max(), (cdf - np.arange(0, n) / n).max()))


def distribution_statistics(draw):
    """{name: (value, limit)} for draw(seed, env_ids, steps) -> [envs, steps, 3]."""
    ids, steps = [DIST_ENV0 + i for i in range(GRID)], [DIST_STEP0 + t for t in range(GRID)]
    z = draw(DIST_SEED, ids, steps).astype(np.float64)
    se = 1.0 / math.sqrt(N_DRAWS)
    out = {}
    for c in range(3):
        out[f"mean z{c}"] = (abs(z[..., c].mean()), 5 * se)
        out[f"variance z{c}"] = (abs(z[..., c].var() - 1.0), 5 * math.sqrt(2.0 / N_DRAWS))
        out[f"KS z{c}"] = (_ks_normal(z[..., c]), math.sqrt(-0.5 * math.log(0.5e-6) / N_DRAWS))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        out[f"corr z{a} z{b}"] = (abs(_corr(z[..., a], z[..., b])), 5 * se)
    out["corr z0^2+z1^2 z2^2"] = (abs(_corr(z[..., 0] ** 2 + z[..., 1] ** 2, z[..., 2] ** 2)), 5 * se)
    plus_one = draw(DIST_SEED + 1, ids, steps)
    high = draw(DIST_SEED + 5 * 2 ** 32, ids, steps)
    for c in range(3):
        out[f"corr z{c} next env"] = (abs(_corr(z[:-1, :, c], z[1:, :, c])), 5 * se)
        out[f"corr z{c} next step"] = (abs(_corr(z[:, :-1, c], z[:, 1:, c])), 5 * se)
        out[f"corr z{c} seed + 1"] = (abs(_corr(z[..., c], plus_one[..., c])), 5 * se)
        out[f"corr z{c} seed high word"] = (abs(_corr(z[..., c], high[..., c])), 5 * se)
    # Not one of the correlations above sees a period that divides the grid in
    # the env id or the step (lag 1 of a repeated block is as uncorrelated as
    # lag 1 of fresh draws), and the moments only lose effective samples.
    # Three float32 normals carry > 60 bits, so among 2^18 true draws (2^35
    # pairs) none repeats: every repeated triple is a repeated key.
    flat = np.ascontiguousarray(z.astype(np.float32)).reshape(-1, 3).view([("", np.float32)] * 3)
    out["repeated draws"] = (float(N_DRAWS - len(np.unique(flat))), 0.0)
    return out


def test_noise_distribution_over_512_env_ids_by_512_steps():
    """One fixed draw of N = 2^18: each component's mean (standard error
    1/sqrt N) and variance (sqrt(2/N)) and the correlations (1/sqrt N) between
    the components, between z0^2 + z1^2 and z2^2, with the next env id, the
    next step, seed + 1 and another high seed word within 5 standard errors;
    each component's Kolmogorov-Smirnov distance to N(0, 1) below the 1e-6
    level sqrt(-0.5 ln(0.5e-6) / N) = 0.00526; no draw repeated.

    The test fails for these wrong variants of sr_policy_noise (made in a
    copy of the function, the limits as above; value / limit):
    * the third normal from the first radius: corr z0^2+z1^2 z2^2 0.709 / 0.00977,
      nothing else;
    * the step taken modulo 8: 258 048 repeated draws, KS z0 0.0113, z1 0.0214,
      z2 0.0063 / 0.00526, variance z1 0.0439 / 0.0138, mean z1 0.0197 / 0.00977
      and nine correlations (the largest, z0 with the other high seed word,
      0.0358 / 0.00977);
    * the env id taken modulo 256: 131 072 repeated draws, nothing else (two
      copies of 2^17 good draws pass every moment and correlation above);
    and a seed without its high word: corr z with the other high word 1.0."""
    stats = distribution_statistics(oracle.policy_noise)
    for name, (value, limit) in stats.items():
        print(f"{name}: {value:.3e} (limit {limit:.3e})")
    failed = {k: v for k, v in stats.items() if not v[0] <= v[1]}
    assert not failed, failed
