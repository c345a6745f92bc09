"""The arguments sm_log (csrc/salp_math.h) is tested at, shared by the CPU
accuracy test (tests/test_policy_noise.py) and the device / oracle equality
(tests/test_gpu_parity.py test_device_math_equals_oracle_math)."""
import numpy as np


def log_samples():
    """float64 [n]:
    * the Box-Muller draws' own domain u = k 2^-32, k in 1 .. 2^32: random k, the
      two ends, and the k next to 2^32, where |u - 1| < 2^-20 takes fdlibm's
      short branch;
    * 600 decades, 1e-300 .. 1e300, and the neighbourhood of 1 at float64
      resolution;
    * 0, -0, inf, nan, negative arguments, the smallest normal and denormals."""
    rng = np.random.default_rng(7)
    k = np.concatenate([rng.integers(1, 2 ** 32, 20000, endpoint=True), [1, 2, 3, 2 ** 32, 2 ** 31, 2 ** 31 + 1],
                        2 ** 32 - np.arange(1, 4200, 7), 2 ** 32 - 2 ** np.arange(0, 32)])
    unit = k.astype(np.float64) * 2.0 ** -32
    decades = 10.0 ** rng.uniform(-300, 300, 4000)
    near_one = np.concatenate([1.0 + np.arange(-64, 65) * 2.0 ** -52, 1.0 + rng.uniform(-1, 1, 500) * 2.0 ** -19,
                               1.0 + rng.uniform(-1, 1, 500) * 2.0 ** -21, [np.sqrt(2.0), np.sqrt(0.5), 2.0, 0.5]])
    tiny = np.float64(2.0 ** -1022)
    special = np.array([0.0, -0.0, np.inf, np.nan, -1.0, -np.inf, -5e-324, tiny, np.nextafter(tiny, 0.0), 5e-324,
                        1e-310, 3e-320, 1.7976931348623157e308])
    denormal = rng.integers(1, 2 ** 52, 300).astype(np.uint64).view(np.float64)
    return np.concatenate([unit, decades, near_one, special, denormal])
