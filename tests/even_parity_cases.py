"""Inputs of the even-test checks (csrc/rtc_parity.h), shared by tests/test_host_even_parity.py and
tests/test_gpu_even_parity.py, and the predicate both compare against: fmod(x, 2.0) == 0.0 as numpy evaluates it."""
import numpy as np


def even_inputs(n_random=4_000_000, seed=20260519):
    """(name, values) groups; tests/test_gpu_even_parity.py runs a part of the same values through the device."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 64, size=n_random, dtype=np.uint64).view(np.float64)
    with np.errstate(invalid="ignore"):
        floors = np.floor(bits)
    ints = np.arange(-1_000_000, 1_000_001, dtype=np.float64)
    around = []
    for p in (52, 53, 54):
        c = np.uint64(np.float64(2.0 ** p).view(np.uint64))
        steps = np.arange(-2048, 2049, dtype=np.int64).astype(np.uint64)   # neighbouring doubles on both sides of 2^p
        v = (c + steps).view(np.float64)
        around += [v, -v]
    around = np.concatenate(around)
    tiny, huge = np.float64(5e-324), np.finfo(np.float64).max
    edges = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, tiny, -tiny, 2.0 * tiny, huge, -huge, 2.0 ** 1023, -2.0 ** 1023,
                      1.0, -1.0, 2.0, -2.0, 3.0, 0.5, 1.5, 2.5, -2.5, 2.0 ** 52 + 1.0, 2.0 ** 53 - 1.0, 2.0 ** 53, 2.0 ** 53 + 2.0,
                      2.0 ** -1022, 2.0 ** -1021, 4.0 - 2.0 ** -50, 4.0 + 2.0 ** -50], dtype=np.float64)
    return [("edges", edges), ("around 2^52, 2^53, 2^54", around), ("integers", ints), ("floors", floors), ("random bits", bits)]


def fmod_is_zero(x):
    with np.errstate(invalid="ignore"):
        return np.fmod(x, 2.0) == 0.0
