"""CPU-only tests of the gamma threshold tables behind the device's Canvas::to_imgbuf (csrc/rtc_gamma.h, rtc_gamma_thresholds):
the lookup rule — restated here in numpy, and the header's own code run on the host — gives exactly the bytes of the host
conversion rtc_canvas_to_rgba8 (glibc pow) on special values, every threshold +-50 ulp and a million random values."""
import ctypes as C

import numpy as np
import pytest

GAMMAS = [1.0, 2.2, 1.8, 0.5, 0.3, 3.7, 1e-39, 1e20]   # 1e-39: a subnormal f32, 1/gamma overflows to +inf
INF_BITS = 0x7FF0000000000000


def exponent(gamma: float) -> float:
    """e = (double)(1.0f / gamma), as color.rs:55-65 and rtc_canvas_to_rgba8 take it."""
    with np.errstate(over="ignore"):
        return float(np.float32(1.0) / np.float32(gamma))


def restated(T: np.ndarray, e: float, c: np.ndarray) -> np.ndarray:
    """The lookup rule of rtc_gamma.h over the table: #{k : T[k] <= |c|}, then pow's rules for a set sign bit and NaN."""
    out = np.searchsorted(T, np.abs(c), side="right").astype(np.int64)
    neg = np.signbit(c) & ~np.isnan(c)
    if not (np.isinf(e) or (e == np.floor(e) and np.fmod(e, 2.0) == 0.0)):   # even integers and +inf: pow(c, e) = pow(|c|, e)
        if e == np.floor(e):
            out[neg] = 0                                                         # odd integer: a result <= -0
        else:
            out[neg] = np.where(c[neg] == -np.inf, 255, 0)                       # NaN, except pow(-inf, e) = +inf
    out[np.isnan(c)] = 0
    return out.astype(np.uint8)


def host_bytes(rtc, c: np.ndarray, gamma: float) -> np.ndarray:
    """rtc_canvas_to_rgba8 (the host's pow) on the values as the channels of a 1-pixel-wide canvas."""
    pad = (-len(c)) % 3
    canvas = np.concatenate([c, np.zeros(pad)]).reshape(-1, 1, 3)
    return rtc.to_rgba8(canvas, gamma)[:, :, :3].reshape(-1)[: len(c)]


def sample(T: np.ndarray, seed: int = 1) -> np.ndarray:
    """+-0, +-inf, NaNs, subnormals, negatives, values above 1, every finite threshold +-50 ulp (and their negatives),
    10^6 random values in [-0.5, 1.5]."""
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, -np.nan, 5e-324, -5e-324, 2.2250738585072014e-308 / 3, -1e-310, 1e-300,
                        -1.0, -0.5, -1e-5, -2.0, -1e300, 1.0, np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), 1.5, 2.0, 255.0, 1e10,
                        1e300, 1.7976931348623157e308, 1.0 / 255.0, 254.0 / 255.0])
    bits = T[np.isfinite(T)].view(np.int64)
    near = (bits[:, None] + np.arange(-50, 51, dtype=np.int64)[None, :]).reshape(-1)
    near = near[(near >= 0) & (near <= INF_BITS)].view(np.float64)
    rnd = np.random.default_rng(seed).uniform(-0.5, 1.5, 1_000_000)
    return np.concatenate([special, near, -near, rnd])


@pytest.mark.parametrize("gamma", GAMMAS)
def test_threshold_lookup_equals_host_conversion(rtc, gamma):
    T = rtc.gamma_thresholds(gamma)
    assert T.shape == (255,) and T.dtype == np.float64
    assert np.all(T[1:] >= T[:-1]), "thresholds must be non-decreasing"
    c = sample(T)
    want = host_bytes(rtc, c, gamma)
    got = restated(T, exponent(gamma), c)
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, f"gamma {gamma}: {bad.size} mismatches, e.g. c={c[bad[:5]]!r} got {got[bad[:5]]} want {want[bad[:5]]}"


@pytest.mark.parametrize("gamma", GAMMAS)
def test_shared_header_lookup_equals_host_conversion(rtc, gamma):
    """The lookup code the kernels run (rtc_gamma.h), compiled for the host: with the f32 estimate's guess, and with a
    guess that is always wrong so that every value takes the binary search."""
    fn = rtc.lib().rtc_debug_gamma_lookup
    fn.restype = C.c_int32
    fn.argtypes = [C.c_float, C.POINTER(C.c_double), C.c_size_t, C.c_uint32, C.POINTER(C.c_uint8)]
    c = sample(rtc.gamma_thresholds(gamma), seed=2)
    want = host_bytes(rtc, c, gamma)
    for guess in (0, 1):
        got = np.empty(len(c), dtype=np.uint8)
        assert fn(gamma, c.ctypes.data_as(C.POINTER(C.c_double)), len(c), guess, got.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
        bad = np.nonzero(got != want)[0]
        assert bad.size == 0, f"gamma {gamma}, guess mode {guess}: {bad.size} mismatches, e.g. c={c[bad[:5]]!r}"


def test_gamma_one_table_is_color_scale(rtc):
    """e = 1: the table reproduces Color::scale(c, 255) exactly (rtc_render_rgb8's bytes)."""
    T = rtc.gamma_thresholds(1.0)
    c = sample(T, seed=3)
    assert np.array_equal(restated(T, 1.0, c), rtc.color_scale255(c))


def test_extreme_gammas_tables(rtc):
    """e = +inf (gamma 1e-39): pow(c, inf) is 0 below 1 and 255 from 1 on, so every threshold is 1.0. e = 1e-20 (gamma
    1e20): pow(c, e) rounds to 1 for every positive double, so every threshold is the smallest subnormal."""
    assert np.all(rtc.gamma_thresholds(1e-39) == 1.0)
    assert np.all(rtc.gamma_thresholds(1e20) == 5e-324)


@pytest.mark.parametrize("gamma", [0.0, -0.0, -1.0, -2.2, float("nan"), float("inf"), float("-inf")])
def test_invalid_gamma_is_rejected(rtc, gamma):
    with pytest.raises(rtc.RtcError) as ei:
        rtc.gamma_thresholds(gamma)
    assert ei.value.status == 4   # RTC_ERR_ARG
