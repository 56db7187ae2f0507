"""The patterns' even test (csrc/rtc_parity.h) on the host: rtc_debug_even_f64 — the function the device's stripe, ring
and checker patterns call, compiled for the CPU — against fmod(x, 2.0) == 0.0 as numpy evaluates it. Equality everywhere:
random bit patterns (every exponent, NaNs and infinities among them), their floors, integers, both sides of 2^52, 2^53 and
2^54, and the special values."""
import ctypes as C

import numpy as np

from even_parity_cases import even_inputs, fmod_is_zero


def host_even(rtc, x):
    f = rtc.lib().rtc_debug_even_f64
    f.argtypes = [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_uint8)]
    f.restype = C.c_int32
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.full(x.size, 7, dtype=np.uint8)
    assert f(x.ctypes.data_as(C.POINTER(C.c_double)), x.size, out.ctypes.data_as(C.POINTER(C.c_uint8))) == 0
    return out


def test_even_test_equals_fmod_everywhere(rtc):
    for name, x in even_inputs():
        got, want = host_even(rtc, x), fmod_is_zero(x)
        assert set(np.unique(got)) <= {0, 1}, name
        bad = np.flatnonzero(got.astype(bool) != want)
        assert bad.size == 0, (name, bad.size, [x[i].hex() for i in bad[:8]])
    # both answers occur, so the comparison above says something
    assert fmod_is_zero(np.array([4.0]))[0] and not fmod_is_zero(np.array([3.0]))[0]


def test_arguments_are_checked(rtc):
    f = rtc.lib().rtc_debug_even_f64
    f.argtypes = [C.POINTER(C.c_double), C.c_size_t, C.POINTER(C.c_uint8)]
    f.restype = C.c_int32
    assert f(None, 0, None) != 0
