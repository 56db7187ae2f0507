"""The patterns' even test (csrc/rtc_parity.h) on the device: rtc_device_arith op 7 against fmod(x, 2.0) == 0.0 as numpy
evaluates it, on the special values and on 1 M of the values tests/test_host_even_parity.py puts through the host build."""
import numpy as np
import pytest

from even_parity_cases import even_inputs, fmod_is_zero

pytestmark = pytest.mark.gpu


def test_device_even_test_equals_fmod(gpu):
    groups = dict(even_inputs(n_random=400_000))
    rng = np.random.default_rng(7)
    x = np.concatenate([groups["edges"], groups["around 2^52, 2^53, 2^54"], rng.choice(groups["integers"], 200_000, replace=False),
                        groups["floors"], groups["random bits"]])
    assert x.size >= 1_000_000
    got = gpu.device_arith(7, x)
    assert np.isin(got, (0.0, 1.0)).all()
    bad = np.flatnonzero((got == 1.0) != fmod_is_zero(x))
    assert bad.size == 0, (bad.size, [x[i].hex() for i in bad[:8]])
    assert got[x == 4.0].all() and not got[x == 3.0].any()


def test_op_4_is_still_fmod(gpu):
    x = np.array([0.0, 1.0, 2.0, 3.5, -7.0, 2.0 ** 53 + 2.0])
    assert np.array_equal(gpu.device_arith(4, x), np.fmod(x, 2.0))
