"""tests/support.py's own rules, without a GPU: what environ sets, unsets and puts back, and what same_bits calls the same."""
import os

import numpy as np
import pytest

from support import environ, same_bits

SET, ABSENT = 'CROWDNAV_AMD_TEST_SUPPORT_SET', 'CROWDNAV_AMD_TEST_SUPPORT_ABSENT'


@pytest.fixture
def variables(monkeypatch):
    monkeypatch.setenv(SET, 'before')
    monkeypatch.delenv(ABSENT, raising=False)


def test_environ_sets_unsets_and_restores(variables):
    with environ(**{SET: 3, ABSENT: 'x'}):
        assert os.environ[SET] == '3' and os.environ[ABSENT] == 'x'
    assert os.environ[SET] == 'before' and ABSENT not in os.environ
    with environ(**{SET: None, ABSENT: None}):  # None: unset for the duration
        assert SET not in os.environ and ABSENT not in os.environ
    assert os.environ[SET] == 'before' and ABSENT not in os.environ


def test_environ_restores_when_the_body_raises(variables):
    with pytest.raises(KeyError):
        with environ(**{SET: None, ABSENT: 1}):
            assert SET not in os.environ and os.environ[ABSENT] == '1'
            raise KeyError('body')
    assert os.environ[SET] == 'before' and ABSENT not in os.environ


def test_same_bits_compares_dtype_shape_and_bytes():
    assert not same_bits(np.array([0.0]), np.array([-0.0]))                   # equal values, other bytes
    assert not same_bits(np.array([1.0], np.float32), np.array([1.0], np.float64))
    assert not same_bits(np.array([1, 2], np.int32), np.array([1, 2], np.int64))
    assert not same_bits(np.zeros((2, 3)), np.zeros((3, 2)))                  # equal bytes, other shape
    assert not same_bits(np.zeros(6), np.zeros((6, 1)))
    whole = np.arange(24.0).reshape(4, 6)
    view = whole[:, ::2]
    assert not view.flags['C_CONTIGUOUS']
    assert same_bits(view, view.copy()) and same_bits(view.copy(), view)
    assert same_bits(whole.T, np.ascontiguousarray(whole.T))
    assert same_bits(np.array([np.nan, -0.0]), np.array([np.nan, -0.0]))      # bytes, not ==


def test_same_bits_takes_tensors():
    import torch
    t = torch.arange(12, dtype=torch.float64).reshape(3, 4)
    assert same_bits(t, t.numpy().copy()) and same_bits(t.t(), t.t().contiguous().numpy())
    assert not same_bits(t, t.numpy().astype(np.float32)) and not same_bits(torch.zeros(1, dtype=torch.float64), np.array([-0.0]))
