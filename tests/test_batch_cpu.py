"""The batched scan's host-side pieces that need no device: pm.batch_offsets,
and the precondition of the GPU tests' input T (tests/batch_inputs.py),
checked with the oracle alone so a change to the recipe that weakens it is
seen on any machine."""
import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import T_BYTES, input_t, precondition


def _check(offs, lens):
    assert isinstance(offs, np.ndarray) and offs.dtype == np.int64
    assert offs.shape == (len(lens) + 1,)
    assert offs[0] == 0 and offs[-1] == sum(lens)
    assert np.array_equal(np.diff(offs), np.asarray(lens, dtype=np.int64))


def test_batch_offsets_empty_list():
    _check(pm.batch_offsets([]), [])


def test_batch_offsets_empty_members():
    _check(pm.batch_offsets([b"", b"abc", b"", b"", b"z", b""]), [0, 3, 0, 0, 1, 0])
    _check(pm.batch_offsets([b"", b""]), [0, 0])


def test_batch_offsets_mixed_types():
    bufs = [b"GET /", bytearray(b"\x00\x01\x02"), np.arange(300, dtype=np.uint8), memoryview(b"xy"),
            np.empty(0, np.uint8)]
    _check(pm.batch_offsets(bufs), [5, 3, 300, 2, 0])


# the issue's figures for this recipe: (differ, of those >= 8 bytes in)
T_FIGURES = {"et": (504, 223), "snort": (582, 232), "merged": (723, 330)}


@pytest.mark.parametrize("key", ["et", "snort", "merged"])
def test_input_t_precondition(key):
    text, offs, exp = input_t(key)
    assert len(text) == T_BYTES and offs[0] == 0 and offs[-1] == T_BYTES
    assert np.all(np.diff(offs) >= 0)
    assert len(offs) - 1 == 385
    assert int(np.count_nonzero(np.diff(offs) == 0)) == 5
    differ, deep = precondition(key)
    print(f"{key}: {differ} positions differ, {deep} of them >= 8 bytes into their stream")
    assert differ >= 300 and deep >= 100
    assert (differ, deep) == T_FIGURES[key]
