"""Expected match lists of the events tests (test_events.py on the GPU,
test_events_cpu.py without one), derived from the oracle alone.  TEST
INFRASTRUCTURE.

For expected codes exp over a buffer the list is [(i, exp[i]) for i if exp[i]
and len_of_code[exp[i]] >= min_len]; len_of_code comes from the oracle's own
pattern list.
"""
import numpy as np

from oracle_lib import oracle_for

_len = {}


def code_lengths(key):
    """(codes ascending, the byte length of each code's pattern)."""
    if key not in _len:
        d = {(f << 24) | l: len(b) for f, l, b in oracle_for(key).patterns()}
        codes = np.array(sorted(d), dtype=np.uint32)
        lens = np.array([d[int(c)] for c in codes], dtype=np.int64)
        for a in (codes, lens):
            a.setflags(write=False)
        _len[key] = (codes, lens)
    return _len[key]


def lengths_of(key, exp):
    """The pattern length of every position's expected code (0 for none)."""
    codes, lens = code_lengths(key)
    exp = np.asarray(exp, dtype=np.uint32)
    out = np.zeros(len(exp), dtype=np.int64)
    nz = np.nonzero(exp)[0]
    k = np.searchsorted(codes, exp[nz])
    assert np.array_equal(codes[k], exp[nz])
    out[nz] = lens[k]
    return out


def expected_events(key, exp, min_len):
    """(positions int64 ascending, codes) of the expected list."""
    pos = np.nonzero(lengths_of(key, exp) >= max(min_len, 1))[0].astype(np.int64)
    return pos, np.asarray(exp, dtype=np.uint32)[pos]
