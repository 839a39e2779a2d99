"""Group tables and expected lists of the pattern-group tests (test_groups.py
on the GPU, test_groups_cpu.py without one).  TEST INFRASTRUCTURE.

The tables are fixed functions of a pattern's bytes and a stream's index; the
expected lists come from the oracle's answers, the suffixes found by
byte-string lookup over the oracle's patterns (match_inputs.suffix_chains) and
these tables.  The library's parent[] and reach[] play no part.
"""
import zlib

import numpy as np

from event_inputs import code_lengths
from match_inputs import expected_matches
from oracle_lib import oracle_for

ALL_GROUPS = 0xFFFFFFFF
TABLE = [1 << k for k in range(8)] + [0x3, 0x1FF, 0, ALL_GROUPS, 1 << 8, 1 << 31]

_cm = {}


def pattern_mask(b):
    """The fixed group mask of a pattern's bytes: none for one pattern in 11,
    else one of groups 0..7, a quarter of them also in group 8."""
    c = zlib.crc32(b)
    if (c >> 5) % 11 == 0:
        return 0
    return (1 << (c & 7)) | ((1 << 8) if (c >> 3) & 3 == 0 else 0)


def all_ones(b):
    return ALL_GROUPS


def stream_masks(nseg):
    """Stream j is scanned for TABLE[j % 14]."""
    return np.array([TABLE[j % len(TABLE)] for j in range(nseg)], dtype=np.uint32)


def masks_by_index(d, fn=pattern_mask):
    """One mask per pattern of a pm.Dictionary, in its (add) order."""
    return np.array([fn(p) for p in d.patterns()], dtype=np.uint32)


def code_masks(key, fn=pattern_mask):
    """(codes ascending, the mask of each code's pattern bytes)."""
    if (key, fn) not in _cm:
        d = {(f << 24) | l: fn(b) for f, l, b in oracle_for(key).patterns()}
        codes = np.array(sorted(d), dtype=np.uint32)
        _cm[(key, fn)] = (codes, np.array([d[int(c)] for c in codes], dtype=np.uint32))
    return _cm[(key, fn)]


def stream_of(offs, pos):
    """The stream holding each position: the last one that begins at or
    before it (of a run of empty streams: the last of the run)."""
    offs = np.asarray(offs, dtype=np.int64)
    return np.clip(np.searchsorted(offs, pos, side="right") - 1, 0, len(offs) - 2)


def expected_groups(key, exp, offs, sgroups, min_len, all_matches, fn=pattern_mask):
    """(positions int64, codes u32), ascending by (position, code): of every
    pattern of at least min_len bytes ending at a position, those whose mask
    meets the mask of the position's stream; all_matches false: of these the
    longest one per position."""
    pos, codes = expected_matches(key, exp, min_len)
    cm_codes, cm_masks = code_masks(key, fn)
    pmask = cm_masks[np.searchsorted(cm_codes, codes)]
    smask = np.asarray(sgroups, dtype=np.uint32)[stream_of(offs, pos)]
    vis = (pmask & smask) != 0
    pos, codes = pos[vis], codes[vis]
    if not all_matches and len(pos):
        lc, ll = code_lengths(key)
        ln = ll[np.searchsorted(lc, codes)]
        order = np.lexsort((-ln, pos))
        pos, codes = pos[order], codes[order]
        head = np.concatenate([[True], pos[1:] != pos[:-1]])
        pos, codes = pos[head], codes[head]
    return pos, codes


def group_stats(key, exp, offs, sgroups, min_len):
    """(unmasked all events, masked all events, masked longest events, those
    of them whose pattern is not the full dictionary's answer, positions with
    >= 2 masked events, streams with a masked event)."""
    exp = np.asarray(exp, dtype=np.uint32)
    unmasked = len(expected_matches(key, exp, min_len)[0])
    ap, _ = expected_groups(key, exp, offs, sgroups, min_len, True)
    lp, lcodes = expected_groups(key, exp, offs, sgroups, min_len, False)
    per = np.unique(ap, return_counts=True)[1]
    return (unmasked, len(ap), len(lp), int(np.count_nonzero(lcodes != exp[lp])), int(np.count_nonzero(per >= 2)),
            len(np.unique(stream_of(offs, ap))))
