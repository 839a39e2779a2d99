"""Window tables and expected lists of the pattern-window tests
(test_windows.py on the GPU, test_windows_cpu.py without one).  TEST
INFRASTRUCTURE.

A pattern's window is a fixed function of its bytes (window_of); the expected
lists come from the oracle's answers, the suffixes found by byte-string lookup
over the oracle's patterns (match_inputs.expected_matches), the oracle's
pattern lengths, group_inputs' masks and this table.  The library's parent /
reach / window tables play no part.
"""
import zlib

import numpy as np

from event_inputs import code_lengths
from flow_inputs import F_FLOW_BYTES, F_FLOWS
from group_inputs import code_masks, pattern_mask, stream_of
from match_inputs import expected_matches
from oracle_lib import oracle_for

INF = 0xFFFFFFFF

_cw = {}


def window_sel(b):
    return zlib.crc32(b) % 8


def window_of(b):
    """(min_start, max_end) of a pattern's bytes.  sel 0-2: unbounded; 3:
    anchored at the stream's start; 4: within the first 64 bytes; 5: not
    before an offset; 6: a window of the pattern's length plus some slack at
    an offset; 7: a window one byte too short for the pattern."""
    L, c = len(b), zlib.crc32(b)
    sel = c % 8
    if sel <= 2:
        return 0, INF
    if sel == 3:
        return 0, L
    if sel == 4:
        return 0, 64
    if sel == 5:
        return [1, 17, 300, 2000][(c >> 3) & 3], INF
    if sel == 6:
        off = [2, 100, 1000][(c >> 7) % 3]
        return off, off + L + [0, 7, 200][(c >> 5) % 3]
    return 10, 10 + L - 1


def unbounded(b):
    return 0, INF


def windows_by_index(d, fn=window_of):
    """(min_start, max_end) u32 arrays, one entry per pattern of a
    pm.Dictionary in its (add) order."""
    w = [fn(p) for p in d.patterns()]
    return np.array([a for a, _ in w], dtype=np.uint32), np.array([b for _, b in w], dtype=np.uint32)


def code_windows(key, fn=window_of):
    """(codes ascending, min_start, max_end, sel of each code's pattern bytes)."""
    if (key, fn) not in _cw:
        d = {(f << 24) | l: fn(b) + (window_sel(b),) for f, l, b in oracle_for(key).patterns()}
        codes = np.array(sorted(d), dtype=np.uint32)
        _cw[(key, fn)] = (codes, np.array([d[int(c)][0] for c in codes], dtype=np.int64),
                          np.array([d[int(c)][1] for c in codes], dtype=np.int64),
                          np.array([d[int(c)][2] for c in codes], dtype=np.int64))
    return _cw[(key, fn)]


def f_pos_in(F, r):
    """The bytes every flow of input F had before call r."""
    return np.array([int(p[r]) if r < len(p) else F_FLOW_BYTES for p in F.flows], dtype=np.uint64)


def _candidates(key, exp, offs, pos_in, sgroups, min_len, fn, gfn):
    """Every group-visible pattern of at least min_len bytes ending at a
    position: (positions, codes, lengths, passes its window, sel)."""
    pos, codes = expected_matches(key, exp, min_len)
    offs = np.asarray(offs, dtype=np.int64)
    j = stream_of(offs, pos)
    if sgroups is not None:
        cm_codes, cm_masks = code_masks(key, gfn)
        vis = (cm_masks[np.searchsorted(cm_codes, codes)] & np.asarray(sgroups, dtype=np.uint32)[j]) != 0
        pos, codes, j = pos[vis], codes[vis], j[vis]
    lc, ll = code_lengths(key)
    ln = ll[np.searchsorted(lc, codes)]
    wc, lo, hi, sel = code_windows(key, fn)
    k = np.searchsorted(wc, codes)
    base = np.zeros(len(offs) - 1, dtype=np.int64) if pos_in is None else np.asarray(pos_in).astype(np.int64)
    E = base[j] + pos - offs[j] + 1
    ok = (E - ln >= lo[k]) & ((hi[k] == INF) | (E <= hi[k]))
    return pos, codes, ln, ok, sel[k]


def expected_windows(key, exp, offs, pos_in, sgroups, min_len, all_matches, fn=window_of, gfn=pattern_mask):
    """(positions int64, codes u32), ascending by (position, code): of every
    pattern of at least min_len bytes ending at a position, those that pass
    their window there (E = pos_in[j] + position - offs[j] + 1 bytes of the
    stream seen; pos_in None: 0) and, with sgroups, whose mask meets the
    stream's; all_matches false: of these the longest one per position."""
    pos, codes, ln, ok, _ = _candidates(key, exp, offs, pos_in, sgroups, min_len, fn, gfn)
    pos, codes, ln = pos[ok], codes[ok], ln[ok]
    if not all_matches and len(pos):
        order = np.lexsort((-ln, pos))
        pos, codes = pos[order], codes[order]
        head = np.concatenate([[True], pos[1:] != pos[:-1]])
        pos, codes = pos[head], codes[head]
    return pos, codes


def window_stats(key, exp, offs, pos_in, min_len):
    """Without group masks: ({sel: (candidates, kept)} for sel 3..7, all
    candidates, kept events, longest-visible events whose code is not the
    dictionary's answer, positions with >= 2 kept events)."""
    exp = np.asarray(exp, dtype=np.uint32)
    pos, codes, ln, ok, sel = _candidates(key, exp, offs, pos_in, None, min_len, window_of, pattern_mask)
    per_sel = {s: (int(np.count_nonzero(sel == s)), int(np.count_nonzero(ok & (sel == s)))) for s in range(3, 8)}
    lp, lcodes = expected_windows(key, exp, offs, pos_in, None, min_len, False)
    per = np.unique(pos[ok], return_counts=True)[1]
    return (per_sel, len(pos), int(np.count_nonzero(ok)), int(np.count_nonzero(lcodes != exp[lp])),
            int(np.count_nonzero(per >= 2)))


def packet_vs_flow(key, F, min_len):
    """Over every call of input F: (kept events that counting from the
    packet's first byte would lose, dropped ones it would keep)."""
    lost = gained = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        _, _, _, ok_flow, _ = _candidates(key, exp, offs, f_pos_in(F, r), None, min_len, window_of, pattern_mask)
        _, _, _, ok_pkt, _ = _candidates(key, exp, offs, None, None, min_len, window_of, pattern_mask)
        lost += int(np.count_nonzero(ok_flow & ~ok_pkt))
        gained += int(np.count_nonzero(~ok_flow & ok_pkt))
    return lost, gained


def flows_as_streams():
    """Input F's whole text as 256 streams of 4,096 bytes."""
    return np.arange(F_FLOWS + 1, dtype=np.int64) * F_FLOW_BYTES
