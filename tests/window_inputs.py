"""Window tables and expected lists of the pattern-window tests
(test_windows.py on the GPU, test_windows_cpu.py without one).  TEST
INFRASTRUCTURE.

A pattern's window is a fixed function of its bytes (window_of); the expected
lists come from the oracle's answers, the suffixes found by byte-string lookup
over the oracle's patterns (match_inputs.expected_matches), the oracle's
pattern lengths, group_inputs' masks and this table.  The library's parent /
reach / window tables play no part.

The fuzz cases (test_fuzz_windows.py, test_fuzz_windows_cpu.py) have two
tables of their own: fuzz_window_of, window_of scaled to their short streams,
and far_window_of with far_pos_in for flows whose byte count passes 2^32.
Positions stay at or below 2^62 plus a stream's length, so E is exact in
int64, and max_end == INF is the only "unbounded".
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
_am = {}


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


def fuzz_window_of(b):
    """window_of scaled to the streams of fuzz_inputs (most below 300 bytes,
    the head lengths up to 4,097).  sel 0-2: unbounded; 3: anchored at the
    stream's start; 4: within the first 24 bytes; 5: not before an offset below
    64; 6: a window of the pattern's length plus some slack at an offset below
    150; 7: a window one byte too short for the pattern."""
    L, c = len(b), zlib.crc32(b)
    sel = c % 8
    if sel <= 2:
        return 0, INF
    if sel == 3:
        return 0, L
    if sel == 4:
        return 0, 24
    if sel == 5:
        return [1, 5, 17, 40][(c >> 3) & 3], INF
    if sel == 6:
        off = [2, 30, 120][(c >> 7) % 3]
        return off, off + L + [0, 7, 60][(c >> 5) % 3]
    return 10, 10 + L - 1


FAR_START = 0x7FFFFFFF  # the largest min_start pm_hip_set_windows takes


def far_window_of(b):
    """Windows for flows around 2^32 bytes (far_pos_in).  sel 0-2: unbounded;
    3: the largest bounded end; 4: the largest start; 5: both; 6: within the
    first 64 bytes; 7: a window across 2^31."""
    sel = zlib.crc32(b) % 8
    if sel <= 2:
        return 0, INF
    return [(0, INF - 1), (FAR_START, INF), (FAR_START, INF - 1), (0, 64), (0x7FFFFFF0, 0x80000040)][sel - 3]


def far_pos_in(offs):
    """The bytes every stream had before the call: 2^32 - d for stream j, d
    cycling over len + 1, len, len // 2, 17, 16, 1, 0, -1 and -4096 (len the
    stream's length), so that the stream's count passes 0xFFFFFFFF at its last
    byte, one before it, in mid-stream and inside a 16-byte block, or begins on
    or past it; and, in the same cycle, the fixed positions 2^40 and 2^62."""
    lens = np.diff(np.asarray(offs, dtype=np.int64)).tolist()
    out = []
    for j, n in enumerate(lens):
        r = j % 11
        if r >= 9:
            out.append(1 << (40 if r == 9 else 62))
        else:
            out.append((1 << 32) - [n + 1, n, n // 2, 17, 16, 1, 0, -1, -4096][r])
    return np.array(out, dtype=np.uint64)


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


def _all_matches(key, exp, offs, min_len):
    """expected_matches with, per event, its stream, its pattern's length and
    its code's index in the per-code tables (code_lengths, code_masks and
    code_windows list the same codes, ascending).  The last few answers are
    kept: a test asks for the same list under several masks, forms and
    positions in turn."""
    ck = (key, min_len, len(exp), zlib.crc32(exp.tobytes()), zlib.crc32(offs.tobytes()))
    if ck not in _am:
        pos, codes = expected_matches(key, exp, min_len)
        lc, ll = code_lengths(key)
        assert np.array_equal(lc, code_masks(key)[0])
        k = np.searchsorted(lc, codes)
        while len(_am) >= 4:
            _am.pop(next(iter(_am)))
        _am[ck] = (pos, codes, stream_of(offs, pos), ll[k], k)
    return _am[ck]


def _candidates(key, exp, offs, pos_in, sgroups, min_len, fn, gfn):
    """Every group-visible pattern of at least min_len bytes ending at a
    position: (positions, codes, lengths, passes its window, sel)."""
    return _candidates_e(key, exp, offs, pos_in, sgroups, min_len, fn, gfn)[:5]


def _candidates_e(key, exp, offs, pos_in, sgroups, min_len, fn, gfn):
    """_candidates and E, the bytes the stream has had through the position
    (int64: exact while pos_in stays at or below 2^62)."""
    offs = np.asarray(offs, dtype=np.int64)
    pos, codes, j, ln, k = _all_matches(key, np.asarray(exp, dtype=np.uint32), offs, min_len)
    if sgroups is not None:
        cm_codes, cm_masks = code_masks(key, gfn)
        vis = (cm_masks[k] & np.asarray(sgroups, dtype=np.uint32)[j]) != 0
        pos, codes, j, ln, k = pos[vis], codes[vis], j[vis], ln[vis], k[vis]
    wc, lo, hi, sel = code_windows(key, fn)
    base = np.zeros(len(offs) - 1, dtype=np.int64) if pos_in is None else np.asarray(pos_in).astype(np.int64)
    E = base[j] + pos - offs[j] + 1
    ok = (E - ln >= lo[k]) & ((hi[k] == INF) | (E <= hi[k]))
    return pos, codes, ln, ok, sel[k], E


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


def window_stats(key, exp, offs, pos_in, min_len, fn=window_of):
    """Without group masks: ({sel: (candidates, kept)} for sel 3..7, all
    candidates, kept events, longest-visible events whose code is not the
    dictionary's answer, positions with >= 2 kept events)."""
    exp = np.asarray(exp, dtype=np.uint32)
    pos, codes, ln, ok, sel = _candidates(key, exp, offs, pos_in, None, min_len, fn, pattern_mask)
    per_sel = {s: (int(np.count_nonzero(sel == s)), int(np.count_nonzero(ok & (sel == s)))) for s in range(3, 8)}
    lp, lcodes = expected_windows(key, exp, offs, pos_in, None, min_len, False, fn)
    per = np.unique(pos[ok], return_counts=True)[1]
    return (per_sel, len(pos), int(np.count_nonzero(ok)), int(np.count_nonzero(lcodes != exp[lp])),
            int(np.count_nonzero(per >= 2)))


def chain_stats(key, exp, offs, pos_in, depth, fn=window_of):
    """Of the all-matches list at min_len 1 without group masks: (positions
    where the depth-th or a deeper member of the position's suffix chain, the
    head being the first, is kept while a shallower one is dropped, positions
    where such a member is dropped while a shallower one is kept, positions
    with a candidate)."""
    pos, codes, ln, ok, _ = _candidates(key, exp, offs, pos_in, None, 1, fn, pattern_mask)
    order = np.lexsort((-ln, pos))
    pos, ok = pos[order], ok[order]
    first = np.nonzero(np.concatenate([[True], pos[1:] != pos[:-1]]))[0]
    size = np.diff(np.concatenate([first, [len(pos)]]))
    rank = np.arange(len(pos)) - np.repeat(first, size) + 1  # 1: the head
    big = len(pos) + 1
    deep_kept = np.maximum.reduceat(np.where(ok, rank, 0), first)
    deep_dropped = np.maximum.reduceat(np.where(ok, 0, rank), first)
    first_kept = np.minimum.reduceat(np.where(ok, rank, big), first)
    first_dropped = np.minimum.reduceat(np.where(ok, big, rank), first)
    return (int(np.count_nonzero((deep_kept >= depth) & (first_dropped < deep_kept))),
            int(np.count_nonzero((deep_dropped >= depth) & (first_kept < deep_dropped))), len(first))


def far_stats(key, exp, offs, pos_in, min_len, fn=far_window_of):
    """Without group masks: {sel: (candidates whose E is below 0xFFFFFFFF,
    equal to it, above it, kept ones)} for sel 3..7."""
    _, _, _, ok, sel, E = _candidates_e(key, exp, offs, pos_in, None, min_len, fn, pattern_mask)
    return {s: (int(np.count_nonzero((sel == s) & (E < INF))), int(np.count_nonzero((sel == s) & (E == INF))),
                int(np.count_nonzero((sel == s) & (E > INF))), int(np.count_nonzero((sel == s) & ok)))
            for s in range(3, 8)}


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
