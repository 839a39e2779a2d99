"""Expected all-matches lists of the matches tests (test_matches.py on the GPU,
test_matches_cpu.py without one), derived from the oracle alone.  TEST
INFRASTRUCTURE.

For expected codes exp over a buffer the list holds, for every i with exp[i]
!= 0, every pattern of the oracle's own pattern list whose bytes are a suffix
of exp[i]'s pattern, itself included, and whose length is at least min_len.
The suffixes are found by byte-string lookup over the oracle's patterns; the
library's parent[] plays no part.
"""
import numpy as np

from oracle_lib import oracle_for

_chains = {}


def suffix_chains(key):
    """code -> (codes, lengths) of the patterns that are suffixes of the
    code's pattern, itself first, by falling length.  Two patterns with the
    same bytes are one byte string: the lookup gives the code the oracle
    answers with (the later one; asserted in test_matches_cpu.py)."""
    if key not in _chains:
        pats = oracle_for(key).patterns()
        by_bytes = {b: (f << 24) | l for f, l, b in pats}
        chains = {}
        for b, code in by_bytes.items():
            hits = [(by_bytes[b[k:]], len(b) - k) for k in range(len(b)) if b[k:] in by_bytes]
            assert hits[0] == (code, len(b))
            chains[code] = (np.array([h[0] for h in hits], dtype=np.uint32),
                            np.array([h[1] for h in hits], dtype=np.int64))
        _chains[key] = (chains, by_bytes)
    return _chains[key][0]


def deepest_pattern(key):
    """The bytes of the pattern with the most suffix patterns (the longest
    such pattern among equals) and that count."""
    chains = suffix_chains(key)
    by_bytes = _chains[key][1]
    b = max(by_bytes, key=lambda b: (len(chains[by_bytes[b]][0]), len(b), b))
    return b, len(chains[by_bytes[b]][0])


def expected_matches(key, exp, min_len):
    """(positions int64, codes u32) of the expected list, ascending by
    (position, code)."""
    chains = suffix_chains(key)
    exp = np.asarray(exp, dtype=np.uint32)
    nz = np.nonzero(exp)[0]
    uniq, inv = np.unique(exp[nz], return_inverse=True)
    kept = [chains[int(c)][0][chains[int(c)][1] >= max(min_len, 1)] for c in uniq]
    count = np.array([len(k) for k in kept], dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(count)])[:-1]
    flat = np.concatenate(kept) if kept else np.zeros(0, np.uint32)
    per = count[inv]
    pos = np.repeat(nz.astype(np.int64), per)
    # index into flat: the chain's start + 0 .. per - 1
    first = np.repeat(np.cumsum(per) - per, per)
    codes = flat[np.repeat(start[inv], per) + (np.arange(len(pos)) - first)]
    order = np.lexsort((codes, pos))
    return pos[order], codes[order]


def sort_matches(pos, codes):
    """A (positions, codes) list in expected_matches' order."""
    pos, codes = np.asarray(pos, dtype=np.int64), np.asarray(codes, dtype=np.uint32)
    order = np.lexsort((codes, pos))
    return pos[order], codes[order]


def longest_per_position(key, pos, codes):
    """The list reduced to the longest pattern of every position."""
    from event_inputs import code_lengths
    all_codes, lens = code_lengths(key)
    ln = lens[np.searchsorted(all_codes, codes)]
    order = np.lexsort((-ln, pos))
    pos, codes = pos[order], codes[order]
    head = np.concatenate([[True], pos[1:] != pos[:-1]]) if len(pos) else np.zeros(0, bool)
    return pos[head], codes[head]


def match_stats(key, exp, min_len):
    """(heads, all events, positions with >= 3 events, most events at one position)."""
    from event_inputs import expected_events
    pos, _ = expected_matches(key, exp, min_len)
    heads = len(expected_events(key, exp, min_len)[0])
    per = np.unique(pos, return_counts=True)[1]
    return heads, len(pos), int(np.count_nonzero(per >= 3)), int(per.max()) if len(per) else 0
