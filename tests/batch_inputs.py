"""Inputs and oracle answers of the batched-scan tests (test_batch.py on the
GPU, test_batch_cpu.py without one).  TEST INFRASTRUCTURE.

Input T: 64 KiB of dictionary patterns drawn at random, each followed by a
newline, cut into 385 streams whose lengths cover 0 (also in a run), 1..5,
the wave (63/64/65), tile (1023/1024/1025) and multi-tile (4095/4097) edges,
then random lengths below 300.  Dense deep matches make the segmented answers
differ from the unsegmented ones at hundreds of positions, many of them well
inside their stream, so a scan that ignores the boundaries -- or honours them
only for the depth <= 2 lookups -- cannot pass.
"""
import numpy as np

from oracle_lib import oracle_for

T_BYTES = 65536
T_HEAD_LENGTHS = [0, 1, 2, 3, 4, 0, 0, 5, 63, 64, 65, 1023, 1024, 1025, 4095, 4097]

_cache = {}


def t_text(key):
    pats = [p[2] for p in oracle_for(key).patterns()]
    rng = np.random.default_rng(5)
    parts, total = [], 0
    while total < T_BYTES:
        p = pats[rng.integers(0, len(pats))] + b"\n"
        parts.append(p)
        total += len(p)
    return np.frombuffer(b"".join(parts)[:T_BYTES], dtype=np.uint8).copy()


def t_offsets(n=T_BYTES):
    lengths = list(T_HEAD_LENGTHS)
    total = sum(lengths)
    rng = np.random.default_rng(11)
    while total < n:
        k = int(rng.integers(0, 300))
        lengths.append(k)
        total += k
    offs = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    return np.minimum(offs, n)


def oracle_per_stream(key, text, offs):
    """Codes of text scanned stream by stream: reset() before each stream."""
    o = oracle_for(key)
    out = np.zeros(len(text), dtype=np.uint32)
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        if b > a:
            o.reset()
            out[a:b] = o.scan_codes(text[a:b])
    o.reset()
    return out


def input_t(key):
    """(text, offsets, expected codes) of input T for a dictionary; cached,
    callers do not modify them."""
    if key not in _cache:
        text, offs = t_text(key), t_offsets()
        exp = oracle_per_stream(key, text, offs)
        for a in (text, offs, exp):
            a.setflags(write=False)
        _cache[key] = (text, offs, exp)
    return _cache[key]


def precondition(key):
    """(positions whose segmented answer differs from the unsegmented one,
    those of them 8 or more bytes past their stream's start)."""
    text, offs, exp = input_t(key)
    o = oracle_for(key)
    o.reset()
    whole = o.scan_codes(text)
    o.reset()
    diff = np.nonzero(whole != exp)[0]
    start = offs[np.searchsorted(offs, diff, side="right") - 1]
    return int(diff.size), int(np.count_nonzero(diff - start >= 8))
