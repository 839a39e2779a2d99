"""Random dictionaries and their streams (test_fuzz.py, test_fuzz_lists.py on
the GPU, test_fuzz_lists_cpu.py without one).  TEST INFRASTRUCTURE.

fuzz_case: small alphabets for deep walks and shared suffixes, pattern
suffixes and extensions for nesting, byte fans for wide trie nodes, duplicate
and rejected lines for the parser, every byte value.

Four fixed families hold what those cannot (family_case): a dictionary
without a pattern of <= 2 bytes, one with nothing else, one with more than
4,095 patterns (the coded DFA's inline answers end there), and a unary one
whose suffix chain is 48 deep, of the bytes 0x00 and 0xFF.

A case of the list tests (case()) is such a dictionary, written to a file
and registered with oracle_lib under the case's name, and two texts A and B of
49,152 bytes (48 batch tiles) over one set of stream offsets: input T's head
lengths, those around a 16-byte block and around 256 added, then random
lengths below 300.  The batched scans see A; the flow scans see A, then B
continuing every stream.  Every expected answer comes from the oracle.
"""
import atexit
import os
import shutil
import tempfile
import zlib

import numpy as np

from oracle_lib import oracle_for, register

ALPHABETS = (2, 3, 4, 16, 95, 256)


def fuzz_case(seed, stream_bytes):
    rng = np.random.default_rng(1000 + seed)
    a = ALPHABETS[seed % len(ALPHABETS)]
    alphabet = rng.choice(256, size=a, replace=False).astype(np.uint8)
    n = (30, 300, 3000)[seed % 3]
    pats = []
    for _ in range(n):
        r = rng.random()
        if pats and r < 0.2:  # a suffix of an earlier pattern (nesting)
            p = pats[rng.integers(len(pats))]
            p = p[rng.integers(0, len(p)):]
        elif pats and r < 0.35:  # an extension (deep chains)
            p = pats[rng.integers(len(pats))] + bytes(rng.choice(alphabet, 1 + rng.geometric(0.3)))
        else:
            p = bytes(rng.choice(alphabet, min(1 + rng.geometric(0.12), 200)))
        pats.append(p[:200])
    if a >= 16:  # a wide reversed-trie node: many bytes before one suffix
        tail = bytes(rng.choice(alphabet, 3))
        pats += [bytes([c]) + tail for c in alphabet[:40]]
    lines = [b"|" + b" ".join(b"%02x" % c for c in p) + b"|" for p in pats if p]
    # the parser's rejections and skips (parser.c:63-99): they only shift line numbers
    for bad in (b"|41 |", b"|4|", b"|41", b""):
        lines.insert(int(rng.integers(len(lines) + 1)), bad)
    # the stream: runs of alphabet bytes and copies of patterns
    parts, size = [], 0
    while size < stream_bytes:
        if rng.random() < 0.5:
            q = pats[rng.integers(len(pats))]
        else:
            q = bytes(rng.choice(alphabet, int(rng.integers(1, 64))))
        parts.append(q)
        size += len(q)
    text = np.frombuffer(b"".join(parts)[:stream_bytes], np.uint8).copy()
    return b"\n".join(lines) + b"\n", text


def write_dict(tmp_path, seed, data):
    path = os.path.join(str(tmp_path), f"fuzz{seed}.dict")
    with open(path, "wb") as f:
        f.write(data)
    return path


# ---- the four families ---------------------------------------------------------
FAMILIES = ("no_short", "only_short", "many", "unary")
UNARY_X, UNARY_Y, UNARY_DEPTH = 0x00, 0xFF, 48


def _family_patterns(name, rng):
    """(patterns, alphabet, the weight of each alphabet byte in a run)."""
    if name == "no_short":  # about 200 patterns of >= 3 bytes over 3 symbols
        alphabet = rng.choice(256, size=3, replace=False).astype(np.uint8)
        pats = []
        for _ in range(200):
            r = rng.random()
            if pats and r < 0.2:
                p = pats[rng.integers(len(pats))]
                p = p[rng.integers(0, len(p) - 2):]
            elif pats and r < 0.35:
                p = pats[rng.integers(len(pats))] + bytes(rng.choice(alphabet, 1 + rng.geometric(0.3)))
            else:
                p = bytes(rng.choice(alphabet, 2 + rng.geometric(0.25)))
            pats.append(p[:200])
        assert min(map(len, pats)) >= 3
        return pats, alphabet, None
    if name == "only_short":  # 4 one-byte and 30 two-byte patterns over 6 symbols
        alphabet = rng.choice(256, size=6, replace=False).astype(np.uint8)
        pats = [bytes([c]) for c in alphabet[:4]]
        pairs = rng.permutation(36)[:30]
        pats += [bytes([alphabet[k // 6], alphabet[k % 6]]) for k in pairs.tolist()]
        return pats, alphabet, None
    if name == "many":  # 9,000 draws of geometric length over 8 symbols
        alphabet = rng.choice(256, size=8, replace=False).astype(np.uint8)
        return [bytes(rng.choice(alphabet, min(int(rng.geometric(0.12)), 200))) for _ in range(9000)], alphabet, None
    assert name == "unary"  # x^k for k = 1..48 and x^k y for five k: a chain member at every depth
    x, y = bytes([UNARY_X]), bytes([UNARY_Y])
    pats = [x * k for k in range(1, UNARY_DEPTH + 1)] + [x * k + y for k in (0, 1, 2, 5, 47)]
    return pats, np.array([UNARY_X, UNARY_Y], np.uint8), np.array([7, 1]) / 8


def family_case(name, stream_bytes):
    """(dictionary file's bytes, text) of a family, seeded from its name; the
    stream is fuzz_case's: half copies of patterns, half runs of alphabet bytes."""
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pats, alphabet, weight = _family_patterns(name, rng)
    lines = [b"|" + b" ".join(b"%02x" % c for c in p) + b"|" for p in pats]
    parts, size = [], 0
    while size < stream_bytes:
        if rng.random() < 0.5:
            q = pats[rng.integers(len(pats))]
        else:
            q = bytes(rng.choice(alphabet, int(rng.integers(1, 64)), p=weight))
        parts.append(q)
        size += len(q)
    text = np.frombuffer(b"".join(parts)[:stream_bytes], np.uint8).copy()
    return b"\n".join(lines) + b"\n", text


# ---- the cases of the list tests -------------------------------------------------
N = 49152  # 48 batch tiles
SEEDS = tuple(range(18))  # three per alphabet
CASES = FAMILIES + tuple(f"seed{s}" for s in SEEDS)
# the GPU file's: one seed per alphabet (with all 18 it took longer than test_fuzz.py's GPU test;
# the CPU file runs the host path on all of them)
GPU_CASES = FAMILIES + tuple(f"seed{s}" for s in range(len(ALPHABETS)))
HEAD_LENGTHS = [0, 1, 2, 3, 4, 0, 0, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4097]

_dir = []
_cases = {}


def _tmp_dir():
    if not _dir:
        _dir.append(tempfile.mkdtemp(prefix="pm-fuzz-"))
        atexit.register(shutil.rmtree, _dir[0], ignore_errors=True)
    return _dir[0]


def offsets(n=N):
    """batch_inputs.t_offsets with the lengths around 16 and 256 in its head."""
    lengths = list(HEAD_LENGTHS)
    total = sum(lengths)
    rng = np.random.default_rng(11)
    while total < n:
        k = int(rng.integers(0, 300))
        lengths.append(k)
        total += k
    offs = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=offs[1:])
    return np.minimum(offs, n)


def oracle_two_calls(key, A, B, offs):
    """The codes of A_j + B_j per stream j, split back into A's and B's."""
    o = oracle_for(key)
    ea, eb = np.zeros(len(A), np.uint32), np.zeros(len(B), np.uint32)
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        if b > a:
            o.reset()
            both = o.scan_codes(np.concatenate([A[a:b], B[a:b]]))
            ea[a:b], eb[a:b] = both[:b - a], both[b - a:]
    o.reset()
    return ea, eb


def plant_straddlers(A, B, offs, pats, rng):
    """A pattern of 10..64 bytes across every stream boundary of A that has
    room for it, at least 9 of its bytes behind the boundary, and those bytes
    also at the head of the stream of B that continues the stream before the
    boundary.  A scan that ignores a boundary of A, and a flow scan of B
    that starts a stream afresh, then answer wrongly well inside a stream:
    random streams alone leave a handful of such positions (patterns are
    short, boundaries 150 bytes apart).  Returns the number planted."""
    long_pats = sorted({p for p in pats if 10 <= len(p) <= 64})
    if not long_pats:
        return 0
    planted, head = 0, 0  # head: bytes at the start of stream j - 1 that a plant owns
    for j in range(1, len(offs) - 1):
        lo, a, b = int(offs[j - 1]), int(offs[j]), int(offs[j + 1])
        p = long_pats[int(rng.integers(len(long_pats)))]
        k = int(rng.integers(1, len(p) - 8))  # bytes before the boundary
        after = len(p) - k
        if a - lo - head >= k and a - lo >= after and b - a >= after:
            q = np.frombuffer(p, np.uint8)
            A[a - k:a + after] = q
            B[lo:lo + after] = q[k:]
            planted, head = planted + 1, after
        else:
            head = 0
    return planted


class Case:
    """key: the name, registered with oracle_lib; path: the dictionary file;
    A, B: the two texts; offs: the stream offsets; ea, eb: the oracle's codes
    of A and of B, stream j of B continuing stream j of A (ea is also the
    batched scan's answer: every stream of A from its own first byte)."""

    def __init__(self, name):
        self.key = name
        if name in FAMILIES:
            data, text = family_case(name, 2 * N)
        else:
            data, text = fuzz_case(int(name[4:]), 2 * N)
        self.path = write_dict(_tmp_dir(), "-" + name, data)
        register(name, [self.path])
        self.A, self.B = text[:N].copy(), text[N:].copy()
        self.offs = offsets()
        self.nseg = len(self.offs) - 1
        self.planted = plant_straddlers(self.A, self.B, self.offs, [b for _, _, b in oracle_for(name).patterns()],
                                        np.random.default_rng(zlib.crc32(name.encode()) + 1))
        self.ea, self.eb = oracle_two_calls(name, self.A, self.B, self.offs)
        for a in (self.A, self.B, self.offs, self.ea, self.eb):
            a.setflags(write=False)


def case(name):
    """The case of a name of CASES; cached, callers do not modify it."""
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


def stream_starts(offs, n):
    """The first position of the stream that holds each of n positions."""
    offs = np.asarray(offs, dtype=np.int64)
    return offs[np.searchsorted(offs, np.arange(n), side="right") - 1]
