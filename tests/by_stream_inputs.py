"""References, expected answers and hand-made lists of the per-stream-sets
tests (test_by_stream.py and test_fuzz_by_stream.py on the GPU,
test_by_stream_cpu.py and test_fuzz_by_stream_cpu.py without one).  TEST
INFRASTRUCTURE; no device, nothing here calls the library.

reference() is the dozen lines of numpy that pin the host twin
(pm_flat_events_by_stream).  grouped_from_list() goes from an oracle-derived
(positions, codes) list straight to the grouped answer, through neither the
twin nor the library's list.  scan_like(), scattered() and distinct_keys()
make lists of any length over given stream offsets.
"""
import numpy as np

GID_BITS = 24
GID_MAX = (1 << GID_BITS) - 1


def pack(pos, gid):
    return (np.asarray(pos, dtype=np.uint64) << np.uint64(GID_BITS)) | np.asarray(gid, dtype=np.uint64)


def reference(events, offsets, unique):
    """(stream_ptr, events): each stream's range ascending.  The stream of a
    position is the first offset above it, minus one; UNIQUE keeps the
    smallest position of each (stream, gid)."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    pos = (events >> np.uint64(GID_BITS)).astype(np.int64)
    j = np.searchsorted(offs, pos, side="right") - 1
    keep = (j >= 0) & (j < nseg)
    j, ev = j[keep], events[keep]
    if unique:
        first = {}
        for s, e in zip(j.tolist(), ev.tolist()):
            k = (s, e & GID_MAX)
            first[k] = min(first.get(k, e), e)  # equal gid: the smaller event is the smaller position
        j = np.array([k[0] for k in first], dtype=np.int64)
        ev = np.array(list(first.values()), dtype=np.uint64)
    order = np.lexsort((ev, j))
    ptr = np.searchsorted(j[order], np.arange(nseg + 1), side="left").astype(np.int64)
    return ptr, ev[order]


def list_keys(pos, codes):
    """(position, code) pairs as u64 keys, position << 32 | code."""
    return (np.asarray(pos).astype(np.uint64) << np.uint64(32)) | np.asarray(codes).astype(np.uint64)


def grouped_from_list(pos, codes, offs, unique):
    """The expected (stream_ptr, keys) of a by-stream call on a list whose
    events are the (positions, codes) pairs given, in any order: keys are
    position << 32 | code, each stream's range ascending; unique keeps the
    smallest position of every (stream, code).  Sorting only: no hash, no
    dict, none of the library."""
    pos = np.asarray(pos, dtype=np.int64)
    codes = np.asarray(codes).astype(np.int64)
    offs = np.asarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    j = np.searchsorted(offs, pos, side="right") - 1  # empty streams own nothing: the last of equal offsets wins
    keep = (j >= 0) & (pos < offs[-1])
    pos, codes, j = pos[keep], codes[keep], j[keep]
    if unique and len(pos):
        order = np.lexsort((pos, codes, j))
        pos, codes, j = pos[order], codes[order], j[order]
        first = np.concatenate([[True], (j[1:] != j[:-1]) | (codes[1:] != codes[:-1])])
        pos, codes, j = pos[first], codes[first], j[first]
    order = np.lexsort((codes, pos, j))
    ptr = np.searchsorted(j[order], np.arange(nseg + 1), side="left").astype(np.int64)
    return ptr, list_keys(pos[order], codes[order])


def first_difference(ptr, exp_ptr):
    """A message naming the first stream whose count differs, '' when none does."""
    got, want = np.diff(np.asarray(ptr)), np.diff(np.asarray(exp_ptr))
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return ""
    j = int(bad[0])
    return f"{bad.size} streams differ, the first is stream {j}: {int(want[j])} events expected, {int(got[j])} observed"


def first_range_difference(ptr, got, want):
    """got and want: the kept events under one stream_ptr, each range sorted.
    A message naming the first stream whose range differs, '' when none does."""
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    if bad.size == 0:
        return ""
    j = int(np.searchsorted(ptr, bad[0], side="right")) - 1
    n = int(ptr[j + 1] - ptr[j])
    wrong = int(np.count_nonzero((bad >= ptr[j]) & (bad < ptr[j + 1])))
    return (f"{bad.size} kept events differ, the first in stream {j}: {n} events expected and observed there, "
            f"{wrong} of them differ (expected {int(want[bad[0]]):#x}, observed {int(got[bad[0]]):#x})")


# ---- hand-made lists ---------------------------------------------------------------
def mixed_offsets(rng, long_stream=100000, groups=40):
    """Stream offsets that mix lengths 0, 1, about 1,500 and one stream of
    about long_stream positions (in the middle), from a base that is not 0."""
    lens = []
    for g in range(groups):
        lens += [0, 1, 0, 0, 1, 1, int(rng.integers(1400, 1600)), 1, 0]
        if g == groups // 2:
            lens.append(long_stream + int(rng.integers(0, 100)))
    return 1000 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def scattered(n, offs, gids, rng):
    """n events, positions uniform from a few below offsets[0] to a few past
    offsets[-1], gids drawn from `gids`."""
    offs = np.asarray(offs, dtype=np.int64)
    pos = rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n)
    return pack(pos, rng.choice(np.asarray(gids), size=n))


def scan_like(n, offs, gids, rng):
    """scattered() in the order a scan appends: positions ascending, then
    shuffled inside consecutive windows of 64 to 4,096 events, like the
    wave-sized flushes of neighbouring tiles."""
    ev = scattered(n, offs, gids, rng)
    ev = ev[np.argsort(ev >> np.uint64(GID_BITS), kind="stable")]
    at = 0
    while at < n:
        w = int(rng.integers(64, 4097))
        rng.shuffle(ev[at:at + w])
        at += w
    return ev


def distinct_keys(n, offs, rng):
    """n events, every (stream, gid) once, in random order: the non-empty
    streams in turn, gid 1 + (k // streams) for the k-th event, a random
    position of its stream.  With n a power of two UNIQUE's table (2 n slots)
    is exactly half full."""
    offs = np.asarray(offs, dtype=np.int64)
    full = np.nonzero(np.diff(offs) > 0)[0]
    k = np.arange(n)
    j = full[k % len(full)]
    gid = 1 + k // len(full)
    assert int(gid.max()) <= GID_MAX
    pos = offs[j] + rng.integers(0, 1 << 62, size=n) % (offs[j + 1] - offs[j])
    ev = pack(pos, gid)
    rng.shuffle(ev)
    return ev
