"""Dictionaries, texts and the brute-force oracle of the nocase tests
(test_nocase.py on the GPU, test_nocase_cpu.py without one).  TEST
INFRASTRUCTURE.

Nothing here reads the library's tables.  brute() finds every occurrence of
every folded pattern in the folded text with bytes.find, keeps a
case-sensitive pattern iff the real bytes are equal, and applies min_len,
groups, windows and the longest / smallest-gid rule itself.  A flow is
searched as one text (all its packets joined), so a pattern that straddles a
packet boundary is simply found; call_events() cuts the answer per call.
"""
import zlib

import numpy as np

INF = 0xFFFFFFFF
_FOLD = bytes(c + 32 if 65 <= c <= 90 else c for c in range(256))
_SWAP = bytes(c + 32 if 65 <= c <= 90 else c - 32 if 97 <= c <= 122 else c for c in range(256))

# letters of both cases, the four neighbours of the letter ranges, two bytes >= 0x80 that differ
# by 0x20 (no case pair), a digit
ALPHABET = np.frombuffer(b"aAbBcCxX@[`{\xc1\xe11", np.uint8)

HAND = [(b"GET", 0), (b"get", 1), (b"Get", 0), (b"/Admin", 0), (b"admin", 1), (b"@[", 0), (b"\xc1b", 1)]
HAND_TEXTS = [b"GET get gEt /admin /Admin", b"`{ @[ `[", b"\xe1B \xc1B \xc1b \xe1b"]


def fold(b):
    return bytes(b).translate(_FOLD)


def flag_of(p):
    return zlib.crc32(p) & 1


def flip_case(text):
    """The case of about a quarter of the letters flipped, by a hash of the position."""
    t = np.array(text, dtype=np.uint8, copy=True)
    pos = np.arange(len(t), dtype=np.uint64)
    pick = ((pos * np.uint64(2654435761)) >> np.uint64(7)) & np.uint64(3) == 0
    sw = np.frombuffer(_SWAP, np.uint8)
    t[pick] = sw[t[pick]]
    return t


def fuzz_dictionary(seed, n=250, long_cs=True):
    """Patterns over ALPHABET: random strings, suffixes and extensions of earlier
    ones (nesting), case variants of earlier ones (classes of several members),
    one exact duplicate, and a case-sensitive pattern of 150 bytes (history word
    index 2)."""
    rng = np.random.default_rng(4000 + seed)
    pats = []
    for _ in range(n):
        r = rng.random()
        if pats and r < 0.2:
            p = pats[rng.integers(len(pats))]
            p = p[rng.integers(0, len(p)):]
        elif pats and r < 0.35:
            p = pats[rng.integers(len(pats))] + bytes(rng.choice(ALPHABET, 1 + rng.geometric(0.3)))
        elif pats and r < 0.55:
            q = np.frombuffer(pats[rng.integers(len(pats))], np.uint8).copy()
            m = rng.random(len(q)) < 0.5
            q[m] = np.frombuffer(_SWAP, np.uint8)[q[m]]
            p = q.tobytes()
        else:
            p = bytes(rng.choice(ALPHABET, min(1 + rng.geometric(0.2), 60)))
        pats.append(p[:60])
    pats.append(pats[3])  # a byte string added twice: the later add wins
    if long_cs:
        p = bytes(rng.choice(ALPHABET[:8], 150))
        while flag_of(p):
            p = p[:-1] + bytes([ALPHABET[rng.integers(8)]])
        pats.append(p)
    return pats


def fuzz_text(pats, seed, nbytes):
    rng = np.random.default_rng(5000 + seed)
    parts, size = [], 0
    while size < nbytes:
        if rng.random() < 0.5:
            q = pats[rng.integers(len(pats))]
        else:
            q = bytes(rng.choice(ALPHABET, int(rng.integers(1, 40))))
        parts.append(q)
        size += len(q)
    return flip_case(np.frombuffer(b"".join(parts)[:nbytes], np.uint8))


def family_dictionary(name):
    """A family of fuzz_inputs (no_short, only_short, many, unary) with its alphabet
    re-drawn from ALPHABET: symbol k becomes ALPHABET[k], so neighbours are a case
    pair and patterns fall into classes (unary: a^k and a^k A)."""
    from fuzz_inputs import _family_patterns
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    pats, alphabet, _ = _family_patterns(name, rng)
    table = bytearray(range(256))
    for k, c in enumerate(alphabet.tolist()):
        table[c] = int(ALPHABET[k % len(ALPHABET)])
    return [p.translate(bytes(table)) for p in pats]


def real_dictionary(key="et"):
    """The patterns of a shipped dictionary in add order."""
    import patternmatching_amd as pm
    from oracle_lib import dict_paths
    return pm.Dictionary(dict_paths(key)).patterns()


def input_t_flipped(key="et"):
    """Input T's text and offsets, the case of its letters flipped by position."""
    from batch_inputs import t_offsets, t_text
    return flip_case(t_text(key)), t_offsets()


def input_f_flipped(key="et"):
    """Input F: (text of 256 flows of 4,096 bytes, case flipped; per flow its packet
    offsets; the number of calls)."""
    from flow_inputs import f_packets, f_text
    flows = f_packets()
    return flip_case(f_text(key)), flows, max(len(p) - 1 for p in flows)


def f_call(text, flows, r):
    """Call r of input F: (data, offsets, the bytes every flow had before it)."""
    from flow_inputs import F_FLOW_BYTES
    spans, before = [], []
    for f, p in enumerate(flows):
        a, b = (int(p[r]), int(p[r + 1])) if r + 1 < len(p) else (F_FLOW_BYTES, F_FLOW_BYTES)
        spans.append((f * F_FLOW_BYTES + a, f * F_FLOW_BYTES + b))
        before.append(a)
    data = np.concatenate([text[a:b] for a, b in spans] + [np.zeros(0, np.uint8)])
    offs = np.concatenate([[0], np.cumsum([b - a for a, b in spans])]).astype(np.int64)
    return data, offs, np.array(before, dtype=np.int64)


def stream_offsets(n, seed):
    """nseg + 1 offsets over n bytes: empty streams, lengths around a 16-byte block and
    around 256, a 1,500-byte one, then random lengths below 300."""
    rng = np.random.default_rng(6000 + seed)
    lens = [0, 1, 2, 15, 16, 17, 0, 255, 256, 257, 1500, 31, 33]
    while sum(lens) < n:
        lens.append(int(rng.integers(0, 300)))
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    offs = offs[offs < n]
    return np.concatenate([offs, [n]]).astype(np.int64)


def group_of(p):
    return 1 << ((zlib.crc32(p) >> 3) % 3)


def stream_groups(nseg):
    return np.array([(1, 2, 4, 3, 7, 5)[j % 6] for j in range(nseg)], dtype=np.uint32)


def window_of(p):
    c = zlib.crc32(p)
    sel = (c >> 5) % 4
    if sel <= 1:
        return 0, INF
    if sel == 2:
        return 0, 64
    return 5, INF


def winners(pats):
    """{bytes: index of the add that wins (the last one)}."""
    return {p: k for k, p in enumerate(pats)}


def brute(pats, flags, streams, gid_of_index, min_len=1, groups=None, sgroups=None, windows=None, all_matches=True,
          base=None):
    """Events of whole streams: an int64 array of rows (stream, position, gid,
    start of the match), sorted by (stream, position, gid), and a dict of counts
    {"nocase_case_differs", "rejected"}.  flags / groups / windows are per
    pattern index; windows = (min_start, max_end) arrays.  base[j]: the bytes
    stream j had before its position 0 (the windows count them; Python ints)."""
    rows = []
    stats = {"nocase_case_differs": 0, "rejected": 0}
    win = winners(pats)
    for j, t in enumerate(streams):
        t = bytes(t)
        ft = fold(t)
        for p, k in win.items():
            L = len(p)
            if L < min_len:
                continue
            if groups is not None and sgroups is not None and not (int(groups[k]) & int(sgroups[j])):
                continue
            fp = fold(p)
            s = ft.find(fp)
            while s >= 0:
                e = s + L - 1
                raw = t[s:s + L]
                ok = True
                if flags[k]:
                    stats["nocase_case_differs"] += raw != p
                elif raw != p:
                    ok = False
                    stats["rejected"] += 1
                if ok and windows is not None:
                    E = (0 if base is None else int(base[j])) + e + 1
                    lo, hi = int(windows[0][k]), int(windows[1][k])
                    ok = E - L >= lo and (hi == INF or E <= hi)
                if ok:
                    rows.append((j, e, int(gid_of_index[k]), s, L))
                s = ft.find(fp, s + 1)
    if not rows:
        return np.zeros((0, 4), np.int64), stats
    a = np.array(rows, dtype=np.int64)
    if not all_matches:
        order = np.lexsort((a[:, 2], -a[:, 4], a[:, 1], a[:, 0]))
        a = a[order]
        first = np.concatenate([[True], (a[1:, 0] != a[:-1, 0]) | (a[1:, 1] != a[:-1, 1])])
        a = a[first]
    order = np.lexsort((a[:, 2], a[:, 1], a[:, 0]))
    return a[order][:, :4], stats


def batch_events(rows, offs):
    """Rows of brute() over the streams of one batched buffer -> u64 events."""
    offs = np.asarray(offs, dtype=np.int64)
    pos = offs[rows[:, 0]] + rows[:, 1]
    ev = (pos.astype(np.uint64) << np.uint64(24)) | rows[:, 2].astype(np.uint64)
    return np.sort(ev)


def call_events(rows, offs, before):
    """The events of one flow call: rows over whole flows, this call's buffer
    offsets, before[j] = the bytes flow j had before the call.  Returns (u64
    events, the number of them whose match began before the call)."""
    offs = np.asarray(offs, dtype=np.int64)
    before = np.asarray(before, dtype=np.int64)
    j = rows[:, 0]
    ln = offs[1:] - offs[:-1]
    m = (rows[:, 1] >= before[j]) & (rows[:, 1] < before[j] + ln[j])
    r = rows[m]
    pos = offs[r[:, 0]] + r[:, 1] - before[r[:, 0]]
    ev = (pos.astype(np.uint64) << np.uint64(24)) | r[:, 2].astype(np.uint64)
    return np.sort(ev), int(np.count_nonzero(r[:, 3] < before[r[:, 0]]))


def history_words(flow_bytes, W):
    """The W history words after a flow has had flow_bytes: bit b of word w = the
    byte 64 w + b + 1 places from the end was 'A'..'Z'."""
    t = np.frombuffer(bytes(flow_bytes), np.uint8)[::-1][:64 * W]
    up = np.zeros(64 * W, dtype=np.uint64)
    up[:len(t)] = (t >= 65) & (t <= 90)
    sh = np.arange(64, dtype=np.uint64)
    return np.array([np.bitwise_or.reduce(up[64 * w:64 * w + 64] << sh) for w in range(W)], dtype=np.uint64)
