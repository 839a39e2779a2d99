"""Python mirror of the plugin interface (include/pm_mps.h) over libpm.so.

Names and argument meaning follow the reference's MpsElem
(Core/src/mps.h:71-80) so tests read like the reference's own call order:

    d = Dictionary(["et.dict"])              # PatternsTree.c:260-312
    m = HipMatcher("rt")                     # mps_table[...].create()
    m.add_dictionary(d)                      # add_pattern per unique pattern
    m.compile()                              # flatten + upload to HBM
    codes = m.read_block_codes(stream_bytes) # == read_char per byte
    m.reset()                                # new stream file

Every scan goes through the HIP kernels; without a GPU, ``HipMatcher``
creation fails (the library exits, as the reference's FatalExit would).
"""
import ctypes

import numpy as np

from ._lib import load, PmPattern

KIND_RT = 1
KIND_AC = 2
KIND_AUTO = 3


def parse_line(line: bytes):
    """parser.c:63-99 via the library.  Returns the pattern bytes, or None
    when the line is rejected or empty."""
    lib = load()
    n = len(line)
    src = (ctypes.c_uint8 * max(n, 1)).from_buffer_copy(line or b"\0")
    dst = (ctypes.c_uint8 * max(n, 1))()
    k = lib.pm_parse_line(src, n, dst)
    return bytes(dst[:k]) if k else None


class Dictionary:
    """Unique patterns of the -d files, first occurrence wins."""

    def __init__(self, paths=None, patterns=None):
        self.lib = load()
        if paths is not None:
            arr = (ctypes.c_char_p * len(paths))(*[p.encode() for p in paths])
            err = ctypes.create_string_buffer(512)
            self.ptr = self.lib.pm_dict_load(arr, len(paths), err, 512)
            if not self.ptr:
                raise OSError(err.value.decode())
        else:
            self.ptr = self.lib.pm_dict_new()
            for k, p in enumerate(patterns or []):
                b = (ctypes.c_uint8 * max(len(p), 1)).from_buffer_copy(p or b"\0")
                self.lib.pm_dict_add(self.ptr, b, len(p), 0, k + 1)
            self.lib.pm_dict_finalize(self.ptr)
        d = self.ptr.contents
        self.n = d.n
        self.max_len = d.max_len
        self.lines_total = d.lines_total
        self.lines_rejected = d.lines_rejected

    def pattern(self, i):
        p = self.ptr.contents.pats[i]
        return p.file, p.line, ctypes.string_at(p.bytes, p.len)

    def pattern_ptr(self, i):
        """The pm_pattern_id_t of pattern i (address of its PmPattern)."""
        return ctypes.addressof(self.ptr.contents.pats[i])

    def patterns(self):
        return [self.pattern(i)[2] for i in range(self.n)]

    def codes(self):
        """u32 (file << 24 | line) per pattern index."""
        out = np.empty(self.n, dtype=np.uint32)
        pats = self.ptr.contents.pats
        for i in range(self.n):
            out[i] = (pats[i].file << 24) | pats[i].line
        return out

    def parents(self):
        """Index of the longest proper suffix that is a pattern, -1 if none."""
        base = ctypes.addressof(self.ptr.contents.pats[0]) if self.n else 0
        size = ctypes.sizeof(PmPattern)
        out = np.full(self.n, -1, dtype=np.int64)
        pats = self.ptr.contents.pats
        for i in range(self.n):
            par = pats[i].parent
            if par:
                out[i] = (ctypes.addressof(par.contents) - base) // size
        return out

    def gen_lines(self, n, seed) -> np.ndarray:
        """The lines stream of these patterns (pm_gen_lines_dict; the same
        bytes as HipMatcher.gen_lines of a matcher fed this dictionary)."""
        buf = np.empty(n, np.uint8)
        self.lib.pm_gen_lines_dict(self.ptr, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, seed)
        return buf

    def __del__(self):
        ptr = getattr(self, "ptr", None)
        if ptr:
            self.lib.pm_dict_free(ptr)
            self.ptr = None


def gen_stream(n, seed, mode=0, offset=0):
    """Synthetic stream, host implementation."""
    lib = load()
    buf = np.empty(n, dtype=np.uint8)
    lib.pm_gen_stream_host(buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), offset, n, seed, mode)
    return buf


def batch_offsets(buffers) -> np.ndarray:
    """The offsets array of a list of bytes-like streams laid back to back
    (HipMatcher.read_batch_*, scan_batch_device): len(buffers) + 1 int64
    values, 0 first, the total length last.  Pure numpy, no device."""
    lens = [b.size if isinstance(b, np.ndarray) else len(b) for b in buffers]
    offs = np.zeros(len(lens) + 1, dtype=np.int64)
    np.cumsum(np.asarray(lens, dtype=np.int64), out=offs[1:])
    return offs


def _concat(buffers):
    """(data, offsets) of a list of bytes-like streams: their bytes back to
    back as one u8 array, and batch_offsets of them."""
    parts = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray)
             else np.ascontiguousarray(b, dtype=np.uint8).ravel() for b in buffers]
    return (np.concatenate(parts) if parts else np.empty(0, np.uint8)), batch_offsets(buffers)


def _unique_keys(keys, name):
    """ValueError where a flow key comes twice in the packets of one
    FlowTable call (name: the method called)."""
    if len(set(keys)) != len(keys):
        seen = set()
        dup = next(k for k in keys if k in seen or seen.add(k))
        raise ValueError(f"flow {dup!r} appears twice in one {name}(): concatenate its packets")


EVENT_GID_BITS = 24


def unpack_events(ev):
    """(positions int64, gids uint32) of an array of match events
    (include/pm_hip.h: one u64 per event, position << 24 | gid)."""
    ev = np.ascontiguousarray(ev, dtype=np.uint64)
    return ((ev >> np.uint64(EVENT_GID_BITS)).astype(np.int64),
            (ev & np.uint64((1 << EVENT_GID_BITS) - 1)).astype(np.uint32))


def _split_events(pos, codes, offs):
    """Events of a batched buffer -> per stream (positions relative to the
    stream, codes); pos ascending."""
    cut = np.searchsorted(pos, offs)
    return [(pos[cut[j]:cut[j + 1]] - offs[j], codes[cut[j]:cut[j + 1]]) for j in range(len(offs) - 1)]


BY_STREAM_UNIQUE = 1  # PM_BY_STREAM_UNIQUE: one event per (stream, pattern), at its first position


def _by_stream_host_args(events, offsets, out_cap):
    """The host arrays of a per-stream-sets call: (events u64, offsets int64,
    out u64 of out_cap slots -- every event when None --, stream_ptr int64)."""
    ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1:
        raise ValueError("offsets: nseg + 1 values")
    out = np.empty(len(ev) if out_cap is None else out_cap, dtype=np.uint64)
    return ev, offs, out, np.zeros(offs.size, dtype=np.int64)


def events_by_stream_host(events, offsets, unique=True, out_cap=None):
    """pm_flat_events_by_stream, the host twin of HipMatcher.events_by_stream
    (no matcher, no device): (stream_ptr, events) with each stream's range
    ascending; the events array holds min(out_cap, stream_ptr[-1]) of them."""
    ev, offs, out, ptr = _by_stream_host_args(events, offsets, out_cap)
    u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
    rc = load().pm_flat_events_by_stream(ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1,
                                         BY_STREAM_UNIQUE if unique else 0, out.ctypes.data_as(u64p), len(out),
                                         ptr.ctypes.data_as(i64p))
    if rc != 0:
        raise ValueError(f"pm_flat_events_by_stream: bad arguments ({rc})")
    return ptr, out[:min(len(out), int(ptr[-1]))]


RULE_NEGATED = 1 << 31  # PM_RULE_NEGATED: the term must NOT be in the stream's set
RULE_FAST = 1 << 30     # PM_RULE_FAST: the term is the rule's anchor (the caller's fast_pattern)


def pack_rules(rules, fast=None):
    """(term_ptr u32 of len(rules) + 1, terms u32): the CSR form that
    pm_hip_set_rules takes.  A rule is a sequence of ints: g is a positive
    term (pattern gid g), -g a negated one; fast[r] is the gid of rule r's
    RULE_FAST term, or None."""
    rules = [list(r) for r in rules]
    if fast is not None and len(fast) != len(rules):
        raise ValueError("fast: one gid or None per rule")
    ptr = np.zeros(len(rules) + 1, dtype=np.uint32)
    terms = []
    for r, rule in enumerate(rules):
        f = None if fast is None else fast[r]
        if f is not None and f not in rule:
            raise ValueError(f"fast[{r}] = {f} is no positive term of rule {r}")
        for g in rule:
            g = int(g)
            if g == 0 or abs(g) >= 1 << EVENT_GID_BITS:
                raise ValueError(f"rule {r}: a term is a gid in [1, 2^24) or its negative, not {g}")
            terms.append((-g | RULE_NEGATED) if g < 0 else (g | RULE_FAST) if g == f else g)
        ptr[r + 1] = len(terms)
    return ptr, np.asarray(terms, dtype=np.uint32)


def rules_by_stream_host(events, offsets, rules, hits_cap=None):
    """pm_flat_rules_by_stream, the host twin of HipMatcher.rules_by_stream (no
    matcher, no device): (rule_ptr int64 of nseg + 1, hits u64 of position <<
    24 | rule) with each stream's range ascending; rules as pack_rules takes
    them, or its (term_ptr, terms) pair.  The twin sees only the list: it is
    exact for a list from an all-matches scan at a min_len no larger than the
    shortest term with a cap that held every event."""
    ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1:
        raise ValueError("offsets: nseg + 1 values")
    tptr, terms = rules if isinstance(rules, tuple) else pack_rules(rules)
    u64p, i64p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32))
    ptr = np.zeros(offs.size, dtype=np.int64)
    hits = np.empty(0 if hits_cap is None else hits_cap, dtype=np.uint64)
    for _ in range(2):  # the hits are not bounded by the events: the first call counts them
        rc = load().pm_flat_rules_by_stream(ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1,
                                            tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(tptr) - 1,
                                            hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p))
        if rc != 0:
            raise ValueError(f"pm_flat_rules_by_stream: bad arguments ({rc})")
        if hits_cap is not None or len(hits) >= ptr[-1]:
            break
        hits = np.empty(int(ptr[-1]), dtype=np.uint64)
    return ptr, hits[:min(len(hits), int(ptr[-1]))]


SEQ_FREE = 0xFFFFFFFF  # PM_SEQ_FREE: the term may lie anywhere in the stream


def _pack_seq(rules, fast):
    """(term_ptr, terms, gaps, withins, whether any term has a within)."""
    rules = [[tuple(t) for t in r] for r in rules]
    if fast is not None and len(fast) != len(rules):
        raise ValueError("fast: one gid or None per rule")
    ptr = np.zeros(len(rules) + 1, dtype=np.uint32)
    terms, gaps, withins = [], [], []
    bounded = False
    for r, rule in enumerate(rules):
        f = None if fast is None else fast[r]
        if f is not None and f not in [t[0] for t in rule]:
            raise ValueError(f"fast[{r}] = {f} is no positive term of rule {r}")
        for term in rule:
            if len(term) not in (2, 3):
                raise ValueError(f"rule {r}: a term is (gid, gap) or (gid, gap, within), not {term}")
            g, gap, within = int(term[0]), term[1], (term[2] if len(term) == 3 else None)
            if g == 0 or abs(g) >= 1 << EVENT_GID_BITS:
                raise ValueError(f"rule {r}: a term is a gid in [1, 2^24) or its negative, not {g}")
            if gap is not None and not 0 <= int(gap) <= 0x7FFFFFFF:
                raise ValueError(f"rule {r}: a gap is None or a distance in [0, 2^31), not {gap}")
            if within is not None:
                if not 0 <= int(within) <= 0x7FFFFFFF:
                    raise ValueError(f"rule {r}: a within is None or a bound in [0, 2^31), not {within}")
                bounded = True
                gap = 0 if gap is None else gap  # Snort's bare within
            if g == f:
                terms.append(g | RULE_FAST)
                f = None
            else:
                terms.append((-g | RULE_NEGATED) if g < 0 else g)
            gaps.append(SEQ_FREE if gap is None else int(gap))
            withins.append(SEQ_FREE if within is None else int(within))
        ptr[r + 1] = len(terms)
    u32 = lambda v: np.asarray(v, dtype=np.uint32)  # noqa: E731
    return ptr, u32(terms), u32(gaps), u32(withins), bounded


def pack_seq_rules(rules, fast=None):
    """(term_ptr u32 of len(rules) + 1, terms u32, gaps u32): the form that
    pm_hip_set_seq_rules takes.  A rule is a sequence of (gid, gap) pairs: g
    a positive term, -g a negated one; gap None for a free term (PM_SEQ_FREE),
    or d >= 0: the term begins at least d bytes after the positive term listed
    before it has ended.  fast[r] is the gid of rule r's RULE_FAST term (the
    first positive term of that gid), or None.  A term that carries a within
    is an error here: pack_seq_rules_within packs those."""
    ptr, terms, gaps, _, bounded = _pack_seq(rules, fast)
    if bounded:
        raise ValueError("a term carries a within: pack_seq_rules_within packs such rules")
    return ptr, terms, gaps


def pack_seq_rules_within(rules, fast=None):
    """(term_ptr, terms, gaps, withins), the form that
    pm_hip_set_seq_rules_within takes: pack_seq_rules' rules, in which a term
    may also be (gid, gap, within): within None for no upper bound
    (PM_SEQ_FREE), or w >= 0: the term ends at most w bytes after the positive
    term listed before it has ended.  A within with gap None means gap 0
    (Snort's bare within)."""
    return _pack_seq(rules, fast)[:4]


def _packed_seq(rules, fast=None):
    """(term_ptr, terms, gaps, withins or None) of rules in either packed form
    (a tuple of 3 or 4 arrays) or as any sequence of rules; withins None where
    no term has a bound."""
    if isinstance(rules, tuple) and len(rules) in (3, 4) and all(isinstance(a, np.ndarray) for a in rules):
        return tuple(rules) + (None,) if len(rules) == 3 else tuple(rules)
    ptr, terms, gaps, withins, bounded = _pack_seq(rules, fast)
    return ptr, terms, gaps, withins if bounded else None


def seq_rules_by_stream_host(events, offsets, rules, pattern_len, hits_cap=None):
    """pm_flat_seq_rules_by_stream, the host twin of
    HipMatcher.seq_rules_by_stream (no matcher, no device): (rule_ptr int64 of
    nseg + 1, hits u64 of position << 24 | rule) with each stream's range
    ascending; rules as pack_seq_rules or pack_seq_rules_within takes them, or
    the packed triple or 4-tuple; pattern_len the patterns' lengths by gid
    ([0] == 0), which the links need.  Rules with a within go through
    pm_flat_seq_rules_by_stream_within."""
    ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1:
        raise ValueError("offsets: nseg + 1 values")
    tptr, terms, gaps, withins = _packed_seq(rules)
    plen = np.ascontiguousarray(pattern_len, dtype=np.uint32)
    u64p, i64p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32))
    ptr = np.zeros(offs.size, dtype=np.int64)
    hits = np.empty(0 if hits_cap is None else hits_cap, dtype=np.uint64)
    head = (ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1, tptr.ctypes.data_as(u32p),
            terms.ctypes.data_as(u32p), gaps.ctypes.data_as(u32p))
    name = "pm_flat_seq_rules_by_stream" if withins is None else "pm_flat_seq_rules_by_stream_within"
    if withins is not None:
        head += (withins.ctypes.data_as(u32p),)
    for _ in range(2):  # the hits are not bounded by the events: the first call counts them
        rc = getattr(load(), name)(*head, len(tptr) - 1, plen.ctypes.data_as(u32p), len(plen) - 1,
                                   hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p))
        if rc != 0:
            raise ValueError(f"{name}: bad arguments ({rc})")
        if hits_cap is not None or len(hits) >= ptr[-1]:
            break
        hits = np.empty(int(ptr[-1]), dtype=np.uint64)
    return ptr, hits[:min(len(hits), int(ptr[-1]))]


FLOW_RULES_KEEP = 1  # PM_FLOW_RULES_KEEP: report the hits, leave the flows' sets as they are


def _flow_rules_host_args(offsets, sets, rows):
    """The host arrays of a flow-rules call: (offsets int64, sets -- the
    caller's own (nrows, W) u64 array, updated in place --, rows int64 or
    None, rule_ptr int64)."""
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    if offs.ndim != 1 or offs.size < 1:
        raise ValueError("offsets: nseg + 1 values")
    if not (isinstance(sets, np.ndarray) and sets.dtype == np.uint64 and sets.ndim == 2 and sets.flags.c_contiguous
            and sets.flags.writeable):
        raise ValueError("sets: a writeable C-contiguous (nrows, W) uint64 array (it is updated in place)")
    if rows is not None:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        if rows.shape != (offs.size - 1,):
            raise ValueError("rows: one row index per stream")
    return offs, sets, rows, np.zeros(offs.size, dtype=np.int64)


def flow_rule_bits_host(rules, npat):
    """pm_flat_flow_rule_bits: (bit_by_gid u32 of npat + 1 with 0xFFFFFFFF for
    a gid that no term names, K): the bit of a gid is its rank among the
    distinct gids of all terms, ascending.  rules as pack_rules takes them, or
    its pair."""
    tptr, terms = rules if isinstance(rules, tuple) else pack_rules(rules)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    bits = np.zeros(npat + 1, dtype=np.uint32)
    k = ctypes.c_uint32()
    rc = load().pm_flat_flow_rule_bits(tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(tptr) - 1, npat,
                                       bits.ctypes.data_as(u32p), ctypes.byref(k))
    if rc != 0:
        raise ValueError(f"pm_flat_flow_rule_bits: bad arguments ({rc})")
    return bits, int(k.value)


def flow_rules_host(events, offsets, rules, sets, rows=None, keep=False):
    """pm_flat_flow_rules, the host twin of HipMatcher.flow_rules (no matcher,
    no device): (rule_ptr int64 of nseg + 1, hits u64 of position << 24 |
    rule) with each stream's range ascending: the rules whose conjunction
    became true in this call, given the terms each flow carries in its row of
    sets ((nrows, W) u64, W = max(1, ceil(K / 64)) for the K distinct gids of
    the rules' terms).  rows[j] is the row of stream j (None: row j).  sets is
    updated in place unless keep.  rules as pack_rules takes them, or its
    pair."""
    ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
    offs, sets, rows, ptr = _flow_rules_host_args(offsets, sets, rows)
    tptr, terms = rules if isinstance(rules, tuple) else pack_rules(rules)
    u64p, i64p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32))

    def call(flags, hits):
        rc = load().pm_flat_flow_rules(ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1,
                                       tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(tptr) - 1,
                                       sets.ctypes.data_as(u64p), sets.shape[0], sets.shape[1],
                                       None if rows is None else rows.ctypes.data_as(i64p), flags,
                                       hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p))
        if rc != 0:
            raise ValueError(f"pm_flat_flow_rules: bad arguments ({rc})")
    # the hits are not bounded by the events and a committing call cannot be repeated: count them first
    call(FLOW_RULES_KEEP, np.empty(0, dtype=np.uint64))
    hits = np.empty(int(ptr[-1]), dtype=np.uint64)
    call(FLOW_RULES_KEEP if keep else 0, hits)
    return ptr, hits[:int(ptr[-1])]


def _packed_flow_seq(rules, fast=None):
    """(term_ptr, terms, gaps) of flow ordered rules in the packed form or as
    any sequence of rules; a within is an error."""
    ptr, terms, gaps, withins = _packed_seq(rules, fast)
    if withins is not None and np.any(withins != SEQ_FREE):
        raise ValueError("flow ordered rules take no within: a bound across packets is out of scope")
    return ptr, terms, gaps


def _flow_seq_host_args(offsets, prog, rows, pos_in):
    offs, prog, rows, ptr = _flow_rules_host_args(offsets, prog, rows)
    pos_in = np.ascontiguousarray(pos_in, dtype=np.uint64)
    if pos_in.shape != (offs.size - 1,):
        raise ValueError("pos_in: the bytes each flow had before the call, one per stream")
    return offs, prog, rows, pos_in, ptr


def flow_seq_rule_layout_host(rules, pattern_len):
    """pm_flat_flow_seq_rule_layout: (chain_word u32 by term with 0xFFFFFFFF
    where the term heads no chain of two or more, bit_by_gid u32 of npat + 1
    with 0xFFFFFFFF for a gid without a bit, C, K, S): the layout of a flow's
    progress row.  rules as pack_seq_rules takes them, or its triple."""
    tptr, terms, gaps = _packed_flow_seq(rules)
    plen = np.ascontiguousarray(pattern_len, dtype=np.uint32)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    chain = np.zeros(max(len(terms), 1), dtype=np.uint32)
    bits = np.zeros(len(plen), dtype=np.uint32)
    c, k, s = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
    rc = load().pm_flat_flow_seq_rule_layout(tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                             gaps.ctypes.data_as(u32p), len(tptr) - 1, plen.ctypes.data_as(u32p),
                                             len(plen) - 1, chain.ctypes.data_as(u32p), bits.ctypes.data_as(u32p),
                                             ctypes.byref(c), ctypes.byref(k), ctypes.byref(s))
    if rc != 0:
        raise ValueError(f"pm_flat_flow_seq_rule_layout: bad arguments ({rc})")
    return chain[:len(terms)], bits, int(c.value), int(k.value), int(s.value)


def flow_seq_rules_host(events, offsets, rules, pattern_len, prog, pos_in, rows=None, keep=False):
    """pm_flat_flow_seq_rules, the host twin of HipMatcher.flow_seq_rules (no
    matcher, no device): (rule_ptr int64 of nseg + 1, hits u64 of position <<
    24 | rule) with each stream's range ascending: the ordered rules (distance
    only) that became true in this call's bytes, given each flow's progress in
    its row of prog ((nrows, S) u64, flow_seq_rule_layout_host's S) and the
    bytes pos_in[j] that flow j had before the call.  rows[j] is the row of
    stream j (None: row j).  prog is updated in place unless keep.  rules as
    pack_seq_rules takes them, or its triple; pattern_len by gid ([0] == 0)."""
    ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
    offs, prog, rows, pos_in, ptr = _flow_seq_host_args(offsets, prog, rows, pos_in)
    tptr, terms, gaps = _packed_flow_seq(rules)
    plen = np.ascontiguousarray(pattern_len, dtype=np.uint32)
    u64p, i64p, u32p = (ctypes.POINTER(t) for t in (ctypes.c_uint64, ctypes.c_int64, ctypes.c_uint32))

    def call(flags, hits):
        rc = load().pm_flat_flow_seq_rules(ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1,
                                           tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                           gaps.ctypes.data_as(u32p), len(tptr) - 1, plen.ctypes.data_as(u32p),
                                           len(plen) - 1, prog.ctypes.data_as(u64p), prog.shape[0], prog.shape[1],
                                           None if rows is None else rows.ctypes.data_as(i64p),
                                           pos_in.ctypes.data_as(u64p), flags, hits.ctypes.data_as(u64p), len(hits),
                                           ptr.ctypes.data_as(i64p))
        if rc != 0:
            raise ValueError(f"pm_flat_flow_seq_rules: bad arguments ({rc})")
    # the hits are not bounded by the events and a committing call cannot be repeated: count them first
    call(FLOW_RULES_KEEP, np.empty(0, dtype=np.uint64))
    hits = np.empty(int(ptr[-1]), dtype=np.uint64)
    call(FLOW_RULES_KEEP if keep else 0, hits)
    return ptr, hits[:int(ptr[-1])]


class FlowTable:
    """The carried states of many live flows over one matcher (ac / auto
    kinds): a dict of flow key -> flow state, and one flow call
    (HipMatcher.read_flows_codes) per scan().

        flows = FlowTable(m)
        codes = flows.scan([(key, packet_bytes), ...])   # one array per packet
        flows.end(key)                                    # the flow is over

    A key seen for the first time starts a fresh flow.  A key may appear once
    per scan(): two packets of one flow are concatenated by the caller.
    Beside the state the table keeps the bytes each flow has had, which
    scan_windows() counts the patterns' windows from.

    scan_rules() gives the flow rules (HipMatcher.set_flow_rules) that fire
    in each packet: rules whose terms lie in different packets of a flow.
    For it the table keeps each flow's set of carried terms (rule_sets: W u64
    words per flow, HipMatcher.flow_rule_words) and the bytes the flow had
    when scan_rules() last saw it (rule_bytes).  A flow is followed by
    scan_rules() from its first byte or not at all.

    scan_seq_rules() does the same for the flow ordered rules
    (HipMatcher.set_flow_seq_rules): it keeps each flow's progress row
    (seq_rule_rows: flow_seq_rule_words u64 per flow) and the bytes the flow
    had when it last saw it (seq_rule_bytes)."""

    def __init__(self, matcher):
        self.matcher = matcher
        self.states = {}
        self.bytes = {}  # flow key -> the bytes the flow has had (scan_windows' positions)
        # scan_rules: the carried terms of each flow, and the bytes it saw
        self.rule_sets = {}
        self.rule_bytes = {}
        # scan_seq_rules: the progress row of each flow, and the bytes it saw
        self.seq_rule_rows = {}
        self.seq_rule_bytes = {}
        # scan_nocase: the folded automaton's states, the case histories, and the bytes it saw
        self.nocase_states = {}
        self.nocase_case = {}
        self.nocase_bytes = {}

    def scan(self, packets):
        """packets: a list of (key, bytes-like).  Returns the codes of each
        packet, in order, every flow continued from its earlier packets."""
        keys = [k for k, _ in packets]
        _unique_keys(keys, "scan")
        if not packets:
            return []
        data, offs = _concat([b for _, b in packets])
        state = np.array([self.states.get(k, 0) for k in keys], dtype=np.uint32)
        codes, state = self.matcher.read_flows_codes(data, offs, state)
        for k, s in zip(keys, state.tolist()):
            self.states[k] = s
        self._advance(keys, offs)
        return [codes[offs[j]:offs[j + 1]] for j in range(len(packets))]

    def scan_events(self, packets, min_len=3):
        """scan() with the match list instead of dense codes: per packet, in
        order, (positions inside the packet, codes) of the positions where a
        pattern of at least min_len bytes ends (HipMatcher.read_flows_events).
        The flows' states advance exactly as in scan()."""
        return self._scan_list(packets, min_len, self.matcher.read_flows_events, "scan_events")

    def scan_matches(self, packets, min_len=3):
        """scan_events() with every pattern that ends at a position, not only
        the longest (HipMatcher.read_flows_matches): per packet (positions,
        codes), a position once per pattern of at least min_len bytes ending
        there.  The flows' states advance exactly as in scan()."""
        return self._scan_list(packets, min_len, self.matcher.read_flows_matches, "scan_matches")

    def scan_groups(self, packets, min_len=3, all_matches=True):
        """scan_matches() with a group mask per packet: packets is a list of
        (key, bytes-like, groups), and a packet's list holds the patterns
        visible to it only (HipMatcher.read_flows_groups).  The flows' states
        advance exactly as in scan(), whatever the masks."""
        grp = np.array([g for _, _, g in packets], dtype=np.uint32)

        def read(data, offs, state, min_len):
            return self.matcher.read_flows_groups(data, offs, grp, state, min_len, all_matches)
        return self._scan_list([(k, b) for k, b, _ in packets], min_len, read, "scan_groups")

    def scan_windows(self, packets, min_len=3, all_matches=True):
        """scan_groups() with the patterns' windows (HipMatcher.set_windows)
        applied at each flow's own byte count: packets is a list of (key,
        bytes-like) or (key, bytes-like, groups), all of one shape.  The table
        keeps the bytes every flow has had, whichever scan method saw them,
        so a window counts from the flow's first byte, not the packet's
        (HipMatcher.read_flows_windows).  The flows' states advance exactly
        as in scan()."""
        grp = None
        if packets and len(packets[0]) == 3:
            grp = np.array([g for _, _, g in packets], dtype=np.uint32)
        pos_in = np.array([self.bytes.get(p[0], 0) for p in packets], dtype=np.uint64)

        def read(data, offs, state, min_len):
            return self.matcher.read_flows_windows(data, offs, grp, state, pos_in, min_len, all_matches)[:3]
        return self._scan_list([(p[0], p[1]) for p in packets], min_len, read, "scan_windows")

    def scan_nocase(self, packets, min_len=3, all_matches=True):
        """scan_windows() with the patterns' nocase flags honoured
        (HipMatcher.set_nocase; groups and windows where they are set):
        packets as there.  The nocase scan walks the folded automaton, so the
        table keeps its states and the flows' case histories in dictionaries
        of their own, beside the bytes each flow had when scan_nocase last
        saw it.  A flow that got bytes through another scan method since
        cannot be continued (the folded automaton missed them): ValueError."""
        grp = None
        if packets and len(packets[0]) == 3:
            grp = np.array([g for _, _, g in packets], dtype=np.uint32)
        keys = [p[0] for p in packets]
        _unique_keys(keys, "scan_nocase")
        for k in keys:
            if self.bytes.get(k, 0) != self.nocase_bytes.get(k, 0):
                raise ValueError(f"flow {k!r} has had {self.bytes.get(k, 0)} bytes but scan_nocase() saw "
                                 f"{self.nocase_bytes.get(k, 0)} of them")
        if not packets:
            return []
        data, offs = _concat([p[1] for p in packets])
        W = self.matcher.case_words
        state = np.array([self.nocase_states.get(k, 0) for k in keys], dtype=np.uint32)
        pos_in = np.array([self.bytes.get(k, 0) for k in keys], dtype=np.uint64)
        case = np.zeros((len(keys), W), dtype=np.uint64)
        for r, k in enumerate(keys):
            if k in self.nocase_case:
                case[r] = self.nocase_case[k]
        pos, codes, state, _, case = self.matcher.read_flows_nocase(data, offs, grp, state, pos_in, case, min_len,
                                                                    all_matches)
        for r, k in enumerate(keys):
            self.nocase_states[k] = int(state[r])
            self.nocase_case[k] = case[r].copy()
        self._advance(keys, offs)
        for k in keys:
            self.nocase_bytes[k] = self.bytes[k]
        return _split_events(pos, codes, offs)

    def scan_rules(self, packets):
        """packets: a list of (key, bytes-like).  Per packet, in order,
        (positions inside the packet, rule indices) of the flow rules
        (HipMatcher.set_flow_rules) whose conjunction became true in that
        packet, ascending by (position, rule): the terms a flow's earlier
        packets held count, a rule fires at most once per flow, and a negated
        term seen so far suppresses it.  One read_flows_matches call at
        flow_rules_min_len() from the flows' states, then flow_rules over the
        flows' kept sets.  The flows' states and byte counts advance exactly
        as in scan().  A flow that got bytes through another scan method
        since scan_rules() last saw it cannot be continued (its set missed
        their patterns): ValueError; so is a kept set whose length is not the
        matcher's current flow_rule_words (the rules were replaced)."""
        keys = [k for k, _ in packets]
        _unique_keys(keys, "scan_rules")
        W = self.matcher.flow_rule_words
        if W == 0:
            raise ValueError("scan_rules() before the matcher's set_flow_rules()")
        for k in keys:
            if self.bytes.get(k, 0) != self.rule_bytes.get(k, 0):
                raise ValueError(f"flow {k!r} has had {self.bytes.get(k, 0)} bytes but scan_rules() saw "
                                 f"{self.rule_bytes.get(k, 0)} of them")
            if k in self.rule_sets and len(self.rule_sets[k]) != W:
                raise ValueError(f"flow {k!r} keeps a set of {len(self.rule_sets[k])} words but the matcher's flow "
                                 f"rules need {W}")
        if not packets:
            return []
        data, offs = _concat([b for _, b in packets])
        state = np.array([self.states.get(k, 0) for k in keys], dtype=np.uint32)
        sets = np.zeros((len(keys), W), dtype=np.uint64)
        for r, k in enumerate(keys):
            if k in self.rule_sets:
                sets[r] = self.rule_sets[k]
        # read_flows_matches' call, its events kept as they are (position << 24 | gid)
        ev, state = self.matcher._read_events(data, offs, state, self.matcher.flow_rules_min_len(), all_matches=True)
        ptr, hits = self.matcher.flow_rules(ev, offs, sets)
        for r, (k, s) in enumerate(zip(keys, state.tolist())):
            self.states[k] = s
            self.rule_sets[k] = sets[r].copy()
        self._advance(keys, offs)
        for k in keys:
            self.rule_bytes[k] = self.bytes[k]
        hpos, rule = unpack_events(hits)
        return [(hpos[ptr[j]:ptr[j + 1]] - offs[j], rule[ptr[j]:ptr[j + 1]]) for j in range(len(packets))]

    def scan_seq_rules(self, packets):
        """scan_rules() for the flow ordered rules
        (HipMatcher.set_flow_seq_rules): per packet, in order, (positions
        inside the packet, rule indices) of the ordered rules that became
        true in that packet, ascending by (position, rule): a chain's head
        may lie in an earlier packet than its follower, and a link is
        measured in the flow's bytes.  One read_flows_matches call at
        flow_seq_rules_min_len() from the flows' states, then flow_seq_rules
        over the flows' kept rows and the table's byte counts.  The flows'
        states and byte counts advance exactly as in scan().  A flow that got
        bytes through another scan method since scan_seq_rules() last saw it
        cannot be continued (its row missed their patterns): ValueError; so
        is a kept row whose length is not the matcher's current
        flow_seq_rule_words (the rules were replaced)."""
        keys = [k for k, _ in packets]
        _unique_keys(keys, "scan_seq_rules")
        S = self.matcher.flow_seq_rule_words
        if S == 0:
            raise ValueError("scan_seq_rules() before the matcher's set_flow_seq_rules()")
        for k in keys:
            if self.bytes.get(k, 0) != self.seq_rule_bytes.get(k, 0):
                raise ValueError(f"flow {k!r} has had {self.bytes.get(k, 0)} bytes but scan_seq_rules() saw "
                                 f"{self.seq_rule_bytes.get(k, 0)} of them")
            if k in self.seq_rule_rows and len(self.seq_rule_rows[k]) != S:
                raise ValueError(f"flow {k!r} keeps a row of {len(self.seq_rule_rows[k])} words but the matcher's "
                                 f"flow ordered rules need {S}")
        if not packets:
            return []
        data, offs = _concat([b for _, b in packets])
        state = np.array([self.states.get(k, 0) for k in keys], dtype=np.uint32)
        pos_in = np.array([self.bytes.get(k, 0) for k in keys], dtype=np.uint64)
        prog = np.zeros((len(keys), S), dtype=np.uint64)
        for r, k in enumerate(keys):
            if k in self.seq_rule_rows:
                prog[r] = self.seq_rule_rows[k]
        ev, state = self.matcher._read_events(data, offs, state, self.matcher.flow_seq_rules_min_len(),
                                              all_matches=True)
        ptr, hits = self.matcher.flow_seq_rules(ev, offs, prog, pos_in)
        for r, (k, s) in enumerate(zip(keys, state.tolist())):
            self.states[k] = s
            self.seq_rule_rows[k] = prog[r].copy()
        self._advance(keys, offs)
        for k in keys:
            self.seq_rule_bytes[k] = self.bytes[k]
        hpos, rule = unpack_events(hits)
        return [(hpos[ptr[j]:ptr[j + 1]] - offs[j], rule[ptr[j]:ptr[j + 1]]) for j in range(len(packets))]

    def _advance(self, keys, offs):
        for k, n in zip(keys, np.diff(offs).tolist()):
            self.bytes[k] = self.bytes.get(k, 0) + n

    def _scan_list(self, packets, min_len, read, name):
        keys = [k for k, _ in packets]
        _unique_keys(keys, name)
        if not packets:
            return []
        data, offs = _concat([b for _, b in packets])
        state = np.array([self.states.get(k, 0) for k in keys], dtype=np.uint32)
        pos, codes, state = read(data, offs, state, min_len)
        for k, s in zip(keys, state.tolist()):
            self.states[k] = s
        self._advance(keys, offs)
        return _split_events(pos, codes, offs)

    def end(self, key):
        """Forget a flow: its key, seen again, starts a fresh one."""
        self.states.pop(key, None)
        self.bytes.pop(key, None)
        self.nocase_states.pop(key, None)
        self.nocase_case.pop(key, None)
        self.nocase_bytes.pop(key, None)
        self.rule_sets.pop(key, None)
        self.rule_bytes.pop(key, None)
        self.seq_rule_rows.pop(key, None)
        self.seq_rule_bytes.pop(key, None)

    def __len__(self):
        return len(self.states)

    def __contains__(self, key):
        return key in self.states


class HipMatcher:
    """One GPU matcher instance ("rt" = reverse-trie kernel, "ac" = AC DFA,
    "auto" = both, picked per launch)."""

    def __init__(self, kind="rt"):
        self.lib = load()
        self.kind_name = kind
        self.obj = getattr(self.lib, {"rt": "pm_hip_rt_create", "ac": "pm_hip_ac_create",
                                      "auto": "pm_hip_auto_create"}[kind])()
        self._codes = None
        self._dict = None

    # --- MpsElem -------------------------------------------------------
    def add_pattern(self, pat: bytes, pattern_id=None):
        self.lib.pm_hip_add_pattern(self.obj, pat, len(pat), pattern_id)

    def add_dictionary(self, d: Dictionary):
        fn = ctypes.cast(self.lib.pm_hip_add_pattern, ctypes.c_void_p)
        self.lib.pm_dict_feed(d.ptr, self.obj, fn)
        self._dict = d

    def compile(self):
        self.lib.pm_hip_compile(self.obj)
        if self._dict is not None:
            self._codes = self.gid_codes(self._dict.codes())

    def compile_stats(self):
        """Start-up cost of the last compile(): {"compile_ms", "upload_ms",
        "image_bytes", "image_cache_hit"} (pm_hip_compile_stats)."""
        c, u = ctypes.c_double(), ctypes.c_double()
        if self.lib.pm_hip_compile_stats(self.obj, ctypes.byref(c), ctypes.byref(u)) != 0:
            raise RuntimeError("compile_stats before compile()")
        return {"compile_ms": round(c.value, 2), "upload_ms": round(u.value, 2),
                "image_bytes": int(self.lib.pm_hip_table_bytes(self.obj)),
                "image_cache_hit": bool(self.lib.pm_hip_image_cache_hit(self.obj))}

    def serve_stats(self):
        """The resident small-call server of an rt object ("host_serve"):
        {"launches": grids launched, "calls": requests served}
        (pm_hip_serve_stats)."""
        la, ca = ctypes.c_uint64(), ctypes.c_uint64()
        self.lib.pm_hip_serve_stats(self.obj, ctypes.byref(la), ctypes.byref(ca))
        return {"launches": la.value, "calls": ca.value}

    def set_image_cache(self, directory: str):
        self.lib.pm_hip_set_image_cache(self.obj, directory.encode())

    def read_char(self, c: int):
        return self.lib.pm_hip_read_char(self.obj, bytes([c]))

    def read_block_ids(self, data: bytes):
        """pm_pattern_id_t per position (ints; 0 = null)."""
        n = len(data)
        out = (ctypes.c_void_p * max(n, 1))()
        self.lib.pm_hip_read_block(self.obj, data, n, out)
        return [x or 0 for x in out[:n]]

    def read_block_id_array(self, data) -> np.ndarray:
        """pm_hip_read_block into a numpy uintp array (pattern id per position)."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        out = np.empty(max(len(arr), 1), dtype=np.uintp)
        self.lib.pm_hip_read_block(self.obj, arr.ctypes.data_as(ctypes.c_char_p), len(arr),
                                   out.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)))
        return out[:len(arr)]

    def total_mem(self):
        return self.lib.pm_hip_total_mem(self.obj)

    def reset(self):
        self.lib.pm_hip_reset(self.obj)

    def free(self):
        if self.obj:
            self.lib.pm_hip_free(self.obj)
            self.obj = None

    def set_option(self, name: str, value: int) -> int:
        """pm_hip_set_option: a per-object option (include/pm_hip.h lists
        them); 0 on success, -1 for an unknown name or value."""
        return self.lib.pm_hip_set_option(self.obj, name.encode(), int(value))

    def _check(self, rc):
        """RuntimeError with the library's message for a call that returned rc != 0."""
        if rc != 0:
            raise RuntimeError(self.lib.pm_hip_last_error().decode())

    # --- batch ---------------------------------------------------------
    def read_block_gids(self, data) -> np.ndarray:
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        out = np.empty(len(arr), dtype=np.uint32)
        self.lib.pm_hip_read_block_gid(self.obj, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), len(arr),
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        return out

    def gid_codes(self, index_codes: np.ndarray) -> np.ndarray:
        """Table gid -> value, given a value per pattern index (add order)."""
        P = self.lib.pm_hip_n_patterns(self.obj)
        tab = np.zeros(P + 1, dtype=index_codes.dtype)
        for g in range(1, P + 1):
            tab[g] = index_codes[self.lib.pm_hip_gid_index(self.obj, g)]
        return tab

    def read_block_codes(self, data) -> np.ndarray:
        """(file << 24 | line) per position, the golden-fixture format."""
        return self._codes[self.read_block_gids(data)]

    def scan_device(self, d_text_ptr, stream_start, pos0, n, d_out_ptr, d_count_ptr, stream_ptr, out_width=4):
        """Device-resident scan (pm_hip_scan_device / _scan_device16): ids of
        out_width bytes (4 = u32, 2 = u16) to d_out_ptr, or count only."""
        fn = {4: self.lib.pm_hip_scan_device, 2: self.lib.pm_hip_scan_device16}[out_width]
        rc = fn(self.obj, d_text_ptr, stream_start, pos0, n, d_out_ptr, d_count_ptr, stream_ptr)
        self._check(rc)

    # --- batched scan: many independent streams in one launch ------------
    def scan_batch_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_out_ptr, d_count_ptr, stream_ptr, out_width=4):
        """pm_hip_scan_batch_device / _device16: nseg streams back to back in
        d_text[0, n), stream j = [offsets[j], offsets[j+1]) (nseg + 1 device
        int64 values); dense ids of out_width bytes to d_out_ptr, or count
        only.  Every stream is scanned from its own first byte."""
        fn = {4: self.lib.pm_hip_scan_batch_device, 2: self.lib.pm_hip_scan_batch_device16}[out_width]
        rc = fn(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_out_ptr, d_count_ptr, stream_ptr)
        self._check(rc)

    def read_batch_gids(self, data, offsets, out=None) -> np.ndarray:
        """pm_hip_read_batch_gid: gids (u32) of the streams data[offsets[j]:
        offsets[j+1]], each from its own start, in buffer order.  Leaves the
        stream read_block / read_char carry untouched.  out: a contiguous u32
        array of len(data) to fill instead of a new one (a caller in a loop
        then pays no page faults of a fresh array per call)."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or int(offs[-1]) != len(arr):
            raise ValueError("offsets: nseg + 1 values, the last one len(data)")
        if out is None:
            out = np.empty(len(arr), dtype=np.uint32)
        elif out.dtype != np.uint32 or out.shape != (len(arr),) or not out.flags.c_contiguous:
            raise ValueError("out: a contiguous uint32 array of len(data)")
        rc = self.lib.pm_hip_read_batch_gid(self.obj, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), offs.size - 1,
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        self._check(rc)
        return out

    def read_batch_codes(self, data, offsets) -> np.ndarray:
        """(file << 24 | line) per position, like read_block_codes."""
        return self._codes[self.read_batch_gids(data, offsets)]

    def read_batch_id_array(self, data, offsets) -> np.ndarray:
        """pm_hip_read_batch: the add_pattern id per position (uintp)."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or int(offs[-1]) != len(arr):
            raise ValueError("offsets: nseg + 1 values, the last one len(data)")
        out = np.empty(max(len(arr), 1), dtype=np.uintp)
        rc = self.lib.pm_hip_read_batch(self.obj, arr.ctypes.data_as(ctypes.c_char_p),
                                        offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), offs.size - 1,
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)))
        self._check(rc)
        return out[:len(arr)]

    def read_many_codes(self, buffers):
        """One batch call over a list of bytes-like streams; the codes of
        each, in order."""
        data, offs = _concat(buffers)
        codes = self.read_batch_codes(data, offs)
        return [codes[offs[j]:offs[j + 1]] for j in range(len(buffers))]

    # --- match list: events instead of dense ids (batched and flow scans) --
    def pattern_len(self, gid):
        """pm_hip_pattern_len: the bytes of pattern gid (0 out of range)."""
        return self.lib.pm_hip_pattern_len(self.obj, gid)

    def scan_batch_events_device(self, d_text_ptr, d_offsets_ptr, nseg, n, min_len, d_events_ptr, cap, d_nevents_ptr,
                                 stream_ptr):
        """pm_hip_scan_batch_events_device: scan_batch_device's streams, but
        the output is the match list: one u64 event (position << 24 | gid)
        per position whose answer has at least min_len bytes, appended at the
        device u64 cursor d_nevents_ptr into d_events_ptr[0, cap)."""
        rc = self.lib.pm_hip_scan_batch_events_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, min_len,
                                                      d_events_ptr, cap, d_nevents_ptr, stream_ptr)
        self._check(rc)

    def scan_flows_events_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr, min_len,
                                 d_events_ptr, cap, d_nevents_ptr, stream_ptr):
        """pm_hip_scan_flows_events_device: scan_flows_device's streams and
        states with the match list of scan_batch_events_device as output."""
        rc = self.lib.pm_hip_scan_flows_events_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr,
                                                      d_state_out_ptr, min_len, d_events_ptr, cap, d_nevents_ptr,
                                                      stream_ptr)
        self._check(rc)

    def _read_list(self, form, data, offsets, min_len, all_matches, stream_groups=None, state=None, pos=None,
                   case=None):
        """The host list forms, pm_hip_read_{batch,flows}_<form>: form is
        "events", "matches", "groups", "windows" or "nocase"; state None is
        the batched call, an array the flow one.  Returns (events u64
        ascending, state_out, pos_out, case_out), each of the last three None
        where it was not passed.  A host buffer too short for the call's
        events means one more call with room for all of them, from the same
        states, positions and histories."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or int(offs[-1]) != len(arr):
            raise ValueError("offsets: nseg + 1 values, the last one len(data)")
        nseg = offs.size - 1
        for name, a in (("state", state), ("pos", pos)):
            if a is not None and a.shape != (nseg,):
                raise ValueError(f"{name}: nseg values")
        if case is not None and case.shape != (nseg, self.case_words):
            raise ValueError("case: nseg rows of case_words values")
        grp = None
        if stream_groups is not None:
            grp = np.ascontiguousarray(stream_groups, dtype=np.uint32)
            if grp.shape != (nseg,):
                raise ValueError("stream_groups: nseg values")
        u32p, u64p = ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint64)

        def ptr(a, t):
            return None if a is None else a.ctypes.data_as(t)
        fn = getattr(self.lib, f"pm_hip_read_{'batch' if state is None else 'flows'}_{form}")
        cap = max(1024, len(arr) // 16)
        while True:
            ev = np.empty(cap, dtype=np.uint64)
            total = ctypes.c_size_t(0)
            st, ps, cs = (None if a is None else a.copy() for a in (state, pos, case))
            args = [self.obj, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                    offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nseg]
            if state is not None:  # what a flow carries, as far as the form has it
                args.append(st.ctypes.data_as(u32p))
                if form in ("windows", "nocase"):
                    args.append(ptr(ps, u64p))
                if form == "nocase":
                    args.append(ptr(cs if cs is not None and cs.size else None, u64p))  # no words: NULL
            if form in ("events", "matches"):
                args.append(min_len)
            else:
                args += [ptr(grp, u32p), min_len, int(bool(all_matches))]
            self._check(fn(*args, ev.ctypes.data_as(u64p), cap, ctypes.byref(total)))
            if total.value <= cap:
                return ev[:total.value], st, ps, cs
            cap = total.value

    def _read_events(self, data, offsets, state, min_len, all_matches=False, stream_groups=None):
        """_read_list for the events forms (all_matches: the *_matches ones;
        stream_groups: the *_groups ones, in the form all_matches names):
        (events u64 ascending, state_out or None)."""
        form = "groups" if stream_groups is not None else "matches" if all_matches else "events"
        return self._read_list(form, data, offsets, min_len, all_matches, stream_groups, state)[:2]

    def read_batch_events(self, data, offsets, min_len=3):
        """pm_hip_read_batch_events: (positions int64, codes) of the positions
        of read_batch_codes' answer where a pattern of at least min_len bytes
        ends, in position order; codes as read_batch_codes gives them."""
        ev, _ = self._read_events(data, offsets, None, min_len)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids]

    def read_many_events(self, buffers, min_len=3):
        """One batch events call over a list of bytes-like streams: per
        stream, in order, (positions inside the stream, codes)."""
        data, offs = _concat(buffers)
        pos, codes = self.read_batch_events(data, offs, min_len)
        return _split_events(pos, codes, offs)

    def read_flows_events(self, data, offsets, state=None, min_len=3):
        """pm_hip_read_flows_events: (positions, codes, state_out) -- the
        events of read_flows_codes' answer and the flows' states, which
        advance exactly as in read_flows_codes."""
        nseg = len(offsets) - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        ev, st = self._read_events(data, offsets, st, min_len)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids], st

    # --- all matches: every pattern that ends at a position ----------------
    def scan_batch_matches_device(self, d_text_ptr, d_offsets_ptr, nseg, n, min_len, d_events_ptr, cap, d_nevents_ptr,
                                  stream_ptr):
        """pm_hip_scan_batch_matches_device: scan_batch_events_device with an
        event for every pattern of at least min_len bytes that ends at a
        position (the answer's suffix chain), not only the longest; the
        cursor may end above n."""
        rc = self.lib.pm_hip_scan_batch_matches_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, min_len,
                                                       d_events_ptr, cap, d_nevents_ptr, stream_ptr)
        self._check(rc)

    def scan_flows_matches_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr, min_len,
                                  d_events_ptr, cap, d_nevents_ptr, stream_ptr):
        """pm_hip_scan_flows_matches_device: scan_flows_events_device with the
        list of scan_batch_matches_device."""
        rc = self.lib.pm_hip_scan_flows_matches_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr,
                                                       d_state_out_ptr, min_len, d_events_ptr, cap, d_nevents_ptr,
                                                       stream_ptr)
        self._check(rc)

    def read_batch_matches(self, data, offsets, min_len=3):
        """pm_hip_read_batch_matches: read_batch_events with every pattern
        that ends at a position: (positions int64, codes), ascending by
        position and, within a position, by gid."""
        ev, _ = self._read_events(data, offsets, None, min_len, all_matches=True)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids]

    def read_many_matches(self, buffers, min_len=3):
        """read_many_events with every pattern that ends at a position."""
        data, offs = _concat(buffers)
        pos, codes = self.read_batch_matches(data, offs, min_len)
        return _split_events(pos, codes, offs)

    def read_flows_matches(self, data, offsets, state=None, min_len=3):
        """pm_hip_read_flows_matches: read_flows_events with every pattern
        that ends at a position: (positions, codes, state_out)."""
        nseg = len(offsets) - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        ev, st = self._read_events(data, offsets, st, min_len, all_matches=True)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids], st

    # --- per-stream sets: a match list grouped by stream ---------------------
    def by_stream_scratch_bytes(self, cap, nseg, unique=True):
        """pm_hip_by_stream_scratch_bytes: the device scratch, in bytes, that
        events_by_stream_device needs for a list of cap slots over nseg streams."""
        b = self.lib.pm_hip_by_stream_scratch_bytes(cap, nseg, BY_STREAM_UNIQUE if unique else 0)
        if b == ctypes.c_size_t(-1).value:
            raise ValueError("by_stream_scratch_bytes: cap <= 2^40, 0 <= nseg < 2^31")
        return b

    def events_by_stream_device(self, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg, flags, d_out_ptr, out_cap,
                                d_stream_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr):
        """pm_hip_events_by_stream_device: the list a scan left in
        d_events_ptr[0, cap) behind the device cursor d_nevents_ptr, grouped by
        the scan's streams: stream j's events to d_out_ptr[ptr[j] .. ptr[j+1])
        with ptr = the nseg + 1 int64 at d_stream_ptr_ptr; flags
        BY_STREAM_UNIQUE keeps one event per (stream, pattern), at its first
        position.  Enqueued on stream_ptr, no synchronize."""
        rc = self.lib.pm_hip_events_by_stream_device(self.obj, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg,
                                                     flags, d_out_ptr, out_cap, d_stream_ptr_ptr, d_scratch_ptr,
                                                     scratch_bytes, stream_ptr)
        self._check(rc)

    def events_by_stream(self, events, offsets, unique=True):
        """pm_hip_events_by_stream: host arrays through the device call:
        (stream_ptr int64 of nseg + 1, events u64), stream j's events
        events[ptr[j]:ptr[j+1]] ascending; unique: one per (stream, pattern),
        at the pattern's first position in the stream."""
        ev, offs, out, ptr = _by_stream_host_args(events, offsets, None)
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
        rc = self.lib.pm_hip_events_by_stream(self.obj, ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p),
                                              offs.size - 1, BY_STREAM_UNIQUE if unique else 0,
                                              out.ctypes.data_as(u64p), len(out), ptr.ctypes.data_as(i64p))
        self._check(rc)
        return ptr, out[:int(ptr[-1])]

    def read_many_sets(self, buffers, min_len=3, all_matches=True):
        """One batch list call over a list of bytes-like streams, then
        events_by_stream: per stream, in order, (first positions inside the
        stream, codes) of the distinct patterns of at least min_len bytes that
        end in it (all_matches False: of the longest pattern per position)."""
        data, offs = _concat(buffers)
        ev, _ = self._read_events(data, offs, None, min_len, all_matches=all_matches)
        ptr, ev = self.events_by_stream(ev, offs, unique=True)
        pos, gids = unpack_events(ev)
        codes = self._codes[gids]
        return [(pos[ptr[j]:ptr[j + 1]] - offs[j], codes[ptr[j]:ptr[j + 1]]) for j in range(len(buffers))]

    # --- rules: which multi-pattern rules fire in each stream ------------------
    def set_rules(self, rules, fast=None):
        """pm_hip_set_rules: a rule is a sequence of 1 to 64 ints, g a
        positive term (pattern gid g must be in the stream's set), -g a
        negated one (it must not); fast[r] is the gid of rule r's anchor (its
        fast_pattern) or None (the longest positive term).  After compile(); a
        later call replaces the rules (no rules call may be in flight)."""
        ptr, terms = pack_rules(rules, fast)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self.lib.pm_hip_set_rules(self.obj, ptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                              len(ptr) - 1))

    def rule_count(self):
        """pm_hip_rule_count: the rules set (0 before set_rules)."""
        return int(self.lib.pm_hip_rule_count(self.obj))

    def rules_min_len(self):
        """pm_hip_rules_min_len: the length of the shortest pattern any term
        names: the largest min_len a scan may use for exact rule hits (0
        before set_rules)."""
        return int(self.lib.pm_hip_rules_min_len(self.obj))

    def rules_scratch_bytes(self, cap, nseg):
        """pm_hip_rules_scratch_bytes: the device scratch, in bytes, that
        rules_by_stream_device needs for a list of cap slots over nseg streams."""
        b = self.lib.pm_hip_rules_scratch_bytes(cap, nseg)
        if b == ctypes.c_size_t(-1).value:
            raise ValueError("rules_scratch_bytes: cap <= 2^40, 0 <= nseg < 2^31")
        return b

    def rules_by_stream_device(self, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg, d_hits_ptr, hits_cap,
                               d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr):
        """pm_hip_rules_by_stream_device: the rules that fire in each of the
        scan's streams, from the list the scan left in d_events_ptr[0, cap)
        behind the device cursor d_nevents_ptr: stream j's hits (position <<
        24 | rule) to d_hits_ptr[ptr[j] .. ptr[j+1]) with ptr = the nseg + 1
        int64 at d_rule_ptr_ptr, exact whatever hits_cap is.  Enqueued on
        stream_ptr, no synchronize.  Rules see only what the list holds: scan
        with an all-matches form, at a min_len <= rules_min_len(), with a cap
        that holds the whole list."""
        rc = self.lib.pm_hip_rules_by_stream_device(self.obj, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg,
                                                    d_hits_ptr, hits_cap, d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes,
                                                    stream_ptr)
        self._check(rc)

    def rules_by_stream(self, events, offsets):
        """pm_hip_rules_by_stream: host arrays through the device call:
        (rule_ptr int64 of nseg + 1, hits u64), stream j's hits
        hits[ptr[j]:ptr[j+1]] ascending, each position << 24 | rule with the
        position at which the rule's last positive term first appeared
        (unpack_events splits them).  Rules see only what the list holds:
        events from an all-matches scan, at a min_len <= rules_min_len(), with
        a cap that held the whole list."""
        ev, offs, _, ptr = _by_stream_host_args(events, offsets, 0)
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
        hits = np.empty(max(len(ev), 1), dtype=np.uint64)
        for _ in range(2):  # the hits are not bounded by the events: rule_ptr[-1] sizes the retry
            rc = self.lib.pm_hip_rules_by_stream(self.obj, ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p),
                                                 offs.size - 1, hits.ctypes.data_as(u64p), len(hits),
                                                 ptr.ctypes.data_as(i64p))
            self._check(rc)
            if len(hits) >= ptr[-1]:
                break
            hits = np.empty(int(ptr[-1]), dtype=np.uint64)
        return ptr, hits[:int(ptr[-1])]

    def read_many_rules(self, buffers):
        """One all-matches batch list call over a list of bytes-like streams at
        rules_min_len(), then rules_by_stream: per stream, in order,
        (positions inside the stream, rule indices) of the rules that fire in
        it, ascending by position."""
        data, offs = _concat(buffers)
        ev, _ = self._read_events(data, offs, None, self.rules_min_len(), all_matches=True)
        ptr, hits = self.rules_by_stream(ev, offs)
        pos, rule = unpack_events(hits)
        return [(pos[ptr[j]:ptr[j + 1]] - offs[j], rule[ptr[j]:ptr[j + 1]]) for j in range(len(buffers))]

    # --- ordered rules: terms that follow one another at a distance -------------
    def set_seq_rules(self, rules, fast=None):
        """pm_hip_set_seq_rules: a rule set of its own (set_rules and
        set_flow_rules are not touched).  A rule is a sequence of 1 to 64
        (gid, gap) pairs as pack_seq_rules takes them: gap None for a free
        term, d >= 0 for one that begins at least d bytes after the positive
        term before it has ended (d = 0 is Snort's distance:0); -gid a negated
        term.  A term may also be (gid, gap, within) as pack_seq_rules_within
        takes it: it ends at most within bytes after the term before it has
        ended (pm_hip_set_seq_rules_within; any such term and the exact walk
        evaluates the set).  After compile(); a later call replaces the rules (no
        ordered-rules call may be in flight)."""
        ptr, terms, gaps, withins = _packed_seq(rules, fast)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        if withins is None:
            rc = self.lib.pm_hip_set_seq_rules(self.obj, ptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                               gaps.ctypes.data_as(u32p), len(ptr) - 1)
        else:
            rc = self.lib.pm_hip_set_seq_rules_within(self.obj, ptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                                      gaps.ctypes.data_as(u32p), withins.ctypes.data_as(u32p),
                                                      len(ptr) - 1)
        self._check(rc)

    def seq_rules_within_run(self):
        """pm_hip_seq_rules_within_run: the longest run of consecutive bounded
        links (terms with a within) in any rule of the set; 0 where no term
        has a bound and before set_seq_rules."""
        return int(self.lib.pm_hip_seq_rules_within_run(self.obj))

    def seq_rule_count(self):
        """pm_hip_seq_rule_count: the ordered rules set (0 before set_seq_rules)."""
        return int(self.lib.pm_hip_seq_rule_count(self.obj))

    def seq_rules_min_len(self):
        """pm_hip_seq_rules_min_len: the length of the shortest pattern any
        term names: the largest min_len a scan may use for exact hits (0
        before set_seq_rules)."""
        return int(self.lib.pm_hip_seq_rules_min_len(self.obj))

    def seq_rules_scratch_bytes(self, cap, nseg):
        """pm_hip_seq_rules_scratch_bytes: the device scratch, in bytes, that
        seq_rules_by_stream_device needs for a list of cap slots over nseg
        streams."""
        b = self.lib.pm_hip_seq_rules_scratch_bytes(cap, nseg)
        if b == ctypes.c_size_t(-1).value:
            raise ValueError("seq_rules_scratch_bytes: cap <= 2^40, 0 <= nseg < 2^31")
        return b

    def seq_rules_by_stream_device(self, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg, d_hits_ptr, hits_cap,
                                   d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr):
        """pm_hip_seq_rules_by_stream_device: the ordered rules that fire in
        each of the scan's streams; the arguments and the output of
        rules_by_stream_device, the scratch seq_rules_scratch_bytes(cap, nseg).
        Enqueued on stream_ptr, no synchronize.  Scan with an all-matches
        form, at a min_len <= seq_rules_min_len(), with a cap that holds the
        whole list."""
        rc = self.lib.pm_hip_seq_rules_by_stream_device(self.obj, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr,
                                                        nseg, d_hits_ptr, hits_cap, d_rule_ptr_ptr, d_scratch_ptr,
                                                        scratch_bytes, stream_ptr)
        self._check(rc)

    def seq_rules_by_stream(self, events, offsets):
        """pm_hip_seq_rules_by_stream: host arrays through the device call:
        (rule_ptr int64 of nseg + 1, hits u64), stream j's hits
        hits[ptr[j]:ptr[j+1]] ascending, each position << 24 | rule with the
        position at which the stream's prefix first satisfied the rule's
        positive part (unpack_events splits them)."""
        ev, offs, _, ptr = _by_stream_host_args(events, offsets, 0)
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
        hits = np.empty(max(len(ev), 1), dtype=np.uint64)
        for _ in range(2):  # the hits are not bounded by the events: rule_ptr[-1] sizes the retry
            rc = self.lib.pm_hip_seq_rules_by_stream(self.obj, ev.ctypes.data_as(u64p), len(ev),
                                                     offs.ctypes.data_as(i64p), offs.size - 1,
                                                     hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p))
            self._check(rc)
            if len(hits) >= ptr[-1]:
                break
            hits = np.empty(int(ptr[-1]), dtype=np.uint64)
        return ptr, hits[:int(ptr[-1])]

    def read_many_seq_rules(self, buffers):
        """One all-matches batch list call over a list of bytes-like streams at
        seq_rules_min_len(), then seq_rules_by_stream: per stream, in order,
        (positions inside the stream, rule indices) of the ordered rules that
        fire in it, ascending by position."""
        data, offs = _concat(buffers)
        ev, _ = self._read_events(data, offs, None, self.seq_rules_min_len(), all_matches=True)
        ptr, hits = self.seq_rules_by_stream(ev, offs)
        pos, rule = unpack_events(hits)
        return [(pos[ptr[j]:ptr[j + 1]] - offs[j], rule[ptr[j]:ptr[j + 1]]) for j in range(len(buffers))]

    # --- flow rules: rules over a set per flow, carried from call to call ------
    def set_flow_rules(self, rules, fast=None):
        """pm_hip_set_flow_rules: a rule set of its own for flow_rules(), in
        set_rules' form (set_rules and its rules are not touched).  fast[r]
        only decides which term of rule r is tested first.  After compile(); a
        later call replaces the set (no flow-rules call may be in flight), and
        with it the bits and possibly the words of a flow's set."""
        ptr, terms = pack_rules(rules, fast)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self.lib.pm_hip_set_flow_rules(self.obj, ptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                                   len(ptr) - 1))

    def flow_rule_count(self):
        """pm_hip_flow_rule_count: the flow rules set (0 before set_flow_rules)."""
        return int(self.lib.pm_hip_flow_rule_count(self.obj))

    def flow_rules_min_len(self):
        """pm_hip_flow_rules_min_len: the length of the shortest pattern any
        term names: the largest min_len a scan may use for exact hits (0
        before set_flow_rules)."""
        return int(self.lib.pm_hip_flow_rules_min_len(self.obj))

    @property
    def flow_rule_words(self):
        """pm_hip_flow_rule_words: W, the u64 words of one flow's set (0
        before set_flow_rules)."""
        return int(self.lib.pm_hip_flow_rule_words(self.obj))

    def flow_rule_bit(self, gid):
        """pm_hip_flow_rule_bit: the bit of gid in a flow's set (word bit >>
        6, bit bit & 63), or -1 where no term names it."""
        return int(self.lib.pm_hip_flow_rule_bit(self.obj, int(gid)))

    def flow_rules_scratch_bytes(self, cap, nseg):
        """pm_hip_flow_rules_scratch_bytes: the device scratch, in bytes, that
        flow_rules_device needs for a list of cap slots over nseg streams."""
        b = self.lib.pm_hip_flow_rules_scratch_bytes(cap, nseg)
        if b == ctypes.c_size_t(-1).value:
            raise ValueError("flow_rules_scratch_bytes: cap <= 2^40, 0 <= nseg < 2^31")
        return b

    def flow_rules_device(self, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg, d_sets_ptr, nrows, d_rows_ptr,
                          flags, d_hits_ptr, hits_cap, d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr):
        """pm_hip_flow_rules_device: behind a flow scan's list (the arguments
        of rules_by_stream_device), the flow rules whose conjunction became
        true in this call's bytes, given the terms each flow carries in its
        row of the nrows x flow_rule_words u64 at d_sets_ptr (d_rows_ptr:
        nseg int64 row indices, or None for row j); then this call's terms
        are OR-ed into the rows, unless flags holds FLOW_RULES_KEEP.
        Enqueued on stream_ptr, no synchronize."""
        rc = self.lib.pm_hip_flow_rules_device(self.obj, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg,
                                               d_sets_ptr, nrows, d_rows_ptr, flags, d_hits_ptr, hits_cap,
                                               d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr)
        self._check(rc)

    def flow_rules(self, events, offsets, sets, rows=None, keep=False):
        """pm_hip_flow_rules: host arrays through the device call: (rule_ptr
        int64 of nseg + 1, hits u64), stream j's hits hits[ptr[j]:ptr[j+1]]
        ascending, each position << 24 | rule.  sets is a C-contiguous
        (nrows, flow_rule_words) u64 array, a row per flow, updated in place
        unless keep; rows[j] is the row of stream j (None: row j).  events
        come from an all-matches flow scan that continued the same flows, at
        a min_len <= flow_rules_min_len(), with a cap that held the list."""
        ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
        offs, sets, rows, ptr = _flow_rules_host_args(offsets, sets, rows)
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
        if self.flow_rule_words and sets.shape[1] != self.flow_rule_words:  # (0: the call says what is missing)
            raise ValueError(f"sets: {self.flow_rule_words} words per row, not {sets.shape[1]}")

        def call(flags, hits):
            self._check(self.lib.pm_hip_flow_rules(self.obj, ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p),
                                                   offs.size - 1, sets.ctypes.data_as(u64p), sets.shape[0],
                                                   None if rows is None else rows.ctypes.data_as(i64p), flags,
                                                   hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p)))
        # the hits are not bounded by the events and a committing call cannot be repeated: count them first
        call(FLOW_RULES_KEEP, np.empty(0, dtype=np.uint64))
        hits = np.empty(int(ptr[-1]), dtype=np.uint64)
        call(FLOW_RULES_KEEP if keep else 0, hits)
        return ptr, hits[:int(ptr[-1])]

    # --- flow ordered rules: each chain's progress per flow, carried from call to call ---
    def set_flow_seq_rules(self, rules, fast=None):
        """pm_hip_set_flow_seq_rules: a rule set of its own for
        flow_seq_rules(), in pack_seq_rules' term forms (the other three rule
        sets are not touched).  A term with a within raises ValueError: a
        bound across packets is out of scope.  fast is accepted and has no
        effect on the results.  After compile(); a later call replaces the
        set, and with it the layout of a flow's row."""
        ptr, terms, gaps = _packed_flow_seq(rules, fast)
        u32p = ctypes.POINTER(ctypes.c_uint32)
        self._check(self.lib.pm_hip_set_flow_seq_rules(self.obj, ptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                                       gaps.ctypes.data_as(u32p), len(ptr) - 1))

    def flow_seq_rule_count(self):
        """pm_hip_flow_seq_rule_count: the rules set (0 before set_flow_seq_rules)."""
        return int(self.lib.pm_hip_flow_seq_rule_count(self.obj))

    def flow_seq_rules_min_len(self):
        """pm_hip_flow_seq_rules_min_len: the length of the shortest pattern
        any term names (0 before set_flow_seq_rules)."""
        return int(self.lib.pm_hip_flow_seq_rules_min_len(self.obj))

    @property
    def flow_seq_rule_words(self):
        """pm_hip_flow_seq_rule_words: S, the u64 words of one flow's
        progress row (0 before set_flow_seq_rules)."""
        return int(self.lib.pm_hip_flow_seq_rule_words(self.obj))

    def flow_seq_chain_count(self):
        """pm_hip_flow_seq_chain_count: C, the chains of two or more positive
        terms: the chain words at the front of a row."""
        return int(self.lib.pm_hip_flow_seq_chain_count(self.obj))

    def flow_seq_chain_word(self, rule, term_index):
        """pm_hip_flow_seq_chain_word: the word of the chain headed by term
        term_index of rule, as the rule was given, or -1."""
        return int(self.lib.pm_hip_flow_seq_chain_word(self.obj, int(rule), int(term_index)))

    def flow_seq_rule_bit(self, gid):
        """pm_hip_flow_seq_rule_bit: the bit of gid (in word C + bit // 64, at
        bit % 64), or -1 where it has none."""
        return int(self.lib.pm_hip_flow_seq_rule_bit(self.obj, int(gid)))

    def flow_seq_rules_scratch_bytes(self, cap, nseg):
        """pm_hip_flow_seq_rules_scratch_bytes: the device scratch, in bytes,
        that flow_seq_rules_device needs for a list of cap slots over nseg
        streams."""
        b = self.lib.pm_hip_flow_seq_rules_scratch_bytes(cap, nseg)
        if b == ctypes.c_size_t(-1).value:
            raise ValueError("flow_seq_rules_scratch_bytes: cap <= 2^40, 0 <= nseg < 2^31")
        return b

    def flow_seq_rules_device(self, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg, d_prog_ptr, nrows,
                              d_rows_ptr, d_pos_in_ptr, flags, d_hits_ptr, hits_cap, d_rule_ptr_ptr, d_scratch_ptr,
                              scratch_bytes, stream_ptr):
        """pm_hip_flow_seq_rules_device: behind a flow scan's list (the
        arguments of flow_rules_device), the ordered rules that became true
        in this call's bytes, given each flow's row of the nrows x
        flow_seq_rule_words u64 at d_prog_ptr and the nseg u64 byte counts at
        d_pos_in_ptr that the flows had before the call; then the rows are
        advanced, unless flags holds FLOW_RULES_KEEP.  Enqueued on
        stream_ptr, no synchronize."""
        rc = self.lib.pm_hip_flow_seq_rules_device(self.obj, d_events_ptr, cap, d_nevents_ptr, d_offsets_ptr, nseg,
                                                   d_prog_ptr, nrows, d_rows_ptr, d_pos_in_ptr, flags, d_hits_ptr,
                                                   hits_cap, d_rule_ptr_ptr, d_scratch_ptr, scratch_bytes, stream_ptr)
        self._check(rc)

    def flow_seq_rules(self, events, offsets, prog, pos_in, rows=None, keep=False):
        """pm_hip_flow_seq_rules: host arrays through the device call:
        (rule_ptr int64 of nseg + 1, hits u64), stream j's hits
        hits[ptr[j]:ptr[j+1]] ascending, each position << 24 | rule.  prog is
        a C-contiguous (nrows, flow_seq_rule_words) u64 array, a row per flow,
        updated in place unless keep; pos_in[j] the bytes flow j had before
        the call; rows[j] the row of stream j (None: row j).  events come from
        an all-matches flow scan that continued the same flows, at a min_len
        <= flow_seq_rules_min_len(), with a cap that held the list."""
        ev = np.ascontiguousarray(events, dtype=np.uint64).ravel()
        offs, prog, rows, pos_in, ptr = _flow_seq_host_args(offsets, prog, rows, pos_in)
        u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
        S = self.flow_seq_rule_words
        if S and prog.shape[1] != S:  # (0: the call says what is missing)
            raise ValueError(f"prog: {S} words per row, not {prog.shape[1]}")

        def call(flags, hits):
            self._check(self.lib.pm_hip_flow_seq_rules(
                self.obj, ev.ctypes.data_as(u64p), len(ev), offs.ctypes.data_as(i64p), offs.size - 1,
                prog.ctypes.data_as(u64p), prog.shape[0], None if rows is None else rows.ctypes.data_as(i64p),
                pos_in.ctypes.data_as(u64p), flags, hits.ctypes.data_as(u64p), len(hits), ptr.ctypes.data_as(i64p)))
        # the hits are not bounded by the events and a committing call cannot be repeated: count them first
        call(FLOW_RULES_KEEP, np.empty(0, dtype=np.uint64))
        hits = np.empty(int(ptr[-1]), dtype=np.uint64)
        call(FLOW_RULES_KEEP if keep else 0, hits)
        return ptr, hits[:int(ptr[-1])]

    # --- pattern groups: a group mask per pattern and one per stream --------
    def set_groups(self, masks):
        """pm_hip_set_groups: masks[k] is the u32 group mask (bit g = member
        of group g) of the k-th pattern added -- a dictionary's patterns in
        its own order.  After compile(); a later call replaces the masks
        (no group scan may be in flight)."""
        g = np.ascontiguousarray(masks, dtype=np.uint32)
        if g.ndim != 1:
            raise ValueError("masks: one u32 per pattern added")
        rc = self.lib.pm_hip_set_groups(self.obj, g.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), g.size)
        self._check(rc)

    def pattern_groups(self, gid):
        """The group mask of pattern gid (0 out of range or before set_groups)."""
        return int(self.lib.pm_hip_pattern_groups(self.obj, gid))

    def scan_batch_groups_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_stream_groups_ptr, min_len, all_matches,
                                 d_events_ptr, cap, d_nevents_ptr, stream_ptr):
        """pm_hip_scan_batch_groups_device: scan_batch_matches_device with the
        patterns visible to each stream only (groups & d_stream_groups[j]; a
        null pointer: every stream on all groups).  all_matches false: the
        longest visible pattern per position, the answer of a matcher
        compiled from the visible patterns alone."""
        rc = self.lib.pm_hip_scan_batch_groups_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n,
                                                      d_stream_groups_ptr, min_len, int(bool(all_matches)),
                                                      d_events_ptr, cap, d_nevents_ptr, stream_ptr)
        self._check(rc)

    def scan_flows_groups_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr,
                                 d_stream_groups_ptr, min_len, all_matches, d_events_ptr, cap, d_nevents_ptr,
                                 stream_ptr):
        """pm_hip_scan_flows_groups_device: scan_flows_matches_device with the
        list of scan_batch_groups_device; the states do not depend on the
        masks."""
        rc = self.lib.pm_hip_scan_flows_groups_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr,
                                                      d_state_out_ptr, d_stream_groups_ptr, min_len,
                                                      int(bool(all_matches)), d_events_ptr, cap, d_nevents_ptr,
                                                      stream_ptr)
        self._check(rc)

    def read_batch_groups(self, data, offsets, stream_groups, min_len=3, all_matches=True):
        """pm_hip_read_batch_groups: read_batch_matches with the patterns
        visible to each stream only (stream_groups: nseg u32 masks):
        (positions int64, codes), ascending by position, then gid."""
        ev, _ = self._read_events(data, offsets, None, min_len, all_matches, stream_groups)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids]

    def read_many_groups(self, buffers, stream_groups, min_len=3, all_matches=True):
        """read_many_matches with a group mask per buffer."""
        data, offs = _concat(buffers)
        pos, codes = self.read_batch_groups(data, offs, stream_groups, min_len, all_matches)
        return _split_events(pos, codes, offs)

    def read_flows_groups(self, data, offsets, stream_groups, state=None, min_len=3, all_matches=True):
        """pm_hip_read_flows_groups: read_flows_matches with the patterns
        visible to each stream only: (positions, codes, state_out)."""
        nseg = len(offsets) - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        ev, st = self._read_events(data, offsets, st, min_len, all_matches, stream_groups)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids], st

    # --- pattern windows: where in its stream a pattern may lie --------------
    def set_windows(self, min_start, max_end):
        """pm_hip_set_windows: min_start[k] / max_end[k] (Snort's offset and
        offset + depth; 0xFFFFFFFF = unbounded) of the k-th pattern added.
        After compile(); a later call replaces the windows (no window scan
        may be in flight)."""
        lo = np.ascontiguousarray(min_start, dtype=np.uint32)
        hi = np.ascontiguousarray(max_end, dtype=np.uint32)
        if lo.ndim != 1 or hi.shape != lo.shape:
            raise ValueError("min_start, max_end: one u32 each per pattern added")
        u32p = ctypes.POINTER(ctypes.c_uint32)
        rc = self.lib.pm_hip_set_windows(self.obj, lo.ctypes.data_as(u32p), hi.ctypes.data_as(u32p), lo.size)
        self._check(rc)

    def pattern_window(self, gid):
        """(min_start, max_end) of pattern gid; None out of range or before
        set_windows."""
        lo, hi = ctypes.c_uint32(0), ctypes.c_uint32(0)
        if self.lib.pm_hip_pattern_window(self.obj, gid, ctypes.byref(lo), ctypes.byref(hi)) != 0:
            return None
        return int(lo.value), int(hi.value)

    def scan_batch_windows_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_stream_groups_ptr, min_len, all_matches,
                                  d_events_ptr, cap, d_nevents_ptr, stream_ptr):
        """pm_hip_scan_batch_windows_device: scan_batch_groups_device with a
        pattern visible only where it also passes its window, counted from
        its stream's first byte.  Without set_groups every pattern is in
        every group and d_stream_groups_ptr must be null."""
        rc = self.lib.pm_hip_scan_batch_windows_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n,
                                                       d_stream_groups_ptr, min_len, int(bool(all_matches)),
                                                       d_events_ptr, cap, d_nevents_ptr, stream_ptr)
        self._check(rc)

    def scan_flows_windows_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr,
                                  d_stream_groups_ptr, min_len, all_matches, d_events_ptr, cap, d_nevents_ptr,
                                  stream_ptr, d_pos_in_ptr=None, d_pos_out_ptr=None):
        """pm_hip_scan_flows_windows_device: scan_flows_groups_device with the
        windows counted from each flow's own first byte: d_pos_in_ptr holds
        the bytes every flow had before this call (u64, null = 0),
        d_pos_out_ptr receives them after it (null = not wanted)."""
        rc = self.lib.pm_hip_scan_flows_windows_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr,
                                                       d_state_out_ptr, d_stream_groups_ptr, min_len,
                                                       int(bool(all_matches)), d_events_ptr, cap, d_nevents_ptr,
                                                       stream_ptr, d_pos_in_ptr, d_pos_out_ptr)
        self._check(rc)

    def read_batch_windows(self, data, offsets, stream_groups=None, min_len=3, all_matches=True):
        """pm_hip_read_batch_windows: read_batch_groups with the patterns'
        windows applied (stream_groups None: every stream on all groups):
        (positions int64, codes), ascending by position, then gid."""
        ev = self._read_list("windows", data, offsets, min_len, all_matches, stream_groups)[0]
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids]

    def read_many_windows(self, buffers, stream_groups=None, min_len=3, all_matches=True):
        """read_many_groups with the patterns' windows applied, each buffer a
        stream of its own."""
        data, offs = _concat(buffers)
        pos, codes = self.read_batch_windows(data, offs, stream_groups, min_len, all_matches)
        return _split_events(pos, codes, offs)

    def read_flows_windows(self, data, offsets, stream_groups=None, state=None, pos=None, min_len=3,
                           all_matches=True):
        """pm_hip_read_flows_windows: read_flows_groups with the patterns'
        windows applied at pos[j] + (the byte's place in its packet): pos is
        the bytes every flow had before this call (None: 0).  Returns
        (positions, codes, state_out, pos_out)."""
        nseg = len(offsets) - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        ps = np.zeros(nseg, dtype=np.uint64) if pos is None else np.array(pos, dtype=np.uint64, order="C")
        ev, st, ps, _ = self._read_list("windows", data, offsets, min_len, all_matches, stream_groups, st, ps)
        p, gids = unpack_events(ev)
        return p, self._codes[gids], st, ps

    # --- per-pattern nocase: case-insensitive patterns in the list scans -----
    def set_nocase(self, flags):
        """pm_hip_set_nocase: flags[k] != 0 makes the k-th pattern added
        case-insensitive (ASCII).  After compile(); builds and uploads the
        folded images; a later call rebuilds them (no nocase scan may be in
        flight)."""
        f = np.ascontiguousarray(np.asarray(flags) != 0, dtype=np.uint8)
        if f.ndim != 1:
            raise ValueError("flags: one value per pattern added")
        rc = self.lib.pm_hip_set_nocase(self.obj, f.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), f.size)
        self._check(rc)

    def pattern_nocase(self, gid):
        """The nocase flag of pattern gid (bool); None out of range or before
        set_nocase."""
        rc = self.lib.pm_hip_pattern_nocase(self.obj, gid)
        return None if rc < 0 else bool(rc)

    @property
    def nocase_flow_states(self):
        """States of the folded automaton: the nocase flow scans' states are
        its own, below this value (0 before set_nocase or without a DFA)."""
        return int(self.lib.pm_hip_nocase_flow_states(self.obj))

    @property
    def case_words(self):
        """W: the u64 words of case history a flow carries through the
        nocase flow scans (0: none needed)."""
        return int(self.lib.pm_hip_case_words(self.obj))

    def nocase_stats(self):
        """(build ms, upload ms, table bytes) of the last set_nocase; None
        before it."""
        b, u, t = ctypes.c_double(0), ctypes.c_double(0), ctypes.c_size_t(0)
        if self.lib.pm_hip_nocase_stats(self.obj, ctypes.byref(b), ctypes.byref(u), ctypes.byref(t)) != 0:
            return None
        return b.value, u.value, int(t.value)

    def scan_batch_nocase_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_stream_groups_ptr, min_len, all_matches,
                                 d_events_ptr, cap, d_nevents_ptr, stream_ptr):
        """pm_hip_scan_batch_nocase_device: scan_batch_windows_device with the
        patterns' nocase flags honoured; group and window tables are used
        where the object has them."""
        rc = self.lib.pm_hip_scan_batch_nocase_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n,
                                                      d_stream_groups_ptr, min_len, int(bool(all_matches)),
                                                      d_events_ptr, cap, d_nevents_ptr, stream_ptr)
        self._check(rc)

    def scan_flows_nocase_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr,
                                 d_stream_groups_ptr, min_len, all_matches, d_events_ptr, cap, d_nevents_ptr,
                                 stream_ptr, d_pos_in_ptr=None, d_pos_out_ptr=None, d_case_in_ptr=None,
                                 d_case_out_ptr=None):
        """pm_hip_scan_flows_nocase_device: scan_flows_windows_device over the
        folded automaton (states below nocase_flow_states) with nseg *
        case_words u64 of case history in and out per call."""
        rc = self.lib.pm_hip_scan_flows_nocase_device(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr,
                                                      d_state_out_ptr, d_stream_groups_ptr, min_len,
                                                      int(bool(all_matches)), d_events_ptr, cap, d_nevents_ptr,
                                                      stream_ptr, d_pos_in_ptr, d_pos_out_ptr, d_case_in_ptr,
                                                      d_case_out_ptr)
        self._check(rc)

    def _read_nocase(self, data, offsets, stream_groups, state, pos, case, min_len, all_matches):
        """_read_list for the nocase forms: (events u64 ascending, state_out,
        pos_out, case_out -- None for the batched form)."""
        return self._read_list("nocase", data, offsets, min_len, all_matches, stream_groups, state, pos, case)

    def read_batch_nocase(self, data, offsets, stream_groups=None, min_len=3, all_matches=True):
        """pm_hip_read_batch_nocase: read_batch_windows with the patterns'
        nocase flags honoured (groups and windows where they are set):
        (positions int64, codes), ascending by position, then gid."""
        ev, _, _, _ = self._read_nocase(data, offsets, stream_groups, None, None, None, min_len, all_matches)
        pos, gids = unpack_events(ev)
        return pos, self._codes[gids]

    def read_many_nocase(self, buffers, stream_groups=None, min_len=3, all_matches=True):
        """read_batch_nocase over a list of buffers, each a stream of its own:
        per buffer (positions inside it, codes)."""
        data, offs = _concat(buffers)
        pos, codes = self.read_batch_nocase(data, offs, stream_groups, min_len, all_matches)
        return _split_events(pos, codes, offs)

    def read_flows_nocase(self, data, offsets, stream_groups=None, state=None, pos=None, case=None, min_len=3,
                          all_matches=True):
        """pm_hip_read_flows_nocase: read_flows_windows over the folded
        automaton.  state: the folded automaton's states (None: fresh);
        pos: the bytes every flow had before (None: 0; used where windows are
        set); case: (nseg, case_words) u64 of case history (None: zero).
        Returns (positions, codes, state_out, pos_out, case_out); pos_out
        counts the bytes whether or not windows are set."""
        nseg = len(offsets) - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        ps = np.zeros(nseg, dtype=np.uint64) if pos is None else np.array(pos, dtype=np.uint64, order="C")
        cs = (np.zeros((nseg, self.case_words), dtype=np.uint64) if case is None
              else np.array(case, dtype=np.uint64, order="C").reshape(nseg, self.case_words))
        ev, st, ps2, cs = self._read_nocase(data, offsets, stream_groups, st, ps, cs, min_len, all_matches)
        p, gids = unpack_events(ev)
        ps = ps + np.diff(np.asarray(offsets, dtype=np.int64)).astype(np.uint64)
        return p, self._codes[gids], st, ps, cs

    # --- flow scan: the batched layout with a carried state per stream -----
    def scan_flows_device(self, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr, d_out_ptr,
                          d_count_ptr, stream_ptr, out_width=4):
        """pm_hip_scan_flows_device / _device16: scan_batch_device's layout,
        but stream j starts in the state d_state_in[j] (u32 on the device;
        None = every stream fresh) and leaves the state after its last byte
        in d_state_out[j] (None = not wanted).  The two arrays must differ.
        ac / auto kinds."""
        fn = {4: self.lib.pm_hip_scan_flows_device, 2: self.lib.pm_hip_scan_flows_device16}[out_width]
        rc = fn(self.obj, d_text_ptr, d_offsets_ptr, nseg, n, d_state_in_ptr, d_state_out_ptr, d_out_ptr, d_count_ptr,
                stream_ptr)
        self._check(rc)

    def read_flows_gids(self, data, offsets, state=None):
        """pm_hip_read_flows_gid: (gids, state_out).  Stream j = data[offsets[j]:
        offsets[j+1]] continues the flow whose state is state[j] (a u32 array
        of nseg values this object returned earlier, 0 = a fresh flow; None =
        all fresh); state_out is always a new array, to hand back with the
        flows' next packets.  A flow appears at most once per call."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or int(offs[-1]) != len(arr):
            raise ValueError("offsets: nseg + 1 values, the last one len(data)")
        nseg = offs.size - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        if st.shape != (nseg,):
            raise ValueError("state: nseg values")
        out = np.empty(len(arr), dtype=np.uint32)
        rc = self.lib.pm_hip_read_flows_gid(self.obj, arr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                            offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nseg,
                                            st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                            out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        self._check(rc)
        return out, st

    def read_flows_codes(self, data, offsets, state=None):
        """(codes, state_out): (file << 24 | line) per position, like
        read_block_codes, and the flows' states."""
        gids, st = self.read_flows_gids(data, offsets, state)
        return self._codes[gids], st

    def read_flows_id_array(self, data, offsets, state=None):
        """pm_hip_read_flows: (the add_pattern id per position (uintp),
        state_out)."""
        arr = np.ascontiguousarray(np.frombuffer(bytes(data), dtype=np.uint8) if not isinstance(data, np.ndarray)
                                   else data, dtype=np.uint8)
        offs = np.ascontiguousarray(offsets, dtype=np.int64)
        if offs.ndim != 1 or offs.size < 1 or int(offs[-1]) != len(arr):
            raise ValueError("offsets: nseg + 1 values, the last one len(data)")
        nseg = offs.size - 1
        st = np.zeros(nseg, dtype=np.uint32) if state is None else np.array(state, dtype=np.uint32, order="C")
        if st.shape != (nseg,):
            raise ValueError("state: nseg values")
        out = np.empty(max(len(arr), 1), dtype=np.uintp)
        rc = self.lib.pm_hip_read_flows(self.obj, arr.ctypes.data_as(ctypes.c_char_p),
                                        offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), nseg,
                                        st.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                        out.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)))
        self._check(rc)
        return out[:len(arr)], st

    @property
    def flow_states(self):
        """pm_hip_flow_states: valid flow states are 0 .. this - 1 (0 for an
        object without a DFA image)."""
        return self.lib.pm_hip_flow_states(self.obj)

    def gen_lines_device(self, d_dst_ptr, n, seed, stream_ptr):
        """pm_hip_gen_lines_device: the lines stream (random dictionary
        patterns back to back, '\\n' after each) of this object's patterns."""
        rc = self.lib.pm_hip_gen_lines_device(self.obj, d_dst_ptr, n, seed, stream_ptr)
        self._check(rc)

    def gen_lines(self, n, seed) -> np.ndarray:
        """The same bytes on the host (pm_gen_lines_host)."""
        buf = np.empty(n, np.uint8)
        self.lib.pm_gen_lines_host(self.obj, buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), n, seed)
        return buf

    def score_device(self, d_algo_ptr, d_real_ptr, n, d_counts_ptr, stream_ptr):
        """pm_hip_score_device: d_counts (5 u64) += success, partial,
        false_neg, false_pos, all_matches of algo ids against real ids."""
        rc = self.lib.pm_hip_score_device(self.obj, d_algo_ptr, d_real_ptr, n, d_counts_ptr, stream_ptr)
        self._check(rc)

    def pattern_counts_device(self, d_ids_ptr, n, d_hist_ptr, stream_ptr):
        """pm_hip_pattern_counts_device: d_hist (u64[n_patterns + 1], by gid)
        += occurrences of every pattern (suffix chains of the dense ids)."""
        rc = self.lib.pm_hip_pattern_counts_device(self.obj, d_ids_ptr, n, d_hist_ptr, stream_ptr)
        self._check(rc)

    def hold_choice(self, launches):
        """pm_hip_hold_choice: keep the picked kernel for `launches` more
        scan_device launches (1 RT, 2 AC dense rows, 3 AC rows + records;
        0 = nothing to pick; -1 = still measuring)."""
        return self.lib.pm_hip_hold_choice(self.obj, launches)

    def prepare_capture(self):
        """pm_hip_prepare_capture: the scratch captured scan_device launches
        need, allocated before any stream capture begins."""
        if self.lib.pm_hip_prepare_capture(self.obj) != 0:
            raise RuntimeError(self.lib.pm_hip_last_error().decode())

    @property
    def scratch_bytes(self):
        return self.lib.pm_hip_scratch_bytes(self.obj)

    def parent_gid(self, gid):
        return self.lib.pm_hip_parent_gid(self.obj, gid)

    @property
    def kernel_kind(self):
        return self.lib.pm_hip_kernel_kind(self.obj)

    @property
    def dfa_form_last(self):
        """1 = dense rows, 2 = rows + records (pm_flatten.h), 0 = RT ran."""
        return self.lib.pm_hip_dfa_form_last(self.obj)

    @property
    def sparse_kernel_last(self):
        """The sparse form's kernel of the last launch that ran it
        ("sparse_kernel" numbering, 0 before any)."""
        return self.lib.pm_hip_sparse_kernel_last(self.obj)

    @property
    def kernel_last(self):
        """Kernel of the last launch: 1 = reverse trie, 2 = AC DFA."""
        return self.lib.pm_hip_kernel_last(self.obj)

    @property
    def max_pattern_len(self):
        return self.lib.pm_hip_max_pattern_len(self.obj)

    @property
    def table_bytes(self):
        return self.lib.pm_hip_table_bytes(self.obj)

    @property
    def device_seconds(self):
        """Device seconds of read_block's scans since reset(), or None when
        some of them were untimed (small calls with the "host_events" option
        off, its default: pm_hip_device_seconds returns -1)."""
        v = self.lib.pm_hip_device_seconds(self.obj)
        return None if v < 0 else v

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass
