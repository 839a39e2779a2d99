"""The host twin of the nocase scans (pm_hip.h, "nocase"):
pm_flat_build_nocase / pm_flat_host_scan_nocase against the tests' own brute
force (nocase_inputs.brute), batched on the reverse-trie image and as flows on
the DFA image, with the hand-built classes, the flow seams and the history
words.  CPU only."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from nocase_inputs import (HAND, HAND_TEXTS, INF, batch_events, brute, call_events, f_call, family_dictionary, flag_of,
                           flip_case, fold, fuzz_dictionary, fuzz_text, group_of, history_words, input_f_flipped,
                           input_t_flipped, real_dictionary, stream_groups, stream_offsets, window_of)

U8P = ctypes.POINTER(ctypes.c_uint8)
U32P = ctypes.POINTER(ctypes.c_uint32)
U64P = ctypes.POINTER(ctypes.c_uint64)
I64P = ctypes.POINTER(ctypes.c_int64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


class Twin:
    """pm_flat_build_nocase over a pattern list, and one scan call."""

    def __init__(self, pats, flags, kind):
        self.lib = pm.load()
        n = len(pats)
        arr = (ctypes.c_char_p * n)(*pats)
        lens = (ctypes.c_uint32 * n)(*[len(p) for p in pats])
        fl = np.asarray(flags, dtype=np.uint8)
        self.h = self.lib.pm_flat_build_nocase(arr, lens, _p(fl, U8P), n, kind, None)
        assert self.h
        self.kind = kind
        iog = self.array("index_of_gid")
        self.gid_of_index = np.zeros(n, dtype=np.int64)
        self.gid_of_index[iog[1:]] = np.arange(1, len(iog))
        self.info = self.array("nc_info")
        self.W = int(self.info[1])

    def array(self, name):
        data, es = ctypes.c_void_p(), ctypes.c_size_t()
        n = self.lib.pm_flat_array(self.h, name.encode(), ctypes.byref(data), ctypes.byref(es))
        if n == 0:
            return np.zeros(0, np.uint32)
        dt = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[es.value]
        buf = (ctypes.c_char * (n * es.value)).from_address(data.value)
        return np.frombuffer(buf, dtype=dt).copy()

    def scan(self, text, offs, state=None, pos=None, case=None, sgroups=None, groups=None, windows=None, min_len=1,
             all_matches=True, cap=None):
        text = np.ascontiguousarray(text, dtype=np.uint8)
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        nseg = len(offs) - 1
        cap = 16 * len(text) + 64 if cap is None else cap
        ev = np.zeros(cap, dtype=np.uint64)
        total = ctypes.c_size_t(0)
        st_out = np.zeros(nseg, np.uint32)
        pos_out = np.zeros(nseg, np.uint64)
        case_out = np.zeros((nseg, self.W), np.uint64)
        lo, hi = (None, None) if windows is None else windows
        rc = self.lib.pm_flat_host_scan_nocase(
            self.h, _p(text, U8P), _p(offs, I64P), nseg, _p(state, U32P), _p(st_out, U32P), _p(pos, U64P),
            _p(pos_out, U64P), _p(case, U64P) if self.W else None, _p(case_out, U64P) if self.W else None,
            _p(sgroups, U32P), _p(groups, U32P), _p(lo, U32P), _p(hi, U32P), min_len, int(all_matches), _p(ev, U64P),
            cap, ctypes.byref(total))
        assert rc == 0, rc
        assert total.value <= cap
        return ev[:total.value], st_out, pos_out, case_out

    def __del__(self):
        if getattr(self, "h", None):
            self.lib.pm_flat_free(self.h)


def tables_of(pats):
    groups = np.array([group_of(p) for p in pats], dtype=np.uint32)
    w = [window_of(p) for p in pats]
    return groups, (np.array([a for a, _ in w], np.uint32), np.array([b for _, b in w], np.uint32))


def streams_of(text, offs):
    return [bytes(text[offs[j]:offs[j + 1]]) for j in range(len(offs) - 1)]


CONFIGS = [(ml, am, g, w) for ml in (1, 3, 5) for am in (True, False) for g, w in ((False, False), (True, True))]
CONFIGS += [(3, True, True, False), (3, False, False, True)]


@pytest.mark.parametrize("seed", [0, 1])
def test_batched_twin_against_brute_force(seed):
    pats = fuzz_dictionary(seed)
    flags = [flag_of(p) for p in pats]
    tw = Twin(pats, flags, pm.KIND_RT)
    text = fuzz_text(pats, seed, 12288)
    offs = stream_offsets(len(text), seed)
    streams = streams_of(text, offs)
    groups, windows = tables_of(pats)
    sg = stream_groups(len(offs) - 1)
    seen_nc = seen_rej = 0
    for min_len, all_matches, g, w in CONFIGS:
        rows, stats = brute(pats, flags, streams, tw.gid_of_index, min_len, groups if g else None, sg if g else None,
                            windows if w else None, all_matches)
        got = tw.scan(text, offs, sgroups=sg if g else None, groups=groups if g else None,
                      windows=windows if w else None, min_len=min_len, all_matches=all_matches)[0]
        want = batch_events(rows, offs)
        assert len(want) > 0
        assert np.array_equal(got, want), (min_len, all_matches, g, w)
        seen_nc += stats["nocase_case_differs"]
        seen_rej += stats["rejected"]
    assert seen_nc > 0 and seen_rej > 0, "the text must differ in case from nocase patterns and reject exact ones"


@pytest.mark.parametrize("seed", [0, 1])
def test_flow_twin_against_brute_force(seed):
    pats = fuzz_dictionary(seed)
    flags = [flag_of(p) for p in pats]
    tw = Twin(pats, flags, pm.KIND_AC)
    assert tw.W == 3  # the 150-byte case-sensitive pattern: ceil(149 / 64)
    A, B = fuzz_text(pats, seed, 12288), fuzz_text(pats, seed + 50, 12288)
    offs = stream_offsets(len(A), seed)
    nseg = len(offs) - 1
    whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
    groups, windows = tables_of(pats)
    sg = stream_groups(nseg)
    lens = np.diff(offs)
    before_b = lens.astype(np.int64)
    seen_straddle = seen_rej = seen_nc = 0
    for min_len, all_matches, g, w in CONFIGS:
        rows, stats = brute(pats, flags, whole, tw.gid_of_index, min_len, groups if g else None, sg if g else None,
                            windows if w else None, all_matches)
        kw = dict(sgroups=sg if g else None, groups=groups if g else None, windows=windows if w else None,
                  min_len=min_len, all_matches=all_matches)
        ev_a, st, pos, case = tw.scan(A, offs, **kw)
        want_a, _ = call_events(rows, offs, np.zeros(nseg, np.int64))
        assert np.array_equal(ev_a, want_a), ("A", min_len, all_matches, g, w)
        assert np.array_equal(pos, lens.astype(np.uint64))
        for j in (0, 1, 3, 10, nseg - 1):
            assert np.array_equal(case[j], history_words(A[offs[j]:offs[j + 1]], tw.W)), j
        ev_b, st2, pos2, case2 = tw.scan(B, offs, state=st, pos=pos, case=case, **kw)
        want_b, straddle = call_events(rows, offs, before_b)
        assert np.array_equal(ev_b, want_b), ("B", min_len, all_matches, g, w)
        for j in (0, 1, 3, 10, nseg - 1):
            assert np.array_equal(case2[j], history_words(whole[j], tw.W)), j
        seen_straddle += straddle
        seen_rej += stats["rejected"]
        seen_nc += stats["nocase_case_differs"]
    assert seen_straddle > 0 and seen_rej > 0 and seen_nc > 0


FAMILY_CONFIGS = [(1, True, False), (3, False, True), (5, True, True), (1, False, False)]


@pytest.mark.parametrize("name", ["no_short", "only_short", "many", "unary"])
def test_families_batched_and_flow_twin(name):
    """fuzz_inputs' four families over letters of both cases: batched over A, as
    flows over A then B."""
    pats = family_dictionary(name)
    flags = [flag_of(p) for p in pats]
    A, B = fuzz_text(pats, 7, 8192), fuzz_text(pats, 57, 8192)
    offs = stream_offsets(len(A), 7)
    nseg = len(offs) - 1
    lens = np.diff(offs)
    groups, windows = tables_of(pats)
    sg = stream_groups(nseg)
    rt, ac = Twin(pats, flags, pm.KIND_RT), Twin(pats, flags, pm.KIND_AC)
    assert np.array_equal(rt.gid_of_index, ac.gid_of_index)
    whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
    seen = 0
    for min_len, all_matches, tables in FAMILY_CONFIGS:
        g, s, w = (groups, sg, windows) if tables else (None, None, None)
        kw = dict(sgroups=s, groups=g, windows=w, min_len=min_len, all_matches=all_matches)
        rows, _ = brute(pats, flags, streams_of(A, offs), rt.gid_of_index, min_len, g, s, w, all_matches)
        assert np.array_equal(rt.scan(A, offs, **kw)[0], batch_events(rows, offs)), (min_len, all_matches, tables)
        rows, _ = brute(pats, flags, whole, ac.gid_of_index, min_len, g, s, w, all_matches)
        ev, st, pos, case = ac.scan(A, offs, **kw)
        assert np.array_equal(ev, call_events(rows, offs, np.zeros(nseg, np.int64))[0])
        ev, _, _, _ = ac.scan(B, offs, state=st, pos=pos, case=case, **kw)
        assert np.array_equal(ev, call_events(rows, offs, lens)[0]), (min_len, all_matches, tables)
        seen += len(rows)
    assert seen > 0


def test_input_t_and_f_with_a_shipped_dictionary():
    """Input T (batched) and the first calls of input F (flows) under et, the
    case of the text flipped by position, flags crc32 & 1."""
    pats = real_dictionary("et")
    flags = [flag_of(p) for p in pats]
    rt = Twin(pats, flags, pm.KIND_RT)
    text, offs = input_t_flipped("et")
    for min_len, all_matches in ((3, True), (3, False)):
        rows, stats = brute(pats, flags, streams_of(text, offs), rt.gid_of_index, min_len, all_matches=all_matches)
        assert stats["rejected"] > 0 and stats["nocase_case_differs"] > 0
        assert np.array_equal(rt.scan(text, offs, min_len=min_len, all_matches=all_matches)[0],
                              batch_events(rows, offs))
    ac = Twin(pats, flags, pm.KIND_AC)
    ftext, flows, ncalls = input_f_flipped("et")
    flows = flows[:48]  # the head lengths rotate through the flows: 48 hold every one of them three times
    whole = [bytes(ftext[f * 4096:(f + 1) * 4096]) for f in range(len(flows))]
    rows, _ = brute(pats, flags, whole, ac.gid_of_index, 3)
    st = pos = case = None
    straddle = 0
    for r in range(6):
        data, o, before = f_call(ftext, flows, r)
        ev, st, pos, case = ac.scan(data, o, state=st, pos=pos, case=case, min_len=3)
        want, s = call_events(rows, o, before)
        assert np.array_equal(ev, want), r
        straddle += s
    assert straddle > 0


def test_hand_built_classes_and_chains():
    pats = [p for p, _ in HAND]
    flags = [f for _, f in HAND]
    for kind in (pm.KIND_RT, pm.KIND_AC):
        tw = Twin(pats, flags, kind)
        gid = {p: int(tw.gid_of_index[k]) for k, p in enumerate(pats)}
        for t in HAND_TEXTS:
            text = np.frombuffer(t, np.uint8)
            offs = np.array([0, len(t)], np.int64)
            for all_matches in (True, False):
                rows, _ = brute(pats, flags, [t], tw.gid_of_index, 1, all_matches=all_matches)
                got = tw.scan(text, offs, min_len=1, all_matches=all_matches)[0]
                assert np.array_equal(got, batch_events(rows, offs)), (kind, t, all_matches)
        # spelled out: `{ never matches @[, 0xE1 'B' never matches "\xC1b", "\xC1B" does
        ev = tw.scan(np.frombuffer(HAND_TEXTS[1], np.uint8), np.array([0, 8], np.int64))[0]
        assert [(int(e) >> 24, int(e) & 0xFFFFFF) for e in ev] == [(4, gid[b"@["])]
        ev = tw.scan(np.frombuffer(HAND_TEXTS[2], np.uint8), np.array([0, 11], np.int64))[0]
        assert [(int(e) >> 24, int(e) & 0xFFFFFF) for e in ev] == [(4, gid[b"\xc1b"]), (7, gid[b"\xc1b"])]
        # the longest form on "/admin" reports admin; on "GET" the smaller gid of GET and get
        t = HAND_TEXTS[0]
        ev = tw.scan(np.frombuffer(t, np.uint8), np.array([0, len(t)], np.int64), all_matches=False)[0]
        at = {int(e) >> 24: int(e) & 0xFFFFFF for e in ev}
        assert at[t.index(b"/admin") + 5] == gid[b"admin"]
        assert at[t.index(b"/Admin") + 5] == gid[b"/Admin"]
        assert at[2] == min(gid[b"GET"], gid[b"get"])
        assert at[6] == gid[b"get"] and at[10] == gid[b"get"]


def _seam_dictionary():
    rng = np.random.default_rng(77)
    long_p = bytes(rng.choice(np.frombuffer(b"aAbBcC-", np.uint8), 140))
    return [long_p, b"aBcDe", b"abcde", b"cde"], [0, 0, 1, 1], long_p


def test_flow_seams_every_cut():
    """A case-sensitive pattern of 140 bytes (history word index 2) and one of 5,
    cut at every offset across two packets, with matching case and with one letter
    flipped before and after the cut; then byte by byte with an empty packet."""
    pats, flags, long_p = _seam_dictionary()
    tw = Twin(pats, flags, pm.KIND_AC)
    assert tw.W == 3
    gid = {p: int(tw.gid_of_index[k]) for k, p in enumerate(pats)}
    for p in (long_p, b"aBcDe"):
        letters = [k for k, c in enumerate(p) if chr(c).isalpha()]
        for cut in range(1, len(p)):
            lo = [k for k in letters if k < cut]
            hi_ = [k for k in letters if k >= cut]
            variants = [(p, True)]
            if lo:
                q = bytearray(p)
                q[lo[len(lo) // 2]] ^= 0x20
                variants.append((bytes(q), False))
            if hi_:
                q = bytearray(p)
                q[hi_[len(hi_) // 2]] ^= 0x20
                variants.append((bytes(q), False))
            # one flow per variant, all cut at the same place: packet 1 = "--" + v[:cut], packet 2 = v[cut:]
            p1 = [b"--" + v[:cut] for v, _ in variants]
            p2 = [v[cut:] for v, _ in variants]
            o1 = np.concatenate([[0], np.cumsum([len(x) for x in p1])]).astype(np.int64)
            o2 = np.concatenate([[0], np.cumsum([len(x) for x in p2])]).astype(np.int64)
            _, st, pos, case = tw.scan(np.frombuffer(b"".join(p1), np.uint8), o1, min_len=4)
            ev, _, _, case2 = tw.scan(np.frombuffer(b"".join(p2), np.uint8), o2, state=st, pos=pos, case=case,
                                      min_len=4)
            found = {int(np.searchsorted(o2, int(e) >> 24, side="right")) - 1 for e in ev
                     if (int(e) & 0xFFFFFF) == gid[p]}
            assert found == {k for k, (_, good) in enumerate(variants) if good}, (len(p), cut)
            for k, (v, _) in enumerate(variants):
                assert np.array_equal(case2[k], history_words(b"--" + v, tw.W))
    # byte by byte, an empty packet in between, against the flow in one piece
    flow = b"xx" + long_p + b"-abCDe-aBcDe" + long_p[:70] + long_p
    one = tw.scan(np.frombuffer(flow, np.uint8), np.array([0, len(flow)], np.int64))[0]
    rows, _ = brute(pats, flags, [flow], tw.gid_of_index, 1)
    assert np.array_equal(one, batch_events(rows, [0]))
    st = pos = case = None
    got = []
    for k in range(len(flow)):
        if k % 37 == 5:
            ev, st, pos, case = tw.scan(np.zeros(0, np.uint8), np.array([0, 0], np.int64), state=st, pos=pos, case=case)
            assert len(ev) == 0
        ev, st, pos, case = tw.scan(np.frombuffer(flow[k:k + 1], np.uint8), np.array([0, 1], np.int64), state=st,
                                    pos=pos, case=case)
        got += [(k << 24) | (int(e) & 0xFFFFFF) for e in ev]
        assert np.array_equal(case[0], history_words(flow[:k + 1], tw.W)), k
    assert np.array_equal(np.array(got, np.uint64), one)


# ---- history shifts: a middle packet that moves old history across a word boundary --------
SHIFT_LENGTHS = {64: 1, 65: 1, 66: 2, 129: 2, 130: 3, 200: 4}  # pattern length -> history words
SHIFT_MIDDLES = (1, 63, 64, 65, 127, 128)
SHIFT_CUTS = (1, 2, 63, 64, 65)


def shift_pattern(L):
    """A case-sensitive pattern of L letters of both cases."""
    rng = np.random.default_rng(900 + L)
    return bytes(rng.choice(np.frombuffer(b"aAbBcCdD", np.uint8), L))


def shift_flows(p):
    """The flows of one pattern: (packet 1, packet 2, packet 3, reported) with
    "--" + p cut after the first cut and again a middle length later, the third
    packet keeping at least a byte; after each unflipped flow its twins with
    one letter's case flipped in packet 1 and in packet 2."""
    L, flows = len(p), []
    for mid in SHIFT_MIDDLES:
        if mid > L - 2:
            continue
        for cut in sorted({min(c, L - mid - 1) for c in SHIFT_CUTS}):
            assert cut >= 1 and cut + mid < L
            for flip in (None, cut // 2, cut + mid // 2):
                v = bytearray(p)
                if flip is not None:
                    v[flip] ^= 0x20
                flows.append((b"--" + bytes(v[:cut]), bytes(v[cut:cut + mid]), bytes(v[cut + mid:]), flip is None))
    return flows


def shift_calls(flows):
    """Three calls, every flow's k-th packet in call k: [(text, offsets)]."""
    calls = []
    for k in range(3):
        parts = [f[k] for f in flows]
        offs = np.concatenate([[0], np.cumsum([len(x) for x in parts])]).astype(np.int64)
        calls.append((np.frombuffer(b"".join(parts), np.uint8), offs))
    return calls


def assert_shift_call(k, flows, offs, ev, hist, W):
    """Call k (0, 1, 2) of shift_calls: the pattern is reported at the last byte
    of the unflipped flows' third packet and nowhere else, and every flow's
    history is that of its bytes so far."""
    want = [(int(offs[j + 1]) - 1) << 24 | 1 for j, f in enumerate(flows) if f[3]] if k == 2 else []
    assert [int(e) for e in ev] == want, k
    hist = np.asarray(hist).reshape(len(flows), W)
    for j, f in enumerate(flows):
        assert np.array_equal(hist[j], history_words(b"".join(f[:k + 1]), W)), (k, j)


@pytest.mark.parametrize("L", sorted(SHIFT_LENGTHS))
def test_history_shifts_three_packets(L):
    p = shift_pattern(L)
    tw = Twin([p], [0], pm.KIND_AC)
    assert tw.W == SHIFT_LENGTHS[L]
    flows = shift_flows(p)
    assert len(flows) == 3 * sum(f[3] for f in flows)
    assert {len(f[1]) for f in flows} == {m for m in SHIFT_MIDDLES if m <= L - 2}
    st = pos = case = None
    for k, (text, offs) in enumerate(shift_calls(flows)):
        ev, st, pos, case = tw.scan(text, offs, state=st, pos=pos, case=case)
        assert_shift_call(k, flows, offs, ev, case, tw.W)


def two_word_shift_flows():
    """A pattern of 200 bytes (4 history words); packet 2 is 128 bytes that are
    no pattern text, with upper-case letters of their own.  Flow 0 then brings
    the rest of the pattern: the head in its history completes nothing.  Flow
    1 brings the whole pattern, found in the text alone."""
    p = shift_pattern(200)
    filler = bytes(b"xXyYzZ-"[(k * k) % 7] for k in range(128))
    return p, [(b"--" + p[:72], filler, p[72:], False), (b"--" + p[:72], filler, p, True)]


def assert_two_word_shift(flows, hists):
    """hists[k]: the (flows, 4) history words after call k.  Call 2 moved
    every word of call 1 up by two and filled the first two from its bytes."""
    for j, f in enumerate(flows):
        assert len(f[1]) == 128
        assert np.array_equal(hists[1][j][2:], hists[0][j][:2]), j
        assert np.array_equal(hists[1][j][:2], history_words(f[1], 2)), j
        assert hists[0][j][0] != 0 and hists[0][j][1] != 0, j


def test_history_two_word_shift():
    p, flows = two_word_shift_flows()
    tw = Twin([p], [0], pm.KIND_AC)
    assert tw.W == 4
    st = pos = case = None
    hists = []
    for k, (text, offs) in enumerate(shift_calls(flows)):
        ev, st, pos, case = tw.scan(text, offs, state=st, pos=pos, case=case)
        assert_shift_call(k, flows, offs, ev, case, 4)
        hists.append(case.copy())
    assert_two_word_shift(flows, hists)


def test_reductions_and_tables():
    pats = fuzz_dictionary(2, n=120, long_cs=False)
    text = fuzz_text(pats, 2, 8192)
    offs = stream_offsets(len(text), 2)
    streams = streams_of(text, offs)
    # every flag 0: the exact matcher; every flag 1: the matcher of the folded patterns over folded text
    for kind in (pm.KIND_RT, pm.KIND_AC):
        tw0 = Twin(pats, [0] * len(pats), kind)
        rows, _ = brute(pats, [0] * len(pats), streams, tw0.gid_of_index)
        assert np.array_equal(tw0.scan(text, offs)[0], batch_events(rows, offs))
        tw1 = Twin(pats, [1] * len(pats), kind)
        assert tw1.W == 0 and not tw1.array("nc_cword").any()
        rows, _ = brute(pats, [1] * len(pats), streams, tw1.gid_of_index)
        assert np.array_equal(tw1.scan(text, offs)[0], batch_events(rows, offs))
        # gids are those of pm_flat_build of the same patterns
        from table_emulator import FlatImage
        assert np.array_equal(FlatImage(pats, kind).array("index_of_gid"), tw1.array("index_of_gid"))
    # the class tables: heads are the smallest gid of a class, lengths never rise along cnext
    tw = Twin(pats, [flag_of(p) for p in pats], pm.KIND_RT)
    head, cnext, ln = tw.array("nc_head"), tw.array("nc_cnext"), tw.array("len")
    iog = tw.array("index_of_gid")
    for f in range(1, len(head)):
        h = int(head[f]) & 0x7FFFFFFF
        members, steps = [], 0
        while h and steps <= int(tw.info[0]):
            members.append(h)
            h = int(cnext[h]) & 0x7FFFFFFF
            steps += 1
        assert h == 0 and members
        assert all(ln[a] >= ln[b] for a, b in zip(members, members[1:]))
        first = [m for m in members if ln[m] == ln[members[0]]]
        assert first == sorted(first)
        assert len({fold(pats[iog[m]]) for m in first}) == 1


def test_argument_rules():
    pats = [p for p, _ in HAND]
    tw = Twin(pats, [f for _, f in HAND], pm.KIND_RT)
    lib = tw.lib
    text = np.frombuffer(b"GET", np.uint8)
    offs = np.array([0, 3], np.int64)
    ev = np.zeros(8, np.uint64)
    total = ctypes.c_size_t(0)
    sg = np.array([1], np.uint32)

    def call(h, min_len=1, sgroups=None, nev=ctypes.byref(total)):
        return lib.pm_flat_host_scan_nocase(h, _p(text, U8P), _p(offs, I64P), 1, None, None, None, None, None, None,
                                            _p(sgroups, U32P), None, None, None, min_len, 1, _p(ev, U64P), 8, nev)
    assert call(tw.h) == 0 and total.value == 2
    assert call(tw.h, min_len=0) == -2
    assert call(tw.h, sgroups=sg) == -2  # stream masks without pattern masks
    assert call(tw.h, nev=None) == -2
    from table_emulator import FlatImage
    plain = FlatImage(pats, pm.KIND_RT)
    assert call(plain.h) == -1  # not a handle of pm_flat_build_nocase
    # a count-only call
    total.value = 0
    rc = lib.pm_flat_host_scan_nocase(tw.h, _p(text, U8P), _p(offs, I64P), 1, None, None, None, None, None, None, None,
                                      None, None, None, 1, 1, None, 0, ctypes.byref(total))
    assert rc == 0 and total.value == 2


def test_flip_case_changes_letters_only():
    t = np.frombuffer(bytes(range(256)) * 8, np.uint8)
    f = flip_case(t)
    changed = f != t
    assert changed.any()
    assert np.all(np.char.isalpha(t[changed].view("S1").astype("U1")))
    assert fold(f.tobytes()) == fold(t.tobytes()) and INF == 0xFFFFFFFF
