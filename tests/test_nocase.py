"""Per-pattern nocase on the GPU (pm_hip_set_nocase,
pm_hip_scan_batch_nocase_device, pm_hip_scan_flows_nocase_device,
pm_hip_read_*_nocase): expected lists come from the tests' own brute force
(nocase_inputs.brute: bytes.find over folded text, the exact compare for a
case-sensitive pattern), never from the library's tables; events are compared
exactly, as sorted u64."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from nocase_inputs import (HAND, HAND_TEXTS, batch_events, brute, call_events, f_call, family_dictionary, flag_of,
                           fold, fuzz_dictionary, fuzz_text, history_words, input_f_flipped, input_t_flipped,
                           real_dictionary, stream_groups, stream_offsets)
from test_batch import _dev, _stream
from test_events import POISON64, Ev, _text_dev
from test_flows import _state_values, _states
from test_gpu_parity import _torch
from test_nocase_cpu import (SHIFT_LENGTHS, SHIFT_MIDDLES, _seam_dictionary, assert_shift_call, assert_two_word_shift,
                             shift_calls, shift_flows, shift_pattern, streams_of, tables_of, two_word_shift_flows)

pytestmark = pytest.mark.gpu

_cache = {}


def build(pats, kind, flags=None):
    m = pm.HipMatcher(kind)
    for p in pats:
        m.add_pattern(p)
    m.compile()
    if flags is not None:
        m.set_nocase(flags)
    return m


def gids_of(m, n):
    g = np.zeros(n, dtype=np.int64)
    for gid in range(1, n + 1):
        g[m.lib.pm_hip_gid_index(m.obj, gid)] = gid
    return g


def fuzz(kind):
    """The shared fuzz dictionary (seed 0) compiled with its crc32 flags."""
    if kind not in _cache:
        pats = fuzz_dictionary(0)
        flags = [flag_of(p) for p in pats]
        m = build(pats, kind, flags)
        _cache[kind] = (pats, flags, m, gids_of(m, len(pats)))
    return _cache[kind]


def _u64(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64).copy()).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _batch(m, torch, text, offs, sg, min_len, all_matches, ev=None):
    ev = Ev(torch, 64 * len(text)) if ev is None else ev
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    d_sg = None if sg is None else _states(torch, sg)
    m.scan_batch_nocase_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text), _ptr(d_sg), min_len,
                               all_matches, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _flow(m, torch, text, offs, st_in, pos_in, case_in, sg, min_len, all_matches, ev=None):
    """One device flow call: (ev, state_out, pos_out, case_out) as device tensors."""
    nseg = len(offs) - 1
    W = m.case_words
    ev = Ev(torch, 64 * len(text) + 64) if ev is None else ev
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    d_sg = None if sg is None else _states(torch, sg)
    st_out = _states(torch, np.full(nseg, 0xEEEEEEEE, np.uint32))
    pos_out = _u64(torch, np.full(nseg, 0xDDDDDDDDDDDDDDDD, np.uint64))
    case_out = _u64(torch, np.full(max(nseg * W, 1), 0xCCCCCCCCCCCCCCCC, np.uint64))
    m.scan_flows_nocase_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, len(text), _ptr(st_in), st_out.data_ptr(),
                               _ptr(d_sg), min_len, all_matches, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(),
                               _stream(torch), _ptr(pos_in), pos_out.data_ptr(), _ptr(case_in), case_out.data_ptr())
    torch.cuda.synchronize()
    return ev, st_out, pos_out, case_out


def _list(ev):
    total = ev.total()
    assert total <= ev.cap
    got = np.sort(ev.buf[:total].cpu().numpy().view(np.uint64))
    assert bool((ev.buf[total:] == POISON64 - (1 << 64)).all()), "nothing at or past the cursor was written"
    return got


def test_batch_nocase_against_brute_force():
    torch = _torch()
    pats, flags, m, gid = fuzz("auto")
    text = fuzz_text(pats, 0, 49152)
    offs = stream_offsets(len(text), 0)
    streams = streams_of(text, offs)
    groups, windows = tables_of(pats)
    sg = stream_groups(len(offs) - 1)
    seen_nc = seen_rej = 0
    try:
        for tables, configs in ((False, [(1, False), (3, True)]), (True, [(3, True), (5, False), (3, False)])):
            if tables:
                m.set_groups(groups)
                m.set_windows(*windows)
            for min_len, all_matches in configs:
                rows, stats = brute(pats, flags, streams, gid, min_len, groups if tables else None,
                                    sg if tables else None, windows if tables else None, all_matches)
                want = batch_events(rows, offs)
                assert len(want) > 0
                seen_nc += stats["nocase_case_differs"]
                seen_rej += stats["rejected"]
                for small_max in (-1, 0):
                    assert m.set_option("rt_small_max", small_max) == 0
                    got = _list(_batch(m, torch, text, offs, sg if tables else None, min_len, all_matches))
                    assert np.array_equal(got, want), (tables, min_len, all_matches, small_max)
    finally:
        m.set_option("rt_small_max", -1)
        _cache.pop("auto")  # the group and window tables stay set on this object
    assert seen_nc > 0 and seen_rej > 0


def test_flow_nocase_against_brute_force_and_segment_seams():
    torch = _torch()
    pats, flags, m, gid = fuzz("ac")
    assert m.case_words == 3
    A, B = fuzz_text(pats, 0, 49152), fuzz_text(pats, 50, 49152)
    offs = stream_offsets(len(A), 0)
    nseg = len(offs) - 1
    lens = np.diff(offs)
    whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
    hist_a = np.array([history_words(A[offs[j]:offs[j + 1]], 3) for j in range(nseg)])
    hist_ab = np.array([history_words(w, 3) for w in whole])
    seen_straddle = seen_rej = 0
    try:
        for min_len, all_matches, seg in ((3, True, 0), (1, False, 16), (5, True, 16)):
            assert m.set_option("flow_seg", seg) == 0
            rows, stats = brute(pats, flags, whole, gid, min_len, all_matches=all_matches)
            ev, st, pos, case = _flow(m, torch, A, offs, None, None, None, None, min_len, all_matches)
            want_a, _ = call_events(rows, offs, np.zeros(nseg, np.int64))
            assert np.array_equal(_list(ev), want_a), ("A", min_len, all_matches, seg)
            assert np.array_equal(case.cpu().numpy().view(np.uint64).reshape(nseg, 3), hist_a)
            assert np.all(_state_values(st) < m.nocase_flow_states)
            ev, st2, _, case2 = _flow(m, torch, B, offs, st, None, case, None, min_len, all_matches)
            want_b, straddle = call_events(rows, offs, lens)
            assert np.array_equal(_list(ev), want_b), ("B", min_len, all_matches, seg)
            assert np.array_equal(case2.cpu().numpy().view(np.uint64).reshape(nseg, 3), hist_ab)
            seen_straddle += straddle
            seen_rej += stats["rejected"]
        # with group and window tables: positions carried too
        groups, windows = tables_of(pats)
        sg = stream_groups(nseg)
        m.set_groups(groups)
        m.set_windows(*windows)
        m.set_option("flow_seg", 0)
        for all_matches in (True, False):
            rows, stats = brute(pats, flags, whole, gid, 3, groups, sg, windows, all_matches)
            ev, st, pos, case = _flow(m, torch, A, offs, None, None, None, sg, 3, all_matches)
            assert np.array_equal(_list(ev), call_events(rows, offs, np.zeros(nseg, np.int64))[0])
            assert np.array_equal(pos.cpu().numpy().view(np.uint64), lens.astype(np.uint64))
            ev, _, pos2, _ = _flow(m, torch, B, offs, st, pos, case, sg, 3, all_matches)
            assert np.array_equal(_list(ev), call_events(rows, offs, lens)[0])
            assert np.array_equal(pos2.cpu().numpy().view(np.uint64), 2 * lens.astype(np.uint64))
    finally:
        m.set_option("flow_seg", 0)
        _cache.pop("ac")
    assert seen_straddle > 0 and seen_rej > 0


@pytest.mark.parametrize("name", ["no_short", "only_short", "many", "unary"])
def test_families_batched_and_flow(name):
    """fuzz_inputs' four families over letters of both cases on one auto object:
    batched over A, as flows over A then B."""
    torch = _torch()
    pats = family_dictionary(name)
    flags = [flag_of(p) for p in pats]
    m = build(pats, "auto", flags)
    gid = gids_of(m, len(pats))
    A, B = fuzz_text(pats, 7, 16384), fuzz_text(pats, 57, 16384)
    offs = stream_offsets(len(A), 7)
    nseg = len(offs) - 1
    lens = np.diff(offs)
    whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
    seen = 0
    for min_len, all_matches in ((3, True), (1, False)):
        rows, _ = brute(pats, flags, streams_of(A, offs), gid, min_len, all_matches=all_matches)
        assert np.array_equal(_list(_batch(m, torch, A, offs, None, min_len, all_matches)), batch_events(rows, offs))
        rows, _ = brute(pats, flags, whole, gid, min_len, all_matches=all_matches)
        ev, st, _, case = _flow(m, torch, A, offs, None, None, None, None, min_len, all_matches)
        assert np.array_equal(_list(ev), call_events(rows, offs, np.zeros(nseg, np.int64))[0])
        ev, _, _, _ = _flow(m, torch, B, offs, st, None, case if m.case_words else None, None, min_len, all_matches)
        assert np.array_equal(_list(ev), call_events(rows, offs, lens)[0]), (min_len, all_matches)
        seen += len(rows)
    assert seen > 0  # (only_short has no event at min_len 3: its patterns end below it)
    m.free()


def test_input_t_and_f_with_a_shipped_dictionary():
    """Input T (batched) and the first calls of input F (flows) under et, the
    case of the text flipped by position, flags crc32 & 1."""
    torch = _torch()
    pats = real_dictionary("et")
    flags = [flag_of(p) for p in pats]
    m = build(pats, "auto", flags)
    gid = gids_of(m, len(pats))
    text, offs = input_t_flipped("et")
    rows, stats = brute(pats, flags, streams_of(text, offs), gid, 3)
    assert stats["rejected"] > 0 and stats["nocase_case_differs"] > 0
    assert np.array_equal(_list(_batch(m, torch, text, offs, None, 3, True)), batch_events(rows, offs))
    ftext, flows, _ = input_f_flipped("et")
    flows = flows[:48]
    whole = [bytes(ftext[f * 4096:(f + 1) * 4096]) for f in range(len(flows))]
    rows, _ = brute(pats, flags, whole, gid, 3, all_matches=False)
    st = case = None
    straddle = 0
    for r in range(6):
        data, o, before = f_call(ftext, flows, r)
        ev, st, _, case = _flow(m, torch, data, o, st, None, case, None, 3, False)
        want, s = call_events(rows, o, before)
        assert np.array_equal(_list(ev), want), r
        straddle += s
    assert straddle > 0
    m.free()


@pytest.mark.parametrize("kind", ["rt", "ac"])
def test_hand_built_classes_and_chains(kind):
    _torch()
    pats = [p for p, _ in HAND]
    flags = [f for _, f in HAND]
    m = build(pats, kind, flags)
    g = gids_of(m, len(pats))
    gid = {p: int(g[k]) for k, p in enumerate(pats)}
    flows = kind == "ac"

    def read(t, all_matches):
        st = np.zeros(1, np.uint32) if flows else None
        return m._read_nocase(np.frombuffer(t, np.uint8), [0, len(t)], None, st, None, None, 1, all_matches)[0]
    for t in HAND_TEXTS:
        for all_matches in (True, False):
            rows, _ = brute(pats, flags, [t], g, 1, all_matches=all_matches)
            assert np.array_equal(read(t, all_matches), batch_events(rows, [0])), (t, all_matches)
    assert [(int(e) >> 24, int(e) & 0xFFFFFF) for e in read(HAND_TEXTS[1], True)] == [(4, gid[b"@["])]
    assert [int(e) >> 24 for e in read(HAND_TEXTS[2], True)] == [4, 7]
    t = HAND_TEXTS[0]
    at = {int(e) >> 24: int(e) & 0xFFFFFF for e in read(t, False)}
    assert at[t.index(b"/admin") + 5] == gid[b"admin"] and at[t.index(b"/Admin") + 5] == gid[b"/Admin"]
    assert at[2] == min(gid[b"GET"], gid[b"get"])
    for gd in range(1, len(pats) + 1):
        assert m.pattern_nocase(gd) == bool(flags[m.lib.pm_hip_gid_index(m.obj, gd)])
    assert m.pattern_nocase(0) is None and m.pattern_nocase(len(pats) + 1) is None
    m.free()


def test_flow_seams_pieces_equal_one_piece():
    """The 140-byte and the 5-byte case-sensitive pattern cut at every offset
    across two packets (one flow per cut, all in one call), with one letter's
    case flipped before and after the cut; then a flow fed byte by byte."""
    _torch()
    pats, flags, long_p = _seam_dictionary()
    m = build(pats, "ac", flags)
    assert m.case_words == 3
    g = gids_of(m, len(pats))
    gid = {p: int(g[k]) for k, p in enumerate(pats)}
    for p in (long_p, b"aBcDe"):
        letters = [k for k, c in enumerate(p) if chr(c).isalpha()]
        flowsv, good = [], []
        for cut in range(1, len(p)):
            lo = [k for k in letters if k < cut]
            hi = [k for k in letters if k >= cut]
            flowsv.append((p, cut))
            good.append(True)
            for side in (lo, hi):
                if side:
                    q = bytearray(p)
                    q[side[len(side) // 2]] ^= 0x20
                    flowsv.append((bytes(q), cut))
                    good.append(False)
        p1 = [b"--" + v[:c] for v, c in flowsv]
        p2 = [v[c:] for v, c in flowsv]
        o1 = pm.batch_offsets(p1)
        o2 = pm.batch_offsets(p2)
        n = len(flowsv)
        _, st, pos, case = m._read_nocase(np.frombuffer(b"".join(p1), np.uint8), o1, None, np.zeros(n, np.uint32),
                                          np.zeros(n, np.uint64), np.zeros((n, 3), np.uint64), 4, True)
        ev, _, _, case2 = m._read_nocase(np.frombuffer(b"".join(p2), np.uint8), o2, None, st, pos, case, 4, True)
        found = {int(np.searchsorted(o2, int(e) >> 24, side="right")) - 1 for e in ev if (int(e) & 0xFFFFFF) == gid[p]}
        assert found == {k for k in range(n) if good[k]}, len(p)
        want_hist = np.array([history_words(b"--" + v, 3) for v, _ in flowsv])
        assert np.array_equal(case2, want_hist)
    flow = b"xx" + long_p + b"-abCDe-aBcDe" + long_p[:70] + long_p
    one = m._read_nocase(np.frombuffer(flow, np.uint8), [0, len(flow)], None, np.zeros(1, np.uint32), None, None, 1,
                         True)[0]
    rows, _ = brute(pats, flags, [flow], g, 1)
    assert np.array_equal(one, batch_events(rows, [0]))
    st, case, got = np.zeros(1, np.uint32), np.zeros((1, 3), np.uint64), []
    for k in range(len(flow)):
        if k % 37 == 5:  # an empty packet: nothing found, everything kept
            ev, st2, _, case2 = m._read_nocase(np.zeros(0, np.uint8), [0, 0], None, st, None, case, 1, True)
            assert len(ev) == 0 and np.array_equal(st2, st) and np.array_equal(case2, case)
        ev, st, _, case = m._read_nocase(np.frombuffer(flow[k:k + 1], np.uint8), [0, 1], None, st, None, case, 1, True)
        got += [(k << 24) | (int(e) & 0xFFFFFF) for e in ev]
        assert np.array_equal(case[0], history_words(flow[:k + 1], 3)), k
    assert np.array_equal(np.array(got, np.uint64), one)
    m.free()


def _shift_run(m, flows, W):
    """shift_calls through the host form of the flow scan, the states,
    positions and histories carried: the (flows, W) history words after each call."""
    n = len(flows)
    assert m.lib.pm_hip_gid_index(m.obj, 1) == 0  # one pattern: gid 1
    st, pos, case, hists = np.zeros(n, np.uint32), np.zeros(n, np.uint64), np.zeros((n, W), np.uint64), []
    for k, (text, offs) in enumerate(shift_calls(flows)):
        ev, st, pos, case = m._read_nocase(text, offs, None, st, pos, case, 1, True)
        assert_shift_call(k, flows, offs, ev, case, W)
        hists.append(np.asarray(case).reshape(n, W).copy())
    return hists


@pytest.mark.parametrize("L", sorted(SHIFT_LENGTHS))
def test_history_shifts_three_packets(L):
    """nocase_history_kernel with a middle packet of 1, 63, 64, 65, 127 or 128
    bytes between the two parts of a case-sensitive pattern: the old history
    moves across a word boundary (old = back - len, word old >> 6) while the
    pattern is open; a letter whose case was flipped in packet 1 or 2 must
    still reject it at its last byte in packet 3."""
    _torch()
    p = shift_pattern(L)
    m = build([p], "ac", [0])
    try:
        assert m.case_words == SHIFT_LENGTHS[L]
        flows = shift_flows(p)
        assert {len(f[1]) for f in flows} == {mid for mid in SHIFT_MIDDLES if mid <= L - 2}
        _shift_run(m, flows, m.case_words)
    finally:
        m.free()


def test_history_two_word_shift():
    _torch()
    p, flows = two_word_shift_flows()
    m = build([p], "ac", [0])
    try:
        assert m.case_words == 4
        assert_two_word_shift(flows, _shift_run(m, flows, 4))
    finally:
        m.free()


def test_reductions_to_the_matches_calls():
    _torch()
    pats = fuzz_dictionary(2, n=120, long_cs=False)
    text = fuzz_text(pats, 2, 16384)
    offs = stream_offsets(len(text), 2)
    nseg = len(offs) - 1
    for kind in ("rt", "ac"):
        flows = kind == "ac"
        st = np.zeros(nseg, np.uint32) if flows else None
        # every flag 0: the matches call of the same object
        m = build(pats, kind)
        bytes_before = m.table_bytes
        before = m._read_events(text, offs, st, 1, all_matches=True)[0]
        m.set_nocase(np.zeros(len(pats), np.uint8))
        assert m.case_words == 1  # every pattern case-sensitive, the longest with a letter below 66 bytes
        assert np.array_equal(m._read_nocase(text, offs, None, st, None, None, 1, True)[0], before)
        # an existing call's output and the tables it uses are untouched by set_nocase
        assert np.array_equal(m._read_events(text, offs, st, 1, all_matches=True)[0], before)
        assert m.table_bytes == bytes_before + m.nocase_stats()[2] > bytes_before
        # a reload that flips every flag: the folded matcher over folded text, through the pattern bytes
        m.set_nocase(np.ones(len(pats), np.uint8))
        assert m.case_words == 0
        assert m.table_bytes == bytes_before + m.nocase_stats()[2]
        got = m._read_nocase(text, offs, None, st, None, None, 1, True)[0]
        fpats = sorted({fold(p) for p in pats})
        m2 = build(fpats, kind)
        ftext = np.frombuffer(fold(text.tobytes()), np.uint8)
        ev2 = m2._read_events(ftext, offs, st, 1, all_matches=True)[0]
        g1 = gids_of(m, len(pats))
        members = {}  # folded bytes -> the gids of the patterns (the add that wins each byte string) in its class
        for p, k in {p: k for k, p in enumerate(pats)}.items():
            members.setdefault(fold(p), []).append(int(g1[k]))
        want = [(int(e) >> 24 << 24) | gd for e in ev2
                for gd in members[fpats[m2.lib.pm_hip_gid_index(m2.obj, int(e) & 0xFFFFFF)]]]
        assert np.array_equal(got, np.sort(np.array(want, np.uint64)))
        # lower-case patterns and text, every flag 1: the matches call itself
        m3 = build(fpats, kind, np.ones(len(fpats), np.uint8))
        assert np.array_equal(m3._read_nocase(ftext, offs, None, st, None, None, 1, True)[0], ev2)
        # an object that never calls set_nocase holds the tables it held before
        assert m2.table_bytes == build(fpats, kind).table_bytes
        for x in (m, m2, m3):
            x.free()


def test_return_codes_cursor_cap_and_capture():
    torch = _torch()
    lib = pm.load()
    pats = [p for p, _ in HAND]
    flags = np.array([f for _, f in HAND], np.uint8)
    fp = flags.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    raw = pm.HipMatcher("auto")
    for p in pats:
        raw.add_pattern(p)
    assert lib.pm_hip_set_nocase(raw.obj, fp, len(pats)) == -1  # before compile()
    raw.compile()
    text = np.frombuffer(HAND_TEXTS[0] * 40, np.uint8)
    n = len(text)
    offs = np.array([0, 25, 25, 500, n], np.int64)
    nseg = 4
    d_text, d_offs = _text_dev(torch, text), _dev(torch, offs)
    ev = Ev(torch, 4096)
    sgd = _states(torch, np.ones(nseg, np.uint32))
    s = _stream(torch)
    fb, ff = lib.pm_hip_scan_batch_nocase_device, lib.pm_hip_scan_flows_nocase_device
    t, o, e, c = d_text.data_ptr(), d_offs.data_ptr(), ev.buf.data_ptr(), ev.nev.data_ptr()
    assert fb(raw.obj, t, o, nseg, n, None, 1, 1, e, ev.cap, c, s) == -9  # before set_nocase
    assert ff(raw.obj, t, o, nseg, n, None, None, None, 1, 1, e, ev.cap, c, s, None, None, None, None) == -9
    assert lib.pm_hip_pattern_nocase(raw.obj, 1) == -1 and raw.case_words == 0 and raw.nocase_flow_states == 0
    assert lib.pm_hip_set_nocase(raw.obj, fp, len(pats) - 1) == -2
    assert lib.pm_hip_set_nocase(raw.obj, None, len(pats)) == -2
    assert lib.pm_hip_set_nocase(raw.obj, fp, len(pats)) == 0
    W = raw.case_words
    assert W == 1 and raw.nocase_flow_states > 1  # "/Admin": ceil(5 / 64)
    assert fb(raw.obj, t, o, nseg, n, sgd.data_ptr(), 1, 1, e, ev.cap, c, s) == -7  # masks without group tables
    assert ff(raw.obj, t, o, nseg, n, None, None, sgd.data_ptr(), 1, 1, e, ev.cap, c, s, None, None, None, None) == -7
    assert fb(raw.obj, t, o, nseg, n, None, 0, 1, e, ev.cap, c, s) == -2  # min_len 0
    hist = _u64(torch, np.zeros(nseg * W, np.uint64))
    assert ff(raw.obj, t, o, nseg, n, None, None, None, 1, 1, e, ev.cap, c, s, None, None, hist.data_ptr(),
              hist.data_ptr()) == -2  # case_in == case_out
    torch.cuda.synchronize()
    assert ev.total() == 0
    ev.assert_guard(0)
    # the kinds without the folded image a scan walks
    rt, ac = build(pats, "rt", flags), build(pats, "ac", flags)
    assert ff(rt.obj, t, o, nseg, n, None, None, None, 1, 1, e, ev.cap, c, s, None, None, None, None) == -6
    assert fb(ac.obj, t, o, nseg, n, None, 1, 1, e, ev.cap, c, s) == -6
    # the list: appended at the cursor, cut at cap, counted in full; a count-only call
    g = gids_of(raw, len(pats))
    rows, _ = brute(pats, flags, streams_of(text, offs), g, 1)
    want = batch_events(rows, offs)
    full = _list(_batch(raw, torch, text, offs, None, 1, True))
    assert np.array_equal(full, want)
    small = Ev(torch, 7, cursor=3)
    _batch(raw, torch, text, offs, None, 1, True, small)
    assert small.total() == 3 + len(want)
    sl = small.slots()
    assert np.all(sl[:3] == POISON64) and np.all(sl[7:] == POISON64) and set(sl[3:7].tolist()) <= set(want.tolist())
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    assert fb(raw.obj, t, o, nseg, n, None, 1, 1, None, 0, cnt.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert int(cnt.item()) == len(want)
    fl = Ev(torch, 4096)
    _flow(raw, torch, text, offs, None, None, None, None, 1, True, fl)
    assert np.array_equal(_list(fl), want)  # fresh flows answer as streams
    # nseg == 0 and n == 0: nothing launched, nothing written
    assert fb(raw.obj, t, o, 0, 0, None, 1, 1, e, ev.cap, c, s) == 0
    assert ff(raw.obj, t, o, 0, 0, None, None, None, 1, 1, e, ev.cap, c, s, None, None, None, None) == 0
    # n == 0 with streams: the copy pass moves states and histories
    zo = _dev(torch, np.zeros(nseg + 1, np.int64))
    st_in = _states(torch, np.array([1, 0, 1, 0], np.uint32))
    st_out = _states(torch, np.full(nseg, 0xEEEEEEEE, np.uint32))
    h_in = _u64(torch, np.arange(1, nseg * W + 1, dtype=np.uint64))
    h_out = _u64(torch, np.zeros(nseg * W, np.uint64))
    assert ff(raw.obj, t, zo.data_ptr(), nseg, 0, st_in.data_ptr(), st_out.data_ptr(), None, 1, 1, e, ev.cap, c, s,
              None, None, h_in.data_ptr(), h_out.data_ptr()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_state_values(st_out), _state_values(st_in)) and torch.equal(h_in, h_out)
    # NULL histories where W == 0
    nc = build([b"get", b"admin"], "ac", [1, 1])
    assert nc.case_words == 0
    z = Ev(torch, 4096)
    _flow(nc, torch, text, offs, None, None, None, None, 1, True, z)
    assert z.total() > 0
    # both device calls captured into a graph (nothing is allocated) and replayed
    st = torch.cuda.Stream()
    gev_b, gev_f = Ev(torch, 4096), Ev(torch, 4096)
    so, co = _states(torch, np.zeros(nseg, np.uint32)), _u64(torch, np.zeros(nseg * W, np.uint64))
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr, stream=st):
        assert fb(raw.obj, t, o, nseg, n, None, 1, 1, gev_b.buf.data_ptr(), gev_b.cap, gev_b.nev.data_ptr(),
                  st.cuda_stream) == 0
        assert ff(raw.obj, t, o, nseg, n, None, so.data_ptr(), None, 1, 1, gev_f.buf.data_ptr(), gev_f.cap,
                  gev_f.nev.data_ptr(), st.cuda_stream, None, None, None, co.data_ptr()) == 0
    torch.cuda.synchronize()
    for _ in range(2):
        gev_b.nev.zero_()
        gev_f.nev.zero_()
        gr.replay()
        torch.cuda.synchronize()
        assert np.array_equal(np.sort(gev_b.slots()[:gev_b.total()]), want)
        assert np.array_equal(np.sort(gev_f.slots()[:gev_f.total()]), want)
    for x in (raw, rt, ac, nc):
        x.free()


def test_flow_table_scan_nocase():
    _torch()
    pats, flags, long_p = _seam_dictionary()
    m = build(pats, "ac", flags)
    g = gids_of(m, len(pats))
    m._codes = np.arange(len(pats) + 1, dtype=np.uint32)  # no dictionary file: a gid is its own code
    ft = pm.FlowTable(m)
    flow_a = b"--" + long_p + b"aBcDe" + long_p
    flow_b = b"abCDE" + long_p[:100].swapcase() + long_p
    cuts_a, cuts_b = [0, 3, 80, 81, 200, len(flow_a)], [0, 50, 50, 120, 121, len(flow_b)]
    got = {"a": [], "b": []}
    for r in range(5):
        pk = [("a", flow_a[cuts_a[r]:cuts_a[r + 1]]), ("b", flow_b[cuts_b[r]:cuts_b[r + 1]])]
        for (key, _), base, (pos, codes) in zip(pk, (cuts_a[r], cuts_b[r]), ft.scan_nocase(pk, min_len=1)):
            got[key] += [((int(p) + base) << 24) | int(c) for p, c in zip(pos, codes)]
    for key, flow in (("a", flow_a), ("b", flow_b)):
        rows, _ = brute(pats, flags, [flow], g, 1)
        assert np.array_equal(np.sort(np.array(got[key], np.uint64)), batch_events(rows, [0])), key
    # bytes another scan method saw are bytes the folded automaton missed
    ft.scan([("a", b"zz")])
    with pytest.raises(ValueError):
        ft.scan_nocase([("a", b"abcde")])
    ft.end("a")
    assert [len(p) for p, _ in ft.scan_nocase([("a", b"abcde")], min_len=1)] == [2]  # abcde, cde: a fresh flow
    with pytest.raises(ValueError):
        ft.scan_nocase([("b", b"x"), ("b", b"y")])
    m.free()
