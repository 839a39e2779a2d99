"""Pattern groups (pm_hip_set_groups, pm_hip_scan_batch_groups_device,
pm_hip_scan_flows_groups_device, pm_hip_read_*_groups): one merged automaton,
a group mask per pattern and one per stream; a stream's list holds the
patterns visible to it only -- all of them, or the longest one per position.
Expected lists come from the oracle and the tests' own tables
(tests/group_inputs.py); lists are compared after sorting, positions and the
codes of the gids, exactly."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream
from flow_inputs import F_FLOWS, input_f
from group_inputs import ALL_GROUPS, TABLE, all_ones, expected_groups, masks_by_index, pattern_mask, stream_masks
from match_inputs import deepest_pattern, sort_matches, suffix_chains
from oracle_lib import dict_paths, oracle_for
from test_batch import _dev, _stream
from test_events import I64P, POISON64, U8P, U32P, U64P, Ev, _batch_events, _flow_events, _text_dev
from test_flows import STATE_POISON, _flows, _oracle_two_calls, _seam_offsets, _state_values, _states
from test_gpu_parity import SHIP, _torch, fresh_matcher, matcher
from test_matches import _batch_matches, _flow_matches

pytestmark = pytest.mark.gpu

_masks = {}


def reversed_mask(b):
    """A second table, for the reload."""
    return pattern_mask(b[::-1])


def gmatcher(key, kind, fn=pattern_mask):
    """The shared matcher with the group table of fn set (every call sets it:
    some tests leave another table behind)."""
    m = matcher(key, kind)
    if (key, fn) not in _masks:
        _masks[(key, fn)] = masks_by_index(m._dict, fn)
    m.set_groups(_masks[(key, fn)])
    return m


def _sg_dev(torch, sg):
    return None if sg is None else _states(torch, sg)


def _batch_groups(m, torch, text, offs, sg, min_len, all_matches, ev):
    d_text, d_offs, d_sg = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64)), _sg_dev(torch, sg)
    m.scan_batch_groups_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text),
                               None if d_sg is None else d_sg.data_ptr(), min_len, all_matches, ev.buf.data_ptr(),
                               ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _flow_groups(m, torch, text, offs, st_in, st_out, sg, min_len, all_matches, ev):
    d_text, d_offs, d_sg = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64)), _sg_dev(torch, sg)
    m.scan_flows_groups_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text),
                               None if st_in is None else st_in.data_ptr(),
                               None if st_out is None else st_out.data_ptr(),
                               None if d_sg is None else d_sg.data_ptr(), min_len, all_matches, ev.buf.data_ptr(),
                               ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _assert_list(m, events, want, what):
    """events (u64, any order) == the expected (positions, codes), ascending by (position, code)."""
    events = np.asarray(events, dtype=np.uint64)
    assert len(events) == len(want[0]), f"{what}: {len(events)} events, expected {len(want[0])}"
    got_pos, got_gid = pm.unpack_events(events)
    got_pos, got_codes = sort_matches(got_pos, m._codes[got_gid])
    assert np.array_equal(got_pos, want[0]), f"{what}: positions differ"
    assert np.array_equal(got_codes, want[1]), f"{what}: codes differ"


def _assert_complete(m, ev, want, what, start=0):
    """The complete list, the cursor and the guard slots."""
    total = len(want[0])
    assert start + total <= ev.cap
    assert ev.total() == start + total, f"{what}: cursor {ev.total()}, expected {start + total}"
    slots = ev.slots()
    assert np.all(slots[:start] == POISON64)
    _assert_list(m, slots[start:start + total], want, what)
    ev.assert_guard(start + total)


# ---- 1. batched form, input T --------------------------------------------------
@pytest.mark.parametrize("min_len", [1, 3, 5])
@pytest.mark.parametrize("key,kind", [("et", "rt"), ("et", "auto"), ("merged", "rt")])
def test_batch_groups_input_t(key, kind, min_len):
    torch = _torch()
    text, offs, exp = input_t(key)
    sg = stream_masks(len(offs) - 1)
    m = gmatcher(key, kind)
    try:
        for all_matches in (True, False):
            want = expected_groups(key, exp, offs, sg, min_len, all_matches)
            assert len(want[0]) > 0
            for small_max in (-1, 0):  # the one-tile-per-workgroup form, and one workgroup per CU
                assert m.set_option("rt_small_max", small_max) == 0
                ev = _batch_groups(m, torch, text, offs, sg, min_len, all_matches, Ev(torch, len(want[0])))
                _assert_complete(m, ev, want, f"all {all_matches} rt_small_max {small_max}")
                assert m.kernel_last == pm.KIND_RT and m.dfa_form_last == 0
    finally:
        m.set_option("rt_small_max", -1)


# ---- 2. flow form, every call of input F -----------------------------------------
@pytest.mark.parametrize("key,kind,min_len", [("et", "ac", 3), ("et", "auto", 1), ("merged", "ac", 3)])
def test_flow_groups_input_f(key, kind, min_len):
    torch = _torch()
    F = input_f(key)
    m = gmatcher(key, kind)
    sg = stream_masks(F_FLOWS)
    other = np.roll(sg, 5)  # the second run's masks
    poison = np.full(F_FLOWS, STATE_POISON, np.uint32)
    ping = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
    pong = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
    dense = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
    seen = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        a, b = r & 1, 1 - (r & 1)
        for all_matches, st in ((True, ping), (False, pong)):
            masks = sg if all_matches else other
            want = expected_groups(key, exp, offs, masks, min_len, all_matches)
            ev = _flow_groups(m, torch, data, offs, st[a], st[b], masks, min_len, all_matches,
                              Ev(torch, len(want[0])))
            _assert_complete(m, ev, want, f"call {r} all {all_matches}")
            assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
            seen += ev.total()
        _flows(m, torch, data, offs, dense[a], dense[b])
        # the states are the dense flow call's, whatever the masks and the form
        assert np.array_equal(_state_values(ping[b]), _state_values(dense[b])), r
        assert np.array_equal(_state_values(pong[b]), _state_values(dense[b])), r
    assert seen > 0


# ---- 3. the deepest chain: direct path and flush, pending without emitting ------------
def test_groups_deepest_chain_repeated():
    """64 KiB of merged's pattern with the deepest suffix chain, repeated, at
    min_len 1, as one stream and cut at input T's offsets.  Stream masks
    alternate between all groups and one group that holds members of the
    chain below the head but not the head: the flow kernel's direct path and
    the flushes inside the rounds run with slots that are pending and do not
    emit."""
    torch = _torch()
    pat, depth = deepest_pattern("merged")
    assert depth == 24
    chains = suffix_chains("merged")
    by_code = {(f << 24) | l: b for f, l, b in oracle_for("merged").patterns()}
    head = next(c for c in chains if by_code[c] == pat)
    member_masks = [pattern_mask(by_code[int(c)]) for c in chains[head][0]]
    below = 0
    for x in member_masks[1:]:
        below |= x
    below &= ~member_masks[0]
    assert below, "a group with chain members but not the head"
    # of these groups the one with the most members of the chain
    one = max((1 << k for k in range(32) if below >> k & 1), key=lambda bit: sum(1 for x in member_masks if x & bit))
    assert sum(1 for x in member_masks if x & one) >= 3
    n = 1 << 16
    text = np.frombuffer((pat * (n // len(pat) + 1))[:n], dtype=np.uint8).copy()
    cuts = input_t("merged")[1]
    assert cuts[-1] == n
    rt, ac = gmatcher("merged", "rt"), gmatcher("merged", "ac")
    try:
        cases = [(np.array([0, n], dtype=np.int64), np.array([ALL_GROUPS], np.uint32)),
                 (np.array([0, n], dtype=np.int64), np.array([one], np.uint32)),
                 (np.asarray(cuts, dtype=np.int64),
                  np.array([ALL_GROUPS if j & 1 else one for j in range(len(cuts) - 1)], np.uint32))]
        for offs, sg in cases:
            exp = oracle_per_stream("merged", text, offs)
            for all_matches in (True, False):
                want = expected_groups("merged", exp, offs, sg, 1, all_matches)
                assert len(want[0]) > n // 4
                what = f"{len(offs) - 1} streams, mask {int(sg[0]):#x}, all {all_matches}"
                for small_max in (-1, 0):
                    assert rt.set_option("rt_small_max", small_max) == 0
                    ev = _batch_groups(rt, torch, text, offs, sg, 1, all_matches, Ev(torch, len(want[0])))
                    _assert_complete(rt, ev, want, f"batch, {what}, small_max {small_max}")
                ev = _flow_groups(ac, torch, text, offs, None, None, sg, 1, all_matches, Ev(torch, len(want[0])))
                _assert_complete(ac, ev, want, f"flows, {what}")
    finally:
        rt.set_option("rt_small_max", -1)


# ---- 4. flow segment seams ------------------------------------------------------------
@pytest.mark.parametrize("n", [600 * 1024, 600 * 1024 - 5])
def test_flow_groups_segment_seams(n):
    """test_flow_events_segment_seams' two-call text and offsets with the
    lane segment forced to 16 and 1,024: masks by TABLE, the all form at
    min_len 1."""
    torch = _torch()
    offs = np.unique(np.minimum(_seam_offsets(600 * 1024), n))
    nseg = len(offs) - 1
    sg = stream_masks(nseg)
    d = pm.Dictionary(dict_paths("snort"))
    texts = [(pm.gen_stream(n, seed=9, mode=0), pm.gen_stream(n, seed=10, mode=0)),
             (d.gen_lines(n, 9), d.gen_lines(n, 10))]
    expect = [_oracle_two_calls("snort", A, B, offs) for A, B in texts]
    m = gmatcher("snort", "ac")
    try:
        for seg in (16, 1024):
            assert m.set_option("flow_seg", seg) == 0
            for (A, B), (ea, eb) in zip(texts, expect):
                s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                want = expected_groups("snort", ea, offs, sg, 1, True)
                ev = _flow_groups(m, torch, A, offs, None, s1, sg, 1, True, Ev(torch, len(want[0])))
                _assert_complete(m, ev, want, f"seg {seg} call 1")
                want = expected_groups("snort", eb, offs, sg, 1, True)
                ev = _flow_groups(m, torch, B, offs, s1, s2, sg, 1, True, Ev(torch, len(want[0])))
                _assert_complete(m, ev, want, f"seg {seg} call 2")
    finally:
        m.set_option("flow_seg", 0)


# ---- 5. capacity and append -------------------------------------------------------------
def _check_capacity(torch, m, run, want_list):
    pos, codes = want_list
    total = len(pos)
    assert total > 8
    want = set(zip(pos.tolist(), codes.tolist()))
    assert len(want) == total
    for cap, null in [(0, True), (0, False), (1, False), (total // 2, False), (total - 1, False), (total, False),
                      (total + 7, False)]:
        ev = Ev(torch, cap)
        if null:  # count only: no list at all
            ev.buf = torch.zeros(0, dtype=torch.int64, device="cuda")
            assert ev.buf.data_ptr() == 0
            run(ev)
            assert ev.total() == total
            continue
        run(ev)
        assert ev.total() == total, cap
        kept = min(cap, total)
        p, g = pm.unpack_events(ev.slots()[:kept])
        got = list(zip(p.tolist(), m._codes[g].tolist()))
        assert len(set(got)) == kept and set(got) <= want, cap
        ev.assert_guard(kept)
    # a non-zero starting cursor appends: the slots before it stay, the list follows
    ev = Ev(torch, total + 5, cursor=5)
    run(ev)
    _assert_complete(m, ev, want_list, "append", start=5)


def test_batch_groups_capacity_and_append():
    torch = _torch()
    text, offs, exp = input_t("et")
    sg = stream_masks(len(offs) - 1)
    m = gmatcher("et", "rt")
    try:
        for small_max in (-1, 0):
            assert m.set_option("rt_small_max", small_max) == 0
            for all_matches in (True, False):
                _check_capacity(torch, m, lambda ev: _batch_groups(m, torch, text, offs, sg, 3, all_matches, ev),
                                expected_groups("et", exp, offs, sg, 3, all_matches))
    finally:
        m.set_option("rt_small_max", -1)


def test_flow_groups_capacity_and_append():
    torch = _torch()
    F = input_f("et")
    m = gmatcher("et", "ac")
    sg = stream_masks(F_FLOWS)
    d0, o0, _ = F.calls[16]
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    s_a = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    # fresh flows: the expected list of call 16 from each packet's first byte
    exp0 = oracle_per_stream("et", d0, o0)
    for all_matches in (True, False):
        _check_capacity(torch, m, lambda ev: _flow_groups(m, torch, d0, o0, zero, s_a, sg, 3, all_matches, ev),
                        expected_groups("et", exp0, o0, sg, 3, all_matches))


# ---- 6. errors and degenerate inputs --------------------------------------------------------
def test_groups_errors_and_degenerates():
    torch = _torch()
    F = input_f("et")
    data, offs, exp = F.calls[3]
    n = len(data)
    d_text, d_offs = _text_dev(torch, data), _dev(torch, offs)
    s_in = _states(torch, np.arange(F_FLOWS, dtype=np.uint32) % 7)
    s_out = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    d_sg = _states(torch, stream_masks(F_FLOWS))
    s = _stream(torch)
    rt, ac = gmatcher("et", "rt"), gmatcher("et", "ac")
    fb, ff = rt.lib.pm_hip_scan_batch_groups_device, rt.lib.pm_hip_scan_flows_groups_device
    ev = Ev(torch, n)
    t, o, e, c, g = d_text.data_ptr(), d_offs.data_ptr(), ev.buf.data_ptr(), ev.nev.data_ptr(), d_sg.data_ptr()
    si, so = s_in.data_ptr(), s_out.data_ptr()

    def untouched(m, last):
        torch.cuda.synchronize()
        assert ev.total() == 0
        ev.assert_guard(0)
        assert np.all(_state_values(s_out) == STATE_POISON)
        assert m.kernel_last == last  # nothing launched

    for m in (rt, ac):
        m.read_block_codes(SHIP[:4096])
    last_rt, last_ac = rt.kernel_last, ac.kernel_last
    # before pm_hip_set_groups: -7, nothing launched or written; the siblings still run
    for kind in ("rt", "ac"):
        raw = pm.HipMatcher(kind)
        raw.add_pattern(b"abcd")
        raw.add_pattern(b"bcd")
        raw.compile()
        tb = raw.table_bytes
        assert raw.pattern_groups(1) == 0
        raw.read_block_gids(SHIP[:4096])
        last = raw.kernel_last
        if kind == "rt":
            assert fb(raw.obj, t, o, F_FLOWS, n, g, 3, 1, e, n, c, s) == -7
        else:
            assert ff(raw.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s) == -7
        assert b"pm_hip_set_groups" in raw.lib.pm_hip_last_error()
        untouched(raw, last)
        h_ev, h_n = np.full(8, POISON64, np.uint64), ctypes.c_size_t(77)
        hg = stream_masks(F_FLOWS)
        hfn, extra = ((raw.lib.pm_hip_read_batch_groups, ()) if kind == "rt"
                      else (raw.lib.pm_hip_read_flows_groups, (None,)))
        assert hfn(raw.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS, *extra,
                   hg.ctypes.data_as(U32P), 3, 1, h_ev.ctypes.data_as(U64P), 8, ctypes.byref(h_n)) == -7
        assert h_n.value == 77 and np.all(h_ev == POISON64)
        assert raw.table_bytes == tb
        # pm_hip_set_groups: n wrong, NULL groups
        two = np.array([1, 2], np.uint32)
        assert raw.lib.pm_hip_set_groups(raw.obj, two.ctypes.data_as(U32P), 1) == -2
        assert raw.lib.pm_hip_set_groups(raw.obj, two.ctypes.data_as(U32P), 3) == -2
        assert raw.lib.pm_hip_set_groups(raw.obj, None, 2) == -2
        assert raw.table_bytes == tb and raw.pattern_groups(1) == 0
        with pytest.raises(RuntimeError, match="bad arguments"):
            raw.set_groups(np.array([1], np.uint32))
        raw.set_groups(two)
        assert raw.table_bytes == tb + 2 * 3 * 4
        assert sorted(raw.pattern_groups(k) for k in (1, 2)) == [1, 2]
        assert raw.pattern_groups(0) == 0 and raw.pattern_groups(3) == 0
        raw.free()
    # before compile(): -1
    raw = pm.HipMatcher("auto")
    raw.add_pattern(b"abcd")
    one = np.array([1], np.uint32)
    assert raw.lib.pm_hip_set_groups(raw.obj, one.ctypes.data_as(U32P), 1) == -1
    assert fb(raw.obj, t, o, F_FLOWS, n, g, 3, 1, e, n, c, s) == -1
    assert ff(raw.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s) == -1
    raw.free()
    untouched(ac, last_ac)
    # the kind without the needed image: -6
    assert fb(ac.obj, t, o, F_FLOWS, n, g, 3, 1, e, n, c, s) == -6
    assert b"reverse-trie image" in ac.lib.pm_hip_last_error()
    untouched(ac, last_ac)
    assert ff(rt.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s) == -6
    assert b"DFA image" in rt.lib.pm_hip_last_error()
    untouched(rt, last_rt)
    with pytest.raises(RuntimeError, match="DFA image"):
        rt.scan_flows_groups_device(t, o, F_FLOWS, n, si, so, g, 3, True, e, n, c, s)
    # bad arguments: -2, as the siblings, and a misaligned d_stream_groups
    for bad in [dict(min_len=0), dict(c=None), dict(e=e + 4), dict(c=c + 4), dict(e=None, cap=4), dict(t=t + 1),
                dict(o=o + 4), dict(nseg=-1), dict(n=-1), dict(n=(1 << 40) + 1), dict(g=g + 2), dict(g=g + 1)]:
        a = dict(t=t, o=o, nseg=F_FLOWS, n=n, min_len=3, e=e, cap=n, c=c, g=g)
        a.update(bad)
        for all_matches in (0, 1):
            assert fb(rt.obj, a["t"], a["o"], a["nseg"], a["n"], a["g"], a["min_len"], all_matches, a["e"], a["cap"],
                      a["c"], s) == -2, bad
            assert ff(ac.obj, a["t"], a["o"], a["nseg"], a["n"], si, so, a["g"], a["min_len"], all_matches, a["e"],
                      a["cap"], a["c"], s) == -2, bad
    assert ff(ac.obj, t, o, F_FLOWS, n, so, so, g, 3, 1, e, n, c, s) == -2
    assert ff(ac.obj, t, o, F_FLOWS, n, si + 2, so, g, 3, 1, e, n, c, s) == -2
    with pytest.raises(RuntimeError, match="bad arguments"):
        rt.scan_batch_groups_device(t, o, F_FLOWS, n, g, 0, True, e, n, c, s)
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # nseg == 0: 0, nothing launched, nothing written
    assert fb(rt.obj, t, o, 0, 0, g, 3, 1, e, n, c, s) == 0
    assert ff(ac.obj, t, o, 0, 0, si, so, g, 3, 1, e, n, c, s) == 0
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # n == 0 with streams: the batch form launches nothing; the flow form copies the states
    zoffs = _dev(torch, np.zeros(F_FLOWS + 1, np.int64))
    assert fb(rt.obj, t, zoffs.data_ptr(), F_FLOWS, 0, g, 3, 1, e, n, c, s) == 0
    untouched(rt, last_rt)
    assert ff(ac.obj, t, zoffs.data_ptr(), F_FLOWS, 0, si, so, g, 3, 1, e, n, c, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_state_values(s_out), _state_values(s_in))
    assert ev.total() == 0
    ev.assert_guard(0)
    # NULL d_stream_groups: every stream on all groups
    ones = np.full(F_FLOWS, ALL_GROUPS, np.uint32)
    fresh = oracle_per_stream("et", data, offs)
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    for all_matches in (True, False):
        want = expected_groups("et", fresh, offs, ones, 1, all_matches)
        assert len(want[0]) > 0
        got = _batch_groups(rt, torch, data, offs, None, 1, all_matches, Ev(torch, len(want[0])))
        _assert_complete(rt, got, want, f"batch, no stream masks, all {all_matches}")
        got = _flow_groups(ac, torch, data, offs, zero, None, None, 1, all_matches, Ev(torch, len(want[0])))
        _assert_complete(ac, got, want, f"flows, no stream masks, all {all_matches}")


# ---- 7. host forms and Python, the relaunch forced ---------------------------------------------
def _read_raw(m, flows, data, offs, state, sg, min_len, all_matches, cap):
    """The C host form: (rc, events as filled + 8 guard slots, total)."""
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(0)
    head = (m.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), len(offs) - 1)
    tail = (sg.ctypes.data_as(U32P), min_len, int(all_matches), ev.ctypes.data_as(U64P), cap, ctypes.byref(total))
    if flows:
        rc = m.lib.pm_hip_read_flows_groups(*head, None if state is None else state.ctypes.data_as(U32P), *tail)
    else:
        rc = m.lib.pm_hip_read_batch_groups(*head, *tail)
    return rc, ev, total.value


def _assert_host_list(pos_codes, want):
    """A Python host form's (positions, codes): position order, and exact."""
    p, c = pos_codes
    assert np.all(np.diff(p) >= 0)
    sp, sc = sort_matches(p, c)
    assert np.array_equal(sp, want[0]) and np.array_equal(sc, want[1])


def test_batch_groups_host_forms():
    text, offs, exp = input_t("et")
    sg = stream_masks(len(offs) - 1)
    m = gmatcher("et", "rt")
    try:
        for cap_opt in (0, 16):  # 16: the first launch's list is too short, the second one's complete
            assert m.set_option("events_cap", cap_opt) == 0
            for all_matches in (True, False):
                want = expected_groups("et", exp, offs, sg, 3, all_matches)
                total = len(want[0])
                _assert_host_list(m.read_batch_groups(text, offs, sg, all_matches=all_matches), want)
                assert m.kernel_last == pm.KIND_RT
                # the C form: ascending as plain u64 (position, then gid), no event twice
                rc, ev, t = _read_raw(m, False, text, offs, None, sg, 3, all_matches, total)
                assert rc == 0 and t == total and np.all(ev[total:] == POISON64)
                assert np.all(ev[1:total] > ev[:total - 1])
                _assert_list(m, ev[:total], want, f"events_cap {cap_opt}")
                # a caller cap below the total: the first cap of that order, and the true total
                cap = total // 3
                rc, short, t = _read_raw(m, False, text, offs, None, sg, 3, all_matches, cap)
                assert rc == 0 and t == total
                assert np.array_equal(short[:cap], ev[:cap]) and np.all(short[cap:] == POISON64)
        # read_many_groups: per stream, positions inside it (events_cap is 16: every call relaunches)
        bufs = [text[a:b] for a, b in zip(offs[:-1], offs[1:])]
        many = m.read_many_groups(bufs, sg, min_len=1)
        assert len(many) == len(bufs)
        for j, ((p, c), a, b) in enumerate(zip(many, offs[:-1], offs[1:])):
            _assert_host_list((p, c), expected_groups("et", exp[a:b], [0, b - a], sg[j:j + 1], 1, True))
        # count only, and refused inputs: -2, nothing written
        total = len(expected_groups("et", exp, offs, sg, 3, True)[0])
        rc, ev, t = _read_raw(m, False, text, offs, None, sg, 3, True, 0)
        assert rc == 0 and t == total and np.all(ev == POISON64)
        bad = np.array([0, 10, 5, len(text)], dtype=np.int64)
        rc, ev, t = _read_raw(m, False, text, bad, None, sg, 3, True, 8)
        assert rc == -2 and np.all(ev == POISON64)
        rc, ev, t = _read_raw(m, False, text, offs, None, sg, 0, True, 8)
        assert rc == -2 and np.all(ev == POISON64)
        with pytest.raises(ValueError, match="stream_groups"):
            m.read_batch_groups(text, offs, sg[:-1])
    finally:
        m.set_option("events_cap", 0)


def test_flow_groups_host_forms():
    F = input_f("et")
    m = gmatcher("et", "ac")
    sg = stream_masks(F_FLOWS)
    calls = F.calls[:12]
    try:
        runs = {}
        for cap_opt in (0, 16):
            assert m.set_option("events_cap", cap_opt) == 0
            state, out = None, []
            for r, (data, offs, exp) in enumerate(calls):
                all_matches = bool(r & 1)
                p, c, new = m.read_flows_groups(data, offs, sg, state, all_matches=all_matches)
                _assert_host_list((p, c), expected_groups("et", exp, offs, sg, 3, all_matches))
                assert new is not state and new.dtype == np.uint32 and new.shape == (F_FLOWS,)
                state = new
                out.append(new)
            runs[cap_opt] = out
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        # the states are those of the dense host form, relaunch or not
        state = None
        for r, (data, offs, exp) in enumerate(calls):
            _, state = m.read_flows_gids(data, offs, state)
            assert np.array_equal(state, runs[0][r]) and np.array_equal(state, runs[16][r]), r
        # (events_cap is 16 from here on: every call below relaunches)
        # a caller cap below the total, from given states: sorted, the true
        # total, and the complete scan's states
        data, offs, exp = F.calls[12]
        want = expected_groups("et", exp, offs, sg, 3, True)
        st = runs[0][11].copy()
        cap = len(want[0]) // 2
        assert cap > 4
        rc, ev, total = _read_raw(m, True, data, offs, st, sg, 3, True, cap)
        assert rc == 0 and total == len(want[0])
        assert np.all(ev[1:cap] > ev[:cap - 1]) and np.all(ev[cap:] == POISON64)
        gp, gg = pm.unpack_events(ev[:cap])
        assert set(zip(gp.tolist(), m._codes[gg].tolist())) <= set(zip(want[0].tolist(), want[1].tolist()))
        assert np.array_equal(gp, want[0][:cap])
        _, dense = m.read_flows_gids(data, offs, runs[0][11])
        assert np.array_equal(st, dense)
        # a wild state: -2, nothing written
        wild = runs[0][11].copy()
        wild[5] = m.flow_states
        keep = wild.copy()
        rc, ev, total = _read_raw(m, True, data, offs, wild, sg, 3, True, 8)
        assert rc == -2 and np.all(ev == POISON64) and np.array_equal(wild, keep)
        # FlowTable.scan_groups: the same packets, the flows in another order every call
        flows = pm.FlowTable(m)
        rng = np.random.default_rng(3)
        for r, (data, offs, exp) in enumerate(calls[:6]):
            order = rng.permutation(F_FLOWS)
            all_matches = bool(r & 1)
            got = flows.scan_groups([(("flow", int(f)), data[offs[f]:offs[f + 1]], TABLE[f % 14]) for f in order],
                                    min_len=2, all_matches=all_matches)
            for f, (p, c) in zip(order.tolist(), got):
                a, b = int(offs[f]), int(offs[f + 1])
                _assert_host_list((p, c), expected_groups("et", exp[a:b], [0, b - a], [TABLE[f % 14]], 2,
                                                          all_matches))
        assert len(flows) == F_FLOWS
        with pytest.raises(ValueError, match="twice"):
            flows.scan_groups([("a", b"xx", 1), ("a", b"yy", 1)])
        # scan_groups() advances the flows as scan() does
        a, b = pm.FlowTable(m), pm.FlowTable(m)
        d6, o6, _ = F.calls[6]
        for tab in (a, b):
            tab.states = {f: int(s) for f, s in enumerate(runs[0][5])}
        a.scan_groups([(f, d6[o6[f]:o6[f + 1]], TABLE[f % 14]) for f in range(F_FLOWS)])
        b.scan([(f, d6[o6[f]:o6[f + 1]]) for f in range(F_FLOWS)])
        assert a.states == b.states
    finally:
        m.set_option("events_cap", 0)


def test_set_groups_again_replaces_the_tables_in_place():
    """A rule reload: the second table's lists hold and table_bytes grew once."""
    text, offs, exp = input_t("et")
    sg = stream_masks(len(offs) - 1)
    m = fresh_matcher("et", "auto")
    try:
        tb = m.table_bytes
        npat = len(m._dict.patterns())
        first, second = masks_by_index(m._dict), masks_by_index(m._dict, reversed_mask)
        assert np.count_nonzero(first != second) > npat // 2
        m.set_groups(first)
        assert m.table_bytes == tb + 2 * 4 * (npat + 1)
        for fn, masks in ((pattern_mask, first), (reversed_mask, second), (pattern_mask, first)):
            m.set_groups(masks)
            assert m.table_bytes == tb + 2 * 4 * (npat + 1)
            gid = int(np.nonzero(m._codes == m._dict.codes()[7])[0][0])
            assert m.pattern_groups(gid) == int(masks[7])
            for all_matches in (True, False):
                want = expected_groups("et", exp, offs, sg, 1, all_matches, fn)
                _assert_host_list(m.read_batch_groups(text, offs, sg, 1, all_matches), want)
                p, c, _ = m.read_flows_groups(text, offs, sg, None, 1, all_matches)
                _assert_host_list((p, c), want)
    finally:
        m.free()


# ---- 8. cross-checks, device against device ------------------------------------------------------
def test_all_ones_masks_are_the_matches_and_the_events_calls():
    torch = _torch()
    text, offs, exp = input_t("merged")
    nseg = len(offs) - 1
    rt = gmatcher("merged", "rt", all_ones)
    for sg in (np.full(nseg, ALL_GROUPS, np.uint32), np.full(nseg, 1 << 17, np.uint32)):
        for min_len in (1, 4):
            sib = _batch_matches(rt, torch, text, offs, min_len, Ev(torch, 2 * len(text)))
            got = _batch_groups(rt, torch, text, offs, sg, min_len, True, Ev(torch, 2 * len(text)))
            assert got.total() == sib.total() > 0
            assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))
            sib = _batch_events(rt, torch, text, offs, min_len)
            got = _batch_groups(rt, torch, text, offs, sg, min_len, False, Ev(torch, len(text)))
            assert got.total() == sib.total() > 0
            assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))
    F = input_f("merged")
    ac = gmatcher("merged", "ac", all_ones)
    data, offs, _ = F.calls[16]
    sg = np.full(F_FLOWS, ALL_GROUPS, np.uint32)
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    for min_len in (1, 4):
        sib = _flow_matches(ac, torch, data, offs, zero, None, min_len, Ev(torch, 2 * len(data)))
        got = _flow_groups(ac, torch, data, offs, zero, None, sg, min_len, True, Ev(torch, 2 * len(data)))
        assert got.total() == sib.total() > 0
        assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))
        sib = _flow_events(ac, torch, data, offs, zero, None, min_len)
        got = _flow_groups(ac, torch, data, offs, zero, None, sg, min_len, False, Ev(torch, len(data)))
        assert got.total() == sib.total() > 0
        assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))


@pytest.mark.parametrize("k", [3, 8])
def test_one_group_is_the_sub_dictionarys_matcher(k):
    """Every stream on group k, longest form, min_len 1: the events list of a
    second matcher compiled from group k's patterns alone, by position and
    pattern bytes -- batched (rt) and as flows (ac) over three calls."""
    torch = _torch()
    pats = [b for _, _, b in oracle_for("et").patterns()]
    sub_pats = [b for b in pats if pattern_mask(b) >> k & 1]
    assert 50 < len(sub_pats) < len(pats) // 2
    bid = {b: n for n, b in enumerate(sorted(set(pats)))}
    by_code = {(f << 24) | l: bid[b] for f, l, b in oracle_for("et").patterns()}

    def sub_matcher(kind):
        m = pm.HipMatcher(kind)
        for b in sub_pats:
            m.add_pattern(b)
        m.compile()
        tab = np.zeros(len(sub_pats) + 1, np.int64)
        for g in range(1, len(sub_pats) + 1):
            tab[g] = bid[sub_pats[m.lib.pm_hip_gid_index(m.obj, g)]]
        return m, tab

    def same(main, ev, tab, sub_ev, what):
        p, g = pm.unpack_events(np.sort(ev.slots()[:ev.total()]))
        sp, sg_ = pm.unpack_events(np.sort(sub_ev.slots()[:sub_ev.total()]))
        assert len(p) == len(sp) > 0, what
        assert np.array_equal(p, sp), what
        assert np.array_equal(np.array([by_code[int(c)] for c in main._codes[g]], np.int64), tab[sg_]), what

    text, offs, _ = input_t("et")
    sg = np.full(len(offs) - 1, 1 << k, np.uint32)
    rt = gmatcher("et", "rt")
    sub, tab = sub_matcher("rt")
    try:
        ev = _batch_groups(rt, torch, text, offs, sg, 1, False, Ev(torch, len(text)))
        same(rt, ev, tab, _batch_events(sub, torch, text, offs, 1), "batch")
    finally:
        sub.free()
    F = input_f("et")
    sg = np.full(F_FLOWS, 1 << k, np.uint32)
    ac = gmatcher("et", "ac")
    sub, tab = sub_matcher("ac")
    try:
        poison = np.full(F_FLOWS, STATE_POISON, np.uint32)
        st = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
        sst = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
        for r, (data, offs, _) in enumerate(F.calls[16:19]):
            ev = _flow_groups(ac, torch, data, offs, st[r & 1], st[1 - (r & 1)], sg, 1, False, Ev(torch, len(data)))
            same(ac, ev, tab, _flow_events(sub, torch, data, offs, sst[r & 1], sst[1 - (r & 1)], 1), f"flows, call {r}")
    finally:
        sub.free()
