"""The all-matches list (pm_hip_scan_batch_matches_device,
pm_hip_scan_flows_matches_device, pm_hip_read_*_matches): an event for every
pattern of at least min_len bytes that ends at a position, not only the
longest.  Expected lists come from the oracle alone (tests/match_inputs.py:
suffixes by byte-string lookup over the oracle's patterns); lists are compared
after sorting, positions and the codes of the gids, exactly."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream
from flow_inputs import F_FLOWS, input_f
from match_inputs import deepest_pattern, expected_matches, longest_per_position, sort_matches
from oracle_lib import dict_paths
from test_batch import _dev, _stream
from test_events import I64P, POISON64, U8P, U32P, U64P, Ev, _assert_list, _batch_events, _flow_events, _text_dev
from test_flows import STATE_POISON, _flows, _oracle_two_calls, _seam_offsets, _state_values, _states
from test_gpu_parity import SHIP, _torch, matcher

pytestmark = pytest.mark.gpu


def _batch_matches(m, torch, text, offs, min_len, ev):
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text), min_len,
                                ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _flow_matches(m, torch, text, offs, st_in, st_out, min_len, ev):
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    m.scan_flows_matches_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text),
                                None if st_in is None else st_in.data_ptr(),
                                None if st_out is None else st_out.data_ptr(), min_len, ev.buf.data_ptr(), ev.cap,
                                ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _assert_matches(m, events, pos, codes, what):
    """events (u64, any order) == the expected list (ascending by position, code)."""
    events = np.asarray(events, dtype=np.uint64)
    assert len(events) == len(pos), f"{what}: {len(events)} events, expected {len(pos)}"
    got_pos, got_gid = pm.unpack_events(events)
    got_pos, got_codes = sort_matches(got_pos, m._codes[got_gid])
    assert np.array_equal(got_pos, pos), f"{what}: positions differ"
    assert np.array_equal(got_codes, codes), f"{what}: codes differ"


def _assert_complete(m, ev, key, exp, min_len, what, start=0):
    pos, codes = expected_matches(key, exp, min_len)
    assert start + len(pos) <= ev.cap
    assert ev.total() == start + len(pos), f"{what}: cursor {ev.total()}, expected {start + len(pos)}"
    slots = ev.slots()
    assert np.all(slots[:start] == POISON64)
    _assert_matches(m, slots[start:start + len(pos)], pos, codes, what)
    ev.assert_guard(start + len(pos))


def _room(key, exp, min_len, extra=0):
    """cap from the expected count: at min_len 1 the list is longer than the buffer."""
    return len(expected_matches(key, exp, min_len)[0]) + extra


# ---- 1. batched form, input T --------------------------------------------------
@pytest.mark.parametrize("min_len", [1, 3, 5])
@pytest.mark.parametrize("key,kind", [("et", "rt"), ("et", "auto"), ("merged", "rt")])
def test_batch_matches_input_t(key, kind, min_len):
    torch = _torch()
    text, offs, exp = input_t(key)
    m = matcher(key, kind)
    try:
        for small_max in (-1, 0):  # the one-tile-per-workgroup form, and one workgroup per CU
            assert m.set_option("rt_small_max", small_max) == 0
            ev = _batch_matches(m, torch, text, offs, min_len, Ev(torch, _room(key, exp, min_len)))
            _assert_complete(m, ev, key, exp, min_len, f"rt_small_max {small_max}")
            assert m.kernel_last == pm.KIND_RT and m.dfa_form_last == 0
    finally:
        m.set_option("rt_small_max", -1)


# ---- 2. flow form, every call of input F -----------------------------------------
@pytest.mark.parametrize("key,kind,min_len", [("et", "ac", 3), ("et", "ac", 8), ("et", "auto", 3), ("et", "auto", 8),
                                              ("merged", "ac", 3), ("merged", "ac", 8), ("et", "ac", 1)])
def test_flow_matches_input_f(key, kind, min_len):
    torch = _torch()
    F = input_f(key)
    m = matcher(key, kind)
    ping = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    dense = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    seen = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        ev = Ev(torch, _room(key, exp, min_len))
        _flow_matches(m, torch, data, offs, ping[r & 1], ping[1 - (r & 1)], min_len, ev)
        _assert_complete(m, ev, key, exp, min_len, f"call {r}")
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        _flows(m, torch, data, offs, dense[r & 1], dense[1 - (r & 1)])
        assert np.array_equal(_state_values(ping[1 - (r & 1)]), _state_values(dense[1 - (r & 1)])), r
        seen += ev.total()
    assert seen == len(expected_matches(key, F.exp, min_len)[0]) > 0


# ---- 3. direct path and flush ---------------------------------------------------------
def test_matches_deepest_chain_repeated():
    """64 KiB of merged's pattern with the deepest suffix chain, repeated
    without separators, at min_len 1: more than an event per position, so one
    wave step of the flow kernel (up to 1,024 positions) brings more events
    than its stage holds and takes the direct path, and the batched kernel's
    stage flushes inside its expansion rounds.  As one stream and cut at
    input T's offsets."""
    torch = _torch()
    pat, depth = deepest_pattern("merged")
    assert depth == 24
    n = 1 << 16
    text = np.frombuffer((pat * (n // len(pat) + 1))[:n], dtype=np.uint8).copy()
    cuts = input_t("merged")[1]
    assert cuts[-1] == n
    rt, ac = matcher("merged", "rt"), matcher("merged", "ac")
    try:
        for offs in (np.array([0, n], dtype=np.int64), np.asarray(cuts, dtype=np.int64)):
            exp = oracle_per_stream("merged", text, offs)
            total = _room("merged", exp, 1)
            assert total > 2 * n
            for small_max in (-1, 0):
                assert rt.set_option("rt_small_max", small_max) == 0
                ev = _batch_matches(rt, torch, text, offs, 1, Ev(torch, total))
                _assert_complete(rt, ev, "merged", exp, 1, f"batch, {len(offs) - 1} streams, small_max {small_max}")
            ev = _flow_matches(ac, torch, text, offs, None, None, 1, Ev(torch, total))
            _assert_complete(ac, ev, "merged", exp, 1, f"flows, {len(offs) - 1} streams")
    finally:
        rt.set_option("rt_small_max", -1)


# ---- 4. flow segment seams ------------------------------------------------------------
@pytest.mark.parametrize("n", [600 * 1024, 600 * 1024 - 5])
def test_flow_matches_segment_seams(n):
    """test_flow_events_segment_seams' two-call text and offsets with the
    lane segment forced to 16 and 1,024, on the all form at min_len 1."""
    torch = _torch()
    offs = np.unique(np.minimum(_seam_offsets(600 * 1024), n))
    nseg = len(offs) - 1
    d = pm.Dictionary(dict_paths("snort"))
    texts = [(pm.gen_stream(n, seed=9, mode=0), pm.gen_stream(n, seed=10, mode=0)),
             (d.gen_lines(n, 9), d.gen_lines(n, 10))]
    expect = [_oracle_two_calls("snort", A, B, offs) for A, B in texts]
    m = matcher("snort", "ac")
    try:
        for seg in (16, 1024):
            assert m.set_option("flow_seg", seg) == 0
            for (A, B), (ea, eb) in zip(texts, expect):
                s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                ev = _flow_matches(m, torch, A, offs, None, s1, 1, Ev(torch, _room("snort", ea, 1)))
                _assert_complete(m, ev, "snort", ea, 1, f"seg {seg} call 1")
                ev = _flow_matches(m, torch, B, offs, s1, s2, 1, Ev(torch, _room("snort", eb, 1)))
                _assert_complete(m, ev, "snort", eb, 1, f"seg {seg} call 2")
    finally:
        m.set_option("flow_seg", 0)


# ---- 5. capacity and append -------------------------------------------------------------
def _check_capacity(torch, m, key, run, exp, min_len):
    pos, codes = expected_matches(key, exp, min_len)
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
    _assert_complete(m, ev, key, exp, min_len, "append", start=5)


def test_batch_matches_capacity_and_append():
    torch = _torch()
    text, offs, exp = input_t("et")
    m = matcher("et", "rt")
    try:
        for small_max in (-1, 0):
            assert m.set_option("rt_small_max", small_max) == 0
            _check_capacity(torch, m, "et", lambda ev: _batch_matches(m, torch, text, offs, 3, ev), exp, 3)
    finally:
        m.set_option("rt_small_max", -1)


def test_flow_matches_capacity_and_append():
    torch = _torch()
    F = input_f("et")
    m = matcher("et", "ac")
    d0, o0, _ = F.calls[16]
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    s_a = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    # fresh flows: the expected list of call 16 from each packet's first byte
    exp0 = oracle_per_stream("et", d0, o0)
    _check_capacity(torch, m, "et", lambda ev: _flow_matches(m, torch, d0, o0, zero, s_a, 3, ev), exp0, 3)


# ---- 6. errors and degenerate inputs --------------------------------------------------------
def test_matches_errors_and_degenerates():
    torch = _torch()
    F = input_f("et")
    data, offs, _ = F.calls[3]
    n = len(data)
    d_text, d_offs = _text_dev(torch, data), _dev(torch, offs)
    s_in = _states(torch, np.arange(F_FLOWS, dtype=np.uint32) % 7)
    s_out = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    s = _stream(torch)
    rt, ac = matcher("et", "rt"), matcher("et", "ac")
    fb, ff = rt.lib.pm_hip_scan_batch_matches_device, rt.lib.pm_hip_scan_flows_matches_device
    ev = Ev(torch, n)
    t, o, e, c = d_text.data_ptr(), d_offs.data_ptr(), ev.buf.data_ptr(), ev.nev.data_ptr()
    si, so = s_in.data_ptr(), s_out.data_ptr()

    def untouched(m, last):
        torch.cuda.synchronize()
        assert ev.total() == 0
        ev.assert_guard(0)
        assert np.all(_state_values(s_out) == STATE_POISON)
        assert m.kernel_last == last  # nothing launched

    # the kind without the needed image: -6
    for m in (rt, ac):
        m.read_block_codes(SHIP[:4096])
    last_rt, last_ac = rt.kernel_last, ac.kernel_last
    assert fb(ac.obj, t, o, F_FLOWS, n, 3, e, n, c, s) == -6
    assert b"reverse-trie image" in ac.lib.pm_hip_last_error()
    untouched(ac, last_ac)
    assert ff(rt.obj, t, o, F_FLOWS, n, si, so, 3, e, n, c, s) == -6
    assert b"DFA image" in rt.lib.pm_hip_last_error()
    untouched(rt, last_rt)
    with pytest.raises(RuntimeError, match="DFA image"):
        rt.scan_flows_matches_device(t, o, F_FLOWS, n, si, so, 3, e, n, c, s)
    # bad arguments: -2, as the events siblings
    for bad in [dict(min_len=0), dict(c=None), dict(e=e + 4), dict(c=c + 4), dict(e=None, cap=4), dict(t=t + 1),
                dict(o=o + 4), dict(nseg=-1), dict(n=-1), dict(n=(1 << 40) + 1)]:
        a = dict(t=t, o=o, nseg=F_FLOWS, n=n, min_len=3, e=e, cap=n, c=c)
        a.update(bad)
        assert fb(rt.obj, a["t"], a["o"], a["nseg"], a["n"], a["min_len"], a["e"], a["cap"], a["c"], s) == -2, bad
        assert ff(ac.obj, a["t"], a["o"], a["nseg"], a["n"], si, so, a["min_len"], a["e"], a["cap"], a["c"],
                  s) == -2, bad
    assert ff(ac.obj, t, o, F_FLOWS, n, so, so, 3, e, n, c, s) == -2
    assert ff(ac.obj, t, o, F_FLOWS, n, si + 2, so, 3, e, n, c, s) == -2
    with pytest.raises(RuntimeError, match="bad arguments"):
        rt.scan_batch_matches_device(t, o, F_FLOWS, n, 0, e, n, c, s)
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # before compile(): -1
    raw = pm.HipMatcher("auto")
    raw.add_pattern(b"abcd")
    assert fb(raw.obj, t, o, F_FLOWS, n, 3, e, n, c, s) == -1
    assert ff(raw.obj, t, o, F_FLOWS, n, si, so, 3, e, n, c, s) == -1
    h_ev, h_n = np.full(8, POISON64, np.uint64), ctypes.c_size_t(77)
    for fn, extra in ((raw.lib.pm_hip_read_batch_matches, ()), (raw.lib.pm_hip_read_flows_matches, (None,))):
        assert fn(raw.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS, *extra, 3,
                  h_ev.ctypes.data_as(U64P), 8, ctypes.byref(h_n)) == -1
        assert h_n.value == 77 and np.all(h_ev == POISON64)
    raw.free()
    untouched(ac, last_ac)
    # nseg == 0: 0, nothing launched, nothing written
    assert fb(rt.obj, t, o, 0, 0, 3, e, n, c, s) == 0
    assert ff(ac.obj, t, o, 0, 0, si, so, 3, e, n, c, s) == 0
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # n == 0 with streams: the batch form launches nothing; the flow form copies the states
    zoffs = _dev(torch, np.zeros(F_FLOWS + 1, np.int64))
    assert fb(rt.obj, t, zoffs.data_ptr(), F_FLOWS, 0, 3, e, n, c, s) == 0
    untouched(rt, last_rt)
    assert ff(ac.obj, t, zoffs.data_ptr(), F_FLOWS, 0, si, so, 3, e, n, c, s) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_state_values(s_out), _state_values(s_in))
    assert ev.total() == 0
    ev.assert_guard(0)


# ---- 7. host forms and Python, the relaunch forced ---------------------------------------------
def _read_raw(m, flows, data, offs, state, min_len, cap):
    """The C host form: (rc, events as filled + 8 guard slots, total)."""
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(0)
    head = (m.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), len(offs) - 1)
    tail = (min_len, ev.ctypes.data_as(U64P), cap, ctypes.byref(total))
    if flows:
        rc = m.lib.pm_hip_read_flows_matches(*head, None if state is None else state.ctypes.data_as(U32P), *tail)
    else:
        rc = m.lib.pm_hip_read_batch_matches(*head, *tail)
    return rc, ev, total.value


def _assert_host_list(m, pos_codes, want):
    """A Python host form's (positions, codes): position order, and exact."""
    p, c = pos_codes
    assert np.all(np.diff(p) >= 0)
    sp, sc = sort_matches(p, c)
    assert np.array_equal(sp, want[0]) and np.array_equal(sc, want[1])


def test_batch_matches_host_forms():
    text, offs, exp = input_t("et")
    want = expected_matches("et", exp, 3)
    total = len(want[0])
    m = matcher("et", "rt")
    try:
        for cap_opt in (0, 16):  # 16: the first launch's list is too short, the second one's complete
            assert m.set_option("events_cap", cap_opt) == 0
            _assert_host_list(m, m.read_batch_matches(text, offs), want)
            assert m.kernel_last == pm.KIND_RT
            # the C form: ascending as plain u64 (position, then gid), no event twice
            rc, ev, t = _read_raw(m, False, text, offs, None, 3, total)
            assert rc == 0 and t == total and np.all(ev[total:] == POISON64)
            assert np.all(ev[1:total] > ev[:total - 1])
            _assert_matches(m, ev[:total], want[0], want[1], f"events_cap {cap_opt}")
            # a caller cap below the total: the first cap of that order, and the true total
            cap = total // 3
            rc, short, t = _read_raw(m, False, text, offs, None, 3, cap)
            assert rc == 0 and t == total
            assert np.array_equal(short[:cap], ev[:cap]) and np.all(short[cap:] == POISON64)
        # min_len 1: more events than bytes, from the default first capacity too
        m.set_option("events_cap", 0)
        _assert_host_list(m, m.read_batch_matches(text, offs, min_len=1), expected_matches("et", exp, 1))
        m.set_option("events_cap", 16)
        # read_many_matches: per stream, positions inside it
        bufs = [text[a:b] for a, b in zip(offs[:-1], offs[1:])]
        many = m.read_many_matches(bufs, min_len=5)
        assert len(many) == len(bufs)
        assert all(np.all((p >= 0) & (p < len(b))) for (p, _), b in zip(many, bufs))
        for (p, c), a, b in zip(many, offs[:-1], offs[1:]):
            _assert_host_list(m, (p, c), expected_matches("et", exp[a:b], 5))
        # count only, and refused inputs: -2, nothing written
        rc, ev, t = _read_raw(m, False, text, offs, None, 3, 0)
        assert rc == 0 and t == total and np.all(ev == POISON64)
        bad = np.array([0, 10, 5, len(text)], dtype=np.int64)
        rc, ev, t = _read_raw(m, False, text, bad, None, 3, 8)
        assert rc == -2 and np.all(ev == POISON64)
        rc, ev, t = _read_raw(m, False, text, offs, None, 0, 8)
        assert rc == -2 and np.all(ev == POISON64)
    finally:
        m.set_option("events_cap", 0)


def test_flow_matches_host_forms():
    F = input_f("et")
    m = matcher("et", "ac")
    calls = F.calls[:12]
    try:
        runs = {}
        for cap_opt in (0, 16):
            assert m.set_option("events_cap", cap_opt) == 0
            state, out = None, []
            for r, (data, offs, exp) in enumerate(calls):
                p, c, new = m.read_flows_matches(data, offs, state)
                _assert_host_list(m, (p, c), expected_matches("et", exp, 3))
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
        want = expected_matches("et", exp, 3)
        st = runs[0][11].copy()
        cap = len(want[0]) // 2
        rc, ev, total = _read_raw(m, True, data, offs, st, 3, cap)
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
        rc, ev, total = _read_raw(m, True, data, offs, wild, 3, 8)
        assert rc == -2 and np.all(ev == POISON64) and np.array_equal(wild, keep)
        # FlowTable.scan_matches: the same packets, the flows in another order every call
        flows = pm.FlowTable(m)
        rng = np.random.default_rng(3)
        for r, (data, offs, exp) in enumerate(calls[:6]):
            order = rng.permutation(F_FLOWS)
            got = flows.scan_matches([(("flow", int(f)), data[offs[f]:offs[f + 1]]) for f in order], min_len=4)
            for f, (p, c) in zip(order.tolist(), got):
                _assert_host_list(m, (p, c), expected_matches("et", exp[offs[f]:offs[f + 1]], 4))
        assert len(flows) == F_FLOWS
        with pytest.raises(ValueError, match="twice"):
            flows.scan_matches([("a", b"xx"), ("a", b"yy")])
        # scan_matches() then scan() continues the flows as two scan() calls would
        a, b = pm.FlowTable(m), pm.FlowTable(m)
        (d6, o6, _), (d7, o7, _) = F.calls[6], F.calls[7]
        for tab in (a, b):
            tab.states = {f: int(s) for f, s in enumerate(runs[0][5])}
        pk6 = [(f, d6[o6[f]:o6[f + 1]]) for f in range(F_FLOWS)]
        pk7 = [(f, d7[o7[f]:o7[f + 1]]) for f in range(F_FLOWS)]
        a.scan_matches(pk6)
        b.scan(pk6)
        assert a.states == b.states
        for x, y in zip(a.scan(pk7), b.scan(pk7)):
            assert np.array_equal(x, y)
        assert a.states == b.states
    finally:
        m.set_option("events_cap", 0)


# ---- 8. cross-check against the events call ------------------------------------------------------
def test_matches_reduce_to_the_events_call():
    """The all list reduced to the longest pattern per position is the
    sibling events call's list on the same input (device against device)."""
    torch = _torch()
    text, offs, exp = input_t("merged")
    rt = matcher("merged", "rt")
    for min_len in (1, 4):
        allv = _batch_matches(rt, torch, text, offs, min_len, Ev(torch, _room("merged", exp, min_len)))
        one = _batch_events(rt, torch, text, offs, min_len)
        p, g = pm.unpack_events(allv.slots()[:allv.total()])
        hp, hc = longest_per_position("merged", *sort_matches(p, rt._codes[g]))
        _assert_list(rt, one.slots()[:one.total()], hp, hc, f"batch min_len {min_len}")
        assert allv.total() > one.total() > 0
    F = input_f("merged")
    ac = matcher("merged", "ac")
    data, offs, exp = F.calls[16]
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    for min_len in (1, 4):
        fresh = oracle_per_stream("merged", data, offs)
        allv = _flow_matches(ac, torch, data, offs, zero, None, min_len, Ev(torch, _room("merged", fresh, min_len)))
        one = _flow_events(ac, torch, data, offs, zero, None, min_len)
        p, g = pm.unpack_events(allv.slots()[:allv.total()])
        hp, hc = longest_per_position("merged", *sort_matches(p, ac._codes[g]))
        _assert_list(ac, one.slots()[:one.total()], hp, hc, f"flows min_len {min_len}")
        assert allv.total() > one.total() > 0
