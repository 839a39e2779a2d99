"""The match list (pm_hip_scan_batch_events_device, pm_hip_scan_flows_events_device,
pm_hip_read_*_events): a compacted array of (position, gid) events for the
positions whose answer has at least min_len bytes.  Expected lists come from
the oracle alone (tests/event_inputs.py); lists are compared after sorting,
positions and the codes of the gids, exactly."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream
from event_inputs import code_lengths, expected_events
from flow_inputs import F_FLOWS, input_f
from oracle_lib import dict_paths, oracle_for
from test_batch import _dev, _stream
from test_flows import STATE_POISON, _flows, _oracle_two_calls, _seam_offsets, _state_values, _states
from test_gpu_parity import SHIP, _torch, matcher

pytestmark = pytest.mark.gpu

U8P = ctypes.POINTER(ctypes.c_uint8)
U32P = ctypes.POINTER(ctypes.c_uint32)
U64P = ctypes.POINTER(ctypes.c_uint64)
I64P = ctypes.POINTER(ctypes.c_int64)
POISON64 = 0xA5A5A5A5A5A5A5A5
GUARD = 64  # poisoned events past cap that must stay untouched


class Ev:
    """A device events buffer of cap slots + GUARD poisoned ones, and its cursor."""

    def __init__(self, torch, cap, cursor=0):
        self.cap = cap
        self.buf = torch.full((cap + GUARD,), POISON64 - (1 << 64), dtype=torch.int64, device="cuda")
        self.nev = torch.full((1,), cursor, dtype=torch.int64, device="cuda")

    def total(self):
        return int(self.nev.item())

    def slots(self):
        return self.buf.cpu().numpy().view(np.uint64)

    def assert_guard(self, used):
        """Nothing at or past slot `used` (<= cap) was written."""
        assert np.all(self.slots()[used:] == POISON64)


def _text_dev(torch, text):
    return _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))


def _batch_events(m, torch, text, offs, min_len, ev=None, cap=None):
    """One device batch events call into ev (a fresh one of cap slots when
    None; cap None: room for every position).  Returns ev."""
    n = len(text)
    if ev is None:
        ev = Ev(torch, n if cap is None else cap)
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    m.scan_batch_events_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, n, min_len, ev.buf.data_ptr(),
                               ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _flow_events(m, torch, text, offs, st_in, st_out, min_len, ev=None, cap=None):
    n = len(text)
    if ev is None:
        ev = Ev(torch, n if cap is None else cap)
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    m.scan_flows_events_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, n,
                               None if st_in is None else st_in.data_ptr(),
                               None if st_out is None else st_out.data_ptr(), min_len, ev.buf.data_ptr(), ev.cap,
                               ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _assert_list(m, events, pos, codes, what):
    """events (u64, any order) == the expected list (pos ascending, codes)."""
    got_pos, got_gid = pm.unpack_events(np.sort(events))
    assert len(got_pos) == len(pos), f"{what}: {len(got_pos)} events, expected {len(pos)}"
    assert np.array_equal(got_pos, pos), f"{what}: positions differ"
    assert np.array_equal(m._codes[got_gid], codes), f"{what}: codes differ"


def _assert_complete(m, ev, key, exp, min_len, what):
    pos, codes = expected_events(key, exp, min_len)
    assert len(pos) <= ev.cap
    assert ev.total() == len(pos), f"{what}: cursor {ev.total()}, expected {len(pos)}"
    _assert_list(m, ev.slots()[:len(pos)], pos, codes, what)
    ev.assert_guard(len(pos))


# ---- 1. batch events, input T ------------------------------------------------
@pytest.mark.parametrize("min_len", [1, 3, 5])
@pytest.mark.parametrize("key,kind", [("et", "rt"), ("et", "auto"), ("merged", "rt")])
def test_batch_events_input_t(key, kind, min_len):
    torch = _torch()
    text, offs, exp = input_t(key)
    assert len(expected_events(key, exp, min_len)[0]) > 0
    m = matcher(key, kind)
    try:
        for small_max in (-1, 0):  # the one-tile-per-workgroup form, and one workgroup per CU
            assert m.set_option("rt_small_max", small_max) == 0
            ev = _batch_events(m, torch, text, offs, min_len)
            _assert_complete(m, ev, key, exp, min_len, f"rt_small_max {small_max}")
            assert m.kernel_last == pm.KIND_RT and m.dfa_form_last == 0
    finally:
        m.set_option("rt_small_max", -1)


# ---- 2. flow events, input F ---------------------------------------------------
@pytest.mark.parametrize("key,kind,min_len", [("et", "ac", 3), ("et", "ac", 8), ("et", "auto", 3), ("et", "auto", 8),
                                              ("merged", "ac", 4)])
def test_flow_events_input_f(key, kind, min_len):
    torch = _torch()
    F = input_f(key)
    m = matcher(key, kind)
    ping = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    dense = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    seen = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        ev = _flow_events(m, torch, data, offs, ping[r & 1], ping[1 - (r & 1)], min_len)
        _assert_complete(m, ev, key, exp, min_len, f"call {r}")
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        _flows(m, torch, data, offs, dense[r & 1], dense[1 - (r & 1)])
        assert np.array_equal(_state_values(ping[1 - (r & 1)]), _state_values(dense[1 - (r & 1)])), r
        seen += ev.total()
    assert seen == len(expected_events(key, F.exp, min_len)[0]) > 0


# ---- 3. seams --------------------------------------------------------------------
@pytest.mark.parametrize("n", [600 * 1024, 600 * 1024 - 5])
def test_flow_events_segment_seams(n):
    """test_flows_segment_seams' two-call text and offsets (1-byte streams,
    ends at +-1 around multiples of 16, 32 and 1,024) with the lane segment
    forced; also with n not a multiple of 16."""
    torch = _torch()
    offs = np.unique(np.minimum(_seam_offsets(600 * 1024), n))
    nseg = len(offs) - 1
    d = pm.Dictionary(dict_paths("snort"))
    texts = [(pm.gen_stream(n, seed=9, mode=0), pm.gen_stream(n, seed=10, mode=0)),
             (d.gen_lines(n, 9), d.gen_lines(n, 10))]
    expect = [_oracle_two_calls("snort", A, B, offs) for A, B in texts]
    m = matcher("snort", "ac")
    try:
        for seg in (0, 16, 64, 4096):
            assert m.set_option("flow_seg", seg) == 0
            for (A, B), (ea, eb) in zip(texts, expect):
                s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                ev = _flow_events(m, torch, A, offs, None, s1, 3)
                _assert_complete(m, ev, "snort", ea, 3, f"seg {seg} call 1")
                ev = _flow_events(m, torch, B, offs, s1, s2, 3)
                _assert_complete(m, ev, "snort", eb, 3, f"seg {seg} call 2")
    finally:
        m.set_option("flow_seg", 0)


# ---- 4. capacity -------------------------------------------------------------------
def _check_capacity(torch, m, key, run, exp, min_len):
    pos, codes = expected_events(key, exp, min_len)
    total = len(pos)
    assert total > 8
    want = set(zip(pos.tolist(), codes.tolist()))
    for cap, null in [(0, True), (0, False), (1, False), (total - 1, False), (total, False), (total + 7, False)]:
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


def test_batch_events_capacity_and_append():
    torch = _torch()
    text, offs, exp = input_t("et")
    m = matcher("et", "rt")
    try:
        for small_max in (-1, 0):
            assert m.set_option("rt_small_max", small_max) == 0
            _check_capacity(torch, m, "et", lambda ev: _batch_events(m, torch, text, offs, 3, ev=ev), exp, 3)
    finally:
        m.set_option("rt_small_max", -1)
    # append: a second buffer without zeroing the cursor gives the union
    text2 = np.ascontiguousarray(text[::-1])
    exp2 = oracle_per_stream("et", text2, offs)
    p1, c1 = expected_events("et", exp, 3)
    p2, c2 = expected_events("et", exp2, 3)
    ev = Ev(torch, len(p1) + len(p2))
    _batch_events(m, torch, text, offs, 3, ev=ev)
    assert ev.total() == len(p1)
    _batch_events(m, torch, text2, offs, 3, ev=ev)
    assert ev.total() == len(p1) + len(p2)
    slots = ev.slots()
    _assert_list(m, slots[:len(p1)], p1, c1, "first launch")
    _assert_list(m, slots[len(p1):len(p1) + len(p2)], p2, c2, "appended launch")
    ev.assert_guard(len(p1) + len(p2))


def test_flow_events_capacity_and_append():
    torch = _torch()
    F = input_f("et")
    m = matcher("et", "ac")
    (d0, o0, e0), (d1, o1, e1) = F.calls[16], F.calls[17]
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    s_a = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    # fresh flows: the expected list of call 16 from each packet's first byte
    exp0 = oracle_per_stream("et", d0, o0)
    _check_capacity(torch, m, "et", lambda ev: _flow_events(m, torch, d0, o0, zero, s_a, 3, ev=ev), exp0, 3)
    # append: call 17 from call 16's states, onto the same list
    o = oracle_for("et")
    exp1 = np.zeros(len(d1), np.uint32)
    for j in range(F_FLOWS):
        o.reset()
        both = o.scan_codes(np.concatenate([d0[o0[j]:o0[j + 1]], d1[o1[j]:o1[j + 1]]]))
        exp1[o1[j]:o1[j + 1]] = both[o0[j + 1] - o0[j]:]
    o.reset()
    p0, c0 = expected_events("et", exp0, 3)
    p1, c1 = expected_events("et", exp1, 3)
    ev = Ev(torch, len(p0) + len(p1))
    _flow_events(m, torch, d0, o0, zero, s_a, 3, ev=ev)
    _flow_events(m, torch, d1, o1, s_a, None, 3, ev=ev)
    assert ev.total() == len(p0) + len(p1)
    slots = ev.slots()
    _assert_list(m, slots[:len(p0)], p0, c0, "first launch")
    _assert_list(m, slots[len(p0):len(p0) + len(p1)], p1, c1, "appended launch")
    ev.assert_guard(len(p0) + len(p1))


# ---- 5. sparse input ---------------------------------------------------------------
def test_events_sparse_single_stream():
    """nseg == 1: 1 MiB of random ASCII with ~50 dictionary patterns planted,
    some ending at positions 0..2 (cut short by the stream's start or whole)
    and in the last 16 bytes; most waves emit nothing.  Both families."""
    torch = _torch()
    n = 1 << 20
    text = pm.gen_stream(n, seed=21, mode=0).copy()
    pats = [p[2] for p in oracle_for("snort").patterns()]
    rng = np.random.default_rng(8)
    long_pats = [p for p in pats if 6 <= len(p) <= 40]
    short3 = next(p for p in pats if len(p) == 3)
    places = {0: short3}  # ends at position 2
    for k in range(46):
        places[int(rng.integers(64, n - 4096))] = long_pats[int(rng.integers(0, len(long_pats)))]
    tail2 = long_pats[1]
    places[n - 9 - len(tail2)] = tail2  # ends inside the last 16 bytes
    tail = next(p for p in long_pats if len(p) <= 8)
    places[n - len(tail)] = tail  # ends at the last position
    for at, p in places.items():
        text[at:at + len(p)] = np.frombuffer(p, np.uint8)
    offs = np.array([0, n], dtype=np.int64)
    exp = oracle_per_stream("snort", text, offs)
    pos, codes = expected_events("snort", exp, 5)
    ends = {at + len(p) - 1 for at, p in places.items() if len(p) >= 5}
    assert ends <= set(pos.tolist()) and len(pos) < 200
    assert pos[-1] == n - 1 and np.count_nonzero(pos >= n - 16) >= 2
    p3, _ = expected_events("snort", exp, 3)
    assert 2 in p3.tolist()
    for kind in ("rt", "ac"):
        m = matcher("snort", kind)
        for min_len in (3, 5):
            if kind == "rt":
                for small_max in (-1, 0):
                    m.set_option("rt_small_max", small_max)
                    ev = _batch_events(m, torch, text, offs, min_len)
                    _assert_complete(m, ev, "snort", exp, min_len, f"rt {small_max} min_len {min_len}")
                m.set_option("rt_small_max", -1)
            else:
                ev = _flow_events(m, torch, text, offs, None, None, min_len)
                _assert_complete(m, ev, "snort", exp, min_len, f"ac min_len {min_len}")


# ---- 6. errors and degenerate inputs -----------------------------------------------
def test_events_errors_and_degenerates():
    torch = _torch()
    F = input_f("et")
    data, offs, _ = F.calls[3]
    n = len(data)
    d_text, d_offs = _text_dev(torch, data), _dev(torch, offs)
    s_in = _states(torch, np.arange(F_FLOWS, dtype=np.uint32) % 7)
    s_out = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    s = _stream(torch)
    rt, ac = matcher("et", "rt"), matcher("et", "ac")
    fb, ff = rt.lib.pm_hip_scan_batch_events_device, rt.lib.pm_hip_scan_flows_events_device
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
        rt.scan_flows_events_device(t, o, F_FLOWS, n, si, so, 3, e, n, c, s)
    # bad arguments: -2
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
        rt.scan_batch_events_device(t, o, F_FLOWS, n, 0, e, n, c, s)
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # before compile(): -1
    raw = pm.HipMatcher("auto")
    raw.add_pattern(b"abcd")
    assert fb(raw.obj, t, o, F_FLOWS, n, 3, e, n, c, s) == -1
    assert ff(raw.obj, t, o, F_FLOWS, n, si, so, 3, e, n, c, s) == -1
    assert raw.pattern_len(1) == 0
    h_ev, h_n = np.full(8, POISON64, np.uint64), ctypes.c_size_t(77)
    assert raw.lib.pm_hip_read_batch_events(raw.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS, 3,
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
    # pattern_len: the bytes of every gid, 0 out of range
    codes, lens = code_lengths("et")
    P = rt.lib.pm_hip_n_patterns(rt.obj)
    assert rt.pattern_len(0) == 0 and rt.pattern_len(P + 1) == 0
    for g in (1, 2, P // 2, P):
        assert rt.pattern_len(g) == int(lens[np.searchsorted(codes, rt._codes[g])])


# ---- 7. host forms and Python --------------------------------------------------------
def _read_raw(m, flows, data, offs, state, min_len, cap):
    """The C host form: (rc, events[:cap] as filled, total, state)."""
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(0)
    head = (m.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), len(offs) - 1)
    tail = (min_len, ev.ctypes.data_as(U64P), cap, ctypes.byref(total))
    if flows:
        rc = m.lib.pm_hip_read_flows_events(*head, None if state is None else state.ctypes.data_as(U32P), *tail)
    else:
        rc = m.lib.pm_hip_read_batch_events(*head, *tail)
    return rc, ev, total.value


def test_batch_events_host_forms():
    text, offs, exp = input_t("et")
    pos, codes = expected_events("et", exp, 3)
    m = matcher("et", "rt")
    try:
        before = m.scratch_bytes
        got = {}
        for cap_opt in (0, 16):  # 16: the first launch's list is too short, the second one's complete
            assert m.set_option("events_cap", cap_opt) == 0
            p, c = m.read_batch_events(text, offs)
            assert np.array_equal(p, pos) and np.array_equal(c, codes), cap_opt
            got[cap_opt] = (p, c)
        assert m.kernel_last == pm.KIND_RT
        assert m.scratch_bytes - before >= len(pos) * 8
        # read_many_events: per stream, positions inside it
        bufs = [text[a:b] for a, b in zip(offs[:-1], offs[1:])]
        many = m.read_many_events(bufs, min_len=5)
        p5, c5 = expected_events("et", exp, 5)
        assert len(many) == len(bufs)
        assert np.array_equal(np.concatenate([p + a for (p, _), a in zip(many, offs[:-1])]), p5)
        assert np.array_equal(np.concatenate([c for _, c in many]), c5)
        assert all(np.all((p >= 0) & (p < len(b))) for (p, _), b in zip(many, bufs))
        # a caller cap below the total: the first cap by position, and the true total
        cap = len(pos) // 3
        rc, ev, total = _read_raw(m, False, text, offs, None, 3, cap)
        assert rc == 0 and total == len(pos)
        _assert_list(m, ev[:cap], pos[:cap], codes[:cap], "short cap")
        assert np.array_equal(ev[:cap], np.sort(ev[:cap])) and np.all(ev[cap:] == POISON64)
        # count only
        rc, ev, total = _read_raw(m, False, text, offs, None, 3, 0)
        assert rc == 0 and total == len(pos) and np.all(ev == POISON64)
        # refused inputs: -2, nothing written
        bad = np.array([0, 10, 5, len(text)], dtype=np.int64)
        rc, ev, total = _read_raw(m, False, text, bad, None, 3, 8)
        assert rc == -2 and np.all(ev == POISON64)
        rc, ev, total = _read_raw(m, False, text, offs, None, 0, 8)
        assert rc == -2 and np.all(ev == POISON64)
    finally:
        m.set_option("events_cap", 0)


def test_flow_events_host_forms():
    F = input_f("et")
    m = matcher("et", "ac")
    try:
        runs = {}
        for cap_opt in (0, 16):
            assert m.set_option("events_cap", cap_opt) == 0
            state, out = None, []
            for r, (data, offs, exp) in enumerate(F.calls[:12]):
                pos, codes = expected_events("et", exp, 3)
                p, c, new = m.read_flows_events(data, offs, state)
                assert np.array_equal(p, pos) and np.array_equal(c, codes), (cap_opt, r)
                assert new is not state and new.dtype == np.uint32 and new.shape == (F_FLOWS,)
                state = new
                out.append(new)
            runs[cap_opt] = out
        assert all(np.array_equal(a, b) for a, b in zip(runs[0], runs[16]))
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        # the states are those of the dense host form
        state = None
        for r, (data, offs, exp) in enumerate(F.calls[:12]):
            _, state = m.read_flows_gids(data, offs, state)
            assert np.array_equal(state, runs[0][r]), r
        # a caller cap below the total, from given states: the first cap by
        # position, the true total, and the complete scan's states
        data, offs, exp = F.calls[12]
        pos, codes = expected_events("et", exp, 3)
        st = runs[0][11].copy()
        cap = len(pos) // 2
        rc, ev, total = _read_raw(m, True, data, offs, st, 3, cap)
        assert rc == 0 and total == len(pos)
        _assert_list(m, ev[:cap], pos[:cap], codes[:cap], "short cap")
        assert np.all(ev[cap:] == POISON64)
        _, want = m.read_flows_gids(data, offs, runs[0][11])
        assert np.array_equal(st, want)
        # a wild state: -2, nothing written
        wild = runs[0][11].copy()
        wild[5] = m.flow_states
        keep = wild.copy()
        rc, ev, total = _read_raw(m, True, data, offs, wild, 3, 8)
        assert rc == -2 and np.all(ev == POISON64) and np.array_equal(wild, keep)
        # FlowTable.scan_events: the same packets, the flows in another order every call
        flows = pm.FlowTable(m)
        rng = np.random.default_rng(3)
        for r, (data, offs, exp) in enumerate(F.calls[:12]):
            order = rng.permutation(F_FLOWS)
            got = flows.scan_events([(("flow", int(f)), data[offs[f]:offs[f + 1]]) for f in order], min_len=4)
            for f, (p, c) in zip(order.tolist(), got):
                wp, wc = expected_events("et", exp[offs[f]:offs[f + 1]], 4)
                assert np.array_equal(p, wp) and np.array_equal(c, wc), (r, f)
        assert len(flows) == F_FLOWS
        with pytest.raises(ValueError, match="twice"):
            flows.scan_events([("a", b"xx"), ("a", b"yy")])
    finally:
        m.set_option("events_cap", 0)
