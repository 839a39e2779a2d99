"""Pattern windows (pm_hip_set_windows, pm_hip_scan_batch_windows_device,
pm_hip_scan_flows_windows_device, pm_hip_read_*_windows): every pattern has a
(min_start, max_end) window counted in the bytes of its stream, a flow's count
carried from call to call; a list holds the patterns that pass their window
and are group-visible -- all of them, or the longest one per position.
Expected lists come from the oracle and the tests' own tables
(tests/window_inputs.py); lists are compared after sorting, positions and the
codes of the gids, exactly."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream
from flow_inputs import F_FLOWS, input_f
from group_inputs import ALL_GROUPS, TABLE, masks_by_index, stream_masks
from match_inputs import deepest_pattern, suffix_chains
from oracle_lib import dict_paths, oracle_for
from test_batch import _dev, _stream
from test_events import I64P, POISON64, U8P, U32P, U64P, Ev, _text_dev
from test_flows import STATE_POISON, _flows, _oracle_two_calls, _seam_offsets, _state_values, _states
from test_gpu_parity import SHIP, _torch, fresh_matcher, matcher
from test_groups import (_assert_complete, _assert_host_list, _assert_list, _batch_groups, _check_capacity,
                         _flow_groups)
from window_inputs import INF, expected_windows, f_pos_in, unbounded, window_of, windows_by_index

pytestmark = pytest.mark.gpu

POS_POISON = 0xDDDDDDDDDDDDDDDD
_tables = {}
_plain = {}


def reversed_window(b):
    """A second table, for the reload."""
    return window_of(b[::-1])


def seam_window(b):
    """Edges at 64 and 300 bytes: on and around the lane segment boundaries."""
    sel = len(b) % 3
    return [(0, 64), (300, INF), (0, INF)][sel]


def wmatcher(key, kind, fn=window_of):
    """The shared matcher with group_inputs' masks and the window table of fn
    set (every call sets them: some tests leave other tables behind)."""
    m = matcher(key, kind)
    if (key, fn) not in _tables:
        _tables[(key, fn)] = (masks_by_index(m._dict), windows_by_index(m._dict, fn))
    masks, win = _tables[(key, fn)]
    m.set_groups(masks)
    m.set_windows(*win)
    return m


def plain_matcher(key, kind):
    """A matcher of its own on which pm_hip_set_groups is never called."""
    if (key, kind) not in _plain:
        m = fresh_matcher(key, kind)
        m.set_windows(*windows_by_index(m._dict))
        _plain[(key, kind)] = m
    return _plain[(key, kind)]


def _pos(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint64).view(np.int64).copy()).cuda()


def _pos_values(t):
    return t.cpu().numpy().view(np.uint64)


def _ptr(t):
    return None if t is None else t.data_ptr()


def _batch_windows(m, torch, text, offs, sg, min_len, all_matches, ev):
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    d_sg = None if sg is None else _states(torch, sg)
    m.scan_batch_windows_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text), _ptr(d_sg), min_len,
                                all_matches, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    torch.cuda.synchronize()
    return ev


def _flow_windows(m, torch, text, offs, st_in, st_out, pos_in, pos_out, sg, min_len, all_matches, ev):
    d_text, d_offs = _text_dev(torch, text), _dev(torch, np.asarray(offs, dtype=np.int64))
    d_sg = None if sg is None else _states(torch, sg)
    m.scan_flows_windows_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text), _ptr(st_in),
                                _ptr(st_out), _ptr(d_sg), min_len, all_matches, ev.buf.data_ptr(), ev.cap,
                                ev.nev.data_ptr(), _stream(torch), _ptr(pos_in), _ptr(pos_out))
    torch.cuda.synchronize()
    return ev


def _ones(nseg):
    return np.full(nseg, ALL_GROUPS, np.uint32)


# ---- 1. batched form, input T --------------------------------------------------
@pytest.mark.parametrize("min_len", [1, 3, 5])
@pytest.mark.parametrize("key,kind", [("et", "rt"), ("et", "auto"), ("merged", "rt")])
def test_batch_windows_input_t(key, kind, min_len):
    torch = _torch()
    text, offs, exp = input_t(key)
    nseg = len(offs) - 1
    m = wmatcher(key, kind)
    try:
        for all_matches in (True, False):
            # stream masks, and none: every stream on all groups (a pattern in no group stays invisible)
            for sg, esg in ((stream_masks(nseg), stream_masks(nseg)), (None, _ones(nseg))):
                want = expected_windows(key, exp, offs, None, esg, min_len, all_matches)
                assert len(want[0]) > 0
                for small_max in (-1, 0):  # the one-tile-per-workgroup form, and one workgroup per CU
                    assert m.set_option("rt_small_max", small_max) == 0
                    ev = _batch_windows(m, torch, text, offs, sg, min_len, all_matches, Ev(torch, len(want[0])))
                    _assert_complete(m, ev, want, f"all {all_matches} masks {sg is not None} small_max {small_max}")
                    assert m.kernel_last == pm.KIND_RT and m.dfa_form_last == 0
    finally:
        m.set_option("rt_small_max", -1)


# ---- 2. flow form, every call of input F -----------------------------------------
@pytest.mark.parametrize("key,kind,min_len", [("et", "ac", 3), ("et", "auto", 1), ("merged", "ac", 3)])
def test_flow_windows_input_f(key, kind, min_len):
    torch = _torch()
    F = input_f(key)
    m = wmatcher(key, kind)
    sg = stream_masks(F_FLOWS)
    poison = np.full(F_FLOWS, STATE_POISON, np.uint32)
    ppoison = np.full(F_FLOWS, POS_POISON, np.uint64)
    st = {a: [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)] for a in (True, False)}
    ps = {a: [_pos(torch, np.zeros(F_FLOWS, np.uint64)), _pos(torch, ppoison)] for a in (True, False)}
    dense = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, poison)]
    seen = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        a, b = r & 1, 1 - (r & 1)
        before, after = f_pos_in(F, r), f_pos_in(F, r + 1)
        for all_matches in (True, False):
            masks = sg if all_matches else None  # the longest form without stream masks
            want = expected_windows(key, exp, offs, before, sg if all_matches else _ones(F_FLOWS), min_len,
                                    all_matches)
            ev = _flow_windows(m, torch, data, offs, st[all_matches][a], st[all_matches][b], ps[all_matches][a],
                               ps[all_matches][b], masks, min_len, all_matches, Ev(torch, len(want[0])))
            _assert_complete(m, ev, want, f"call {r} all {all_matches}")
            assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
            seen += ev.total()
            # the positions: the cumulative packet lengths, an empty stream's copied
            assert np.array_equal(_pos_values(ps[all_matches][b]), after), r
        _flows(m, torch, data, offs, dense[a], dense[b])
        # the states are the dense flow call's, whatever the windows, the masks and the form
        assert np.array_equal(_state_values(st[True][b]), _state_values(dense[b])), r
        assert np.array_equal(_state_values(st[False][b]), _state_values(dense[b])), r
    assert seen > 0
    assert np.all(f_pos_in(F, len(F.calls)) == 4096)


def test_windows_without_group_tables():
    """An object that never calls pm_hip_set_groups: every pattern is in every
    group, the group tables are not read."""
    torch = _torch()
    text, offs, exp = input_t("et")
    m = plain_matcher("et", "auto")
    try:
        for all_matches in (True, False):
            want = expected_windows("et", exp, offs, None, None, 1, all_matches)
            for small_max in (-1, 0):
                assert m.set_option("rt_small_max", small_max) == 0
                ev = _batch_windows(m, torch, text, offs, None, 1, all_matches, Ev(torch, len(want[0])))
                _assert_complete(m, ev, want, f"batch, all {all_matches}, small_max {small_max}")
    finally:
        m.set_option("rt_small_max", -1)
    F = input_f("et")
    st = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    for r, (data, offs, exp) in enumerate(F.calls[:6]):
        all_matches = bool(r & 1)
        want = expected_windows("et", exp, offs, f_pos_in(F, r), None, 3, all_matches)
        ev = _flow_windows(m, torch, data, offs, st[r & 1], st[1 - (r & 1)], _pos(torch, f_pos_in(F, r)), None, None, 3,
                           all_matches, Ev(torch, len(want[0])))
        _assert_complete(m, ev, want, f"flows, call {r}")


# ---- 3. the deepest chain with a window that admits only its third-longest member ----
def test_windows_deepest_chain_repeated():
    torch = _torch()
    pat, depth = deepest_pattern("merged")
    assert depth == 24
    chains = suffix_chains("merged")
    by_code = {(f << 24) | l: b for f, l, b in oracle_for("merged").patterns()}
    head = next(c for c in chains if by_code[c] == pat)
    members = [by_code[int(c)] for c in chains[head][0]]
    third = members[2]

    def only_third(b):
        if b == third:
            return 100, INF
        if b in members:
            return 10, 10 + len(b) - 1  # never satisfiable
        return 0, INF

    n = 1 << 16
    text = np.frombuffer((pat * (n // len(pat) + 1))[:n], dtype=np.uint8).copy()
    cuts = input_t("merged")[1]
    assert cuts[-1] == n
    rt, ac = wmatcher("merged", "rt", only_third), wmatcher("merged", "ac", only_third)
    for m in (rt, ac):  # every pattern in every group: the windows alone decide
        m.set_groups(np.full(len(m._dict.patterns()), ALL_GROUPS, np.uint32))
    third_code = next(c for c, b in by_code.items() if b == third and c in chains)
    try:
        for offs in (np.array([0, n], dtype=np.int64), np.asarray(cuts, dtype=np.int64)):
            exp = oracle_per_stream("merged", text, offs)
            for all_matches in (True, False):
                want = expected_windows("merged", exp, offs, None, None, 1, all_matches, only_third)
                what = f"{len(offs) - 1} streams, all {all_matches}"
                assert np.count_nonzero(want[1] == third_code) > 100, what
                for small_max in (-1, 0):
                    assert rt.set_option("rt_small_max", small_max) == 0
                    ev = _batch_windows(rt, torch, text, offs, None, 1, all_matches, Ev(torch, len(want[0])))
                    _assert_complete(rt, ev, want, f"batch, {what}, small_max {small_max}")
                ev = _flow_windows(ac, torch, text, offs, None, None, None, None, None, 1, all_matches,
                                   Ev(torch, len(want[0])))
                _assert_complete(ac, ev, want, f"flows, {what}")
    finally:
        rt.set_option("rt_small_max", -1)


# ---- 4. flow segment seams ------------------------------------------------------------
@pytest.mark.parametrize("n", [600 * 1024, 600 * 1024 - 5])
def test_flow_windows_segment_seams(n):
    """test_flow_groups_segment_seams' two-call text and offsets with the lane
    segment forced to 16 and 4,096 and window edges at 64 and 300 bytes: the
    300 KiB stream begins at a multiple of 16, so byte 64 of it is the last of
    a 16-byte segment; the second call continues every stream's count."""
    torch = _torch()
    offs = np.unique(np.minimum(_seam_offsets(600 * 1024), n))
    nseg = len(offs) - 1
    sg = stream_masks(nseg)
    d = pm.Dictionary(dict_paths("snort"))
    A, B = d.gen_lines(n, 9), d.gen_lines(n, 10)
    ea, eb = _oracle_two_calls("snort", A, B, offs)
    lens = np.diff(offs).astype(np.uint64)
    m = wmatcher("snort", "ac", seam_window)
    try:
        for seg in (16, 4096):
            assert m.set_option("flow_seg", seg) == 0
            s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
            s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
            p1 = _pos(torch, np.full(nseg, POS_POISON, np.uint64))
            p2 = _pos(torch, np.full(nseg, POS_POISON, np.uint64))
            want = expected_windows("snort", ea, offs, None, sg, 1, True, seam_window)
            assert len(want[0]) > 0
            ev = _flow_windows(m, torch, A, offs, None, s1, None, p1, sg, 1, True, Ev(torch, len(want[0])))
            _assert_complete(m, ev, want, f"seg {seg} call 1")
            assert np.array_equal(_pos_values(p1), lens)
            want = expected_windows("snort", eb, offs, lens, sg, 1, True, seam_window)
            assert len(want[0]) > 0
            ev = _flow_windows(m, torch, B, offs, s1, s2, p1, p2, sg, 1, True, Ev(torch, len(want[0])))
            _assert_complete(m, ev, want, f"seg {seg} call 2")
            assert np.array_equal(_pos_values(p2), 2 * lens)
    finally:
        m.set_option("flow_seg", 0)


# ---- 5. capacity and append -------------------------------------------------------------
def test_batch_windows_capacity_and_append():
    torch = _torch()
    text, offs, exp = input_t("et")
    sg = stream_masks(len(offs) - 1)
    m = wmatcher("et", "rt")
    try:
        for small_max in (-1, 0):
            assert m.set_option("rt_small_max", small_max) == 0
            for all_matches in (True, False):
                _check_capacity(torch, m, lambda ev: _batch_windows(m, torch, text, offs, sg, 3, all_matches, ev),
                                expected_windows("et", exp, offs, None, sg, 3, all_matches))
    finally:
        m.set_option("rt_small_max", -1)


def test_flow_windows_capacity_and_append():
    torch = _torch()
    F = input_f("et")
    m = wmatcher("et", "ac")
    sg = stream_masks(F_FLOWS)
    d0, o0, e0 = F.calls[16]
    before = f_pos_in(F, 16)
    # the flows as they stand before call 16: the states of a dense scan of calls 0..15
    state = None
    for data, offs, _ in F.calls[:16]:
        _, state = m.read_flows_gids(data, offs, state)
    s_in, s_out = _states(torch, state), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    p_in, p_out = _pos(torch, before), _pos(torch, np.full(F_FLOWS, POS_POISON, np.uint64))
    for all_matches in (True, False):
        _check_capacity(torch, m,
                        lambda ev: _flow_windows(m, torch, d0, o0, s_in, s_out, p_in, p_out, sg, 3, all_matches, ev),
                        expected_windows("et", e0, o0, before, sg, 3, all_matches))


# ---- 6. errors and degenerate inputs --------------------------------------------------------
def test_windows_errors_and_degenerates():
    torch = _torch()
    F = input_f("et")
    data, offs, exp = F.calls[3]
    n = len(data)
    d_text, d_offs = _text_dev(torch, data), _dev(torch, offs)
    s_in = _states(torch, np.arange(F_FLOWS, dtype=np.uint32) % 7)
    s_out = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    p_in = _pos(torch, np.arange(F_FLOWS, dtype=np.uint64) * 1000)
    p_out = _pos(torch, np.full(F_FLOWS, POS_POISON, np.uint64))
    d_sg = _states(torch, stream_masks(F_FLOWS))
    s = _stream(torch)
    rt, ac = wmatcher("et", "rt"), wmatcher("et", "ac")
    fb, ff = rt.lib.pm_hip_scan_batch_windows_device, rt.lib.pm_hip_scan_flows_windows_device
    ev = Ev(torch, n)
    t, o, e, c, g = d_text.data_ptr(), d_offs.data_ptr(), ev.buf.data_ptr(), ev.nev.data_ptr(), d_sg.data_ptr()
    si, so, pi, po = s_in.data_ptr(), s_out.data_ptr(), p_in.data_ptr(), p_out.data_ptr()

    def untouched(m, last):
        torch.cuda.synchronize()
        assert ev.total() == 0
        ev.assert_guard(0)
        assert np.all(_state_values(s_out) == STATE_POISON)
        assert np.all(_pos_values(p_out) == POS_POISON)
        assert m.kernel_last == last  # nothing launched

    for m in (rt, ac):
        m.read_block_codes(SHIP[:4096])
    last_rt, last_ac = rt.kernel_last, ac.kernel_last
    # before pm_hip_set_windows: -8, nothing launched or written; then -7 for masks without group tables
    for kind in ("rt", "ac"):
        raw = pm.HipMatcher(kind)
        raw.add_pattern(b"abcd")
        raw.add_pattern(b"bcd")
        raw.compile()
        tb = raw.table_bytes
        assert raw.pattern_window(1) is None
        raw.read_block_gids(SHIP[:4096])
        last = raw.kernel_last

        def call(groups):
            if kind == "rt":
                return fb(raw.obj, t, o, F_FLOWS, n, groups, 3, 1, e, n, c, s)
            return ff(raw.obj, t, o, F_FLOWS, n, si, so, groups, 3, 1, e, n, c, s, pi, po)

        assert call(None) == -8 and call(g) == -8
        assert b"pm_hip_set_windows" in raw.lib.pm_hip_last_error()
        untouched(raw, last)
        h_ev, h_n = np.full(8, POISON64, np.uint64), ctypes.c_size_t(77)
        hfn, extra = ((raw.lib.pm_hip_read_batch_windows, ()) if kind == "rt"
                      else (raw.lib.pm_hip_read_flows_windows, (None, None)))
        hg = stream_masks(F_FLOWS)

        def host(groups):
            return hfn(raw.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS, *extra, groups, 3, 1,
                       h_ev.ctypes.data_as(U64P), 8, ctypes.byref(h_n))

        assert host(None) == -8
        assert h_n.value == 77 and np.all(h_ev == POISON64)
        assert raw.table_bytes == tb
        # pm_hip_set_windows: n wrong, NULL arrays, min_start above 0x7FFFFFFF
        lo, hi = np.array([0, 1], np.uint32), np.array([INF, 4], np.uint32)
        big = np.array([0, 0x80000000], np.uint32)
        lop, hip_, bigp = lo.ctypes.data_as(U32P), hi.ctypes.data_as(U32P), big.ctypes.data_as(U32P)
        assert raw.lib.pm_hip_set_windows(raw.obj, lop, hip_, 1) == -2
        assert raw.lib.pm_hip_set_windows(raw.obj, lop, hip_, 3) == -2
        assert raw.lib.pm_hip_set_windows(raw.obj, None, hip_, 2) == -2
        assert raw.lib.pm_hip_set_windows(raw.obj, lop, None, 2) == -2
        assert raw.lib.pm_hip_set_windows(raw.obj, bigp, hip_, 2) == -2
        assert raw.table_bytes == tb and raw.pattern_window(1) is None
        with pytest.raises(RuntimeError, match="bad arguments"):
            raw.set_windows(lo[:1], hi[:1])
        raw.set_windows(lo, hi)
        assert raw.table_bytes == tb + 16 * 3
        assert sorted(raw.pattern_window(k) for k in (1, 2)) == [(0, INF), (1, 4)]
        assert raw.pattern_window(0) is None and raw.pattern_window(3) is None
        # stream masks without pm_hip_set_groups: -7, nothing launched or written; without masks it runs
        assert call(g) == -7
        assert b"pm_hip_set_groups" in raw.lib.pm_hip_last_error()
        untouched(raw, last)
        assert host(hg.ctypes.data_as(U32P)) == -7
        assert h_n.value == 77 and np.all(h_ev == POISON64)
        assert host(None) == 0
        raw.free()
    # before compile(): -1
    raw = pm.HipMatcher("auto")
    raw.add_pattern(b"abcd")
    one = np.array([1], np.uint32)
    assert raw.lib.pm_hip_set_windows(raw.obj, one.ctypes.data_as(U32P), one.ctypes.data_as(U32P), 1) == -1
    assert fb(raw.obj, t, o, F_FLOWS, n, g, 3, 1, e, n, c, s) == -1
    assert ff(raw.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s, pi, po) == -1
    raw.free()
    untouched(ac, last_ac)
    # the kind without the needed image: -6
    assert fb(ac.obj, t, o, F_FLOWS, n, g, 3, 1, e, n, c, s) == -6
    assert b"reverse-trie image" in ac.lib.pm_hip_last_error()
    untouched(ac, last_ac)
    assert ff(rt.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s, pi, po) == -6
    assert b"DFA image" in rt.lib.pm_hip_last_error()
    untouched(rt, last_rt)
    with pytest.raises(RuntimeError, match="DFA image"):
        rt.scan_flows_windows_device(t, o, F_FLOWS, n, si, so, g, 3, True, e, n, c, s, pi, po)
    # bad arguments: -2, as the siblings; misaligned positions, pos_in == pos_out
    for bad in [dict(min_len=0), dict(c=None), dict(e=e + 4), dict(c=c + 4), dict(e=None, cap=4), dict(t=t + 1),
                dict(o=o + 4), dict(nseg=-1), dict(n=-1), dict(n=(1 << 40) + 1), dict(g=g + 2), dict(g=g + 1)]:
        a = dict(t=t, o=o, nseg=F_FLOWS, n=n, min_len=3, e=e, cap=n, c=c, g=g)
        a.update(bad)
        for all_matches in (0, 1):
            assert fb(rt.obj, a["t"], a["o"], a["nseg"], a["n"], a["g"], a["min_len"], all_matches, a["e"], a["cap"],
                      a["c"], s) == -2, bad
            assert ff(ac.obj, a["t"], a["o"], a["nseg"], a["n"], si, so, a["g"], a["min_len"], all_matches, a["e"],
                      a["cap"], a["c"], s, pi, po) == -2, bad
    assert ff(ac.obj, t, o, F_FLOWS, n, so, so, g, 3, 1, e, n, c, s, pi, po) == -2
    assert ff(ac.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s, po, po) == -2
    assert b"pos_in != pos_out" in ac.lib.pm_hip_last_error()
    assert ff(ac.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s, pi + 4, po) == -2
    assert ff(ac.obj, t, o, F_FLOWS, n, si, so, g, 3, 1, e, n, c, s, pi, po + 4) == -2
    with pytest.raises(RuntimeError, match="bad arguments"):
        rt.scan_batch_windows_device(t, o, F_FLOWS, n, g, 0, True, e, n, c, s)
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # nseg == 0: 0, nothing launched, nothing written
    assert fb(rt.obj, t, o, 0, 0, g, 3, 1, e, n, c, s) == 0
    assert ff(ac.obj, t, o, 0, 0, si, so, g, 3, 1, e, n, c, s, pi, po) == 0
    untouched(rt, last_rt)
    untouched(ac, last_ac)
    # n == 0 with streams: the batch form launches nothing; the flow form copies states and positions
    zoffs = _dev(torch, np.zeros(F_FLOWS + 1, np.int64))
    assert fb(rt.obj, t, zoffs.data_ptr(), F_FLOWS, 0, g, 3, 1, e, n, c, s) == 0
    untouched(rt, last_rt)
    assert ff(ac.obj, t, zoffs.data_ptr(), F_FLOWS, 0, None, None, g, 3, 1, e, n, c, s, pi, po) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_pos_values(p_out), _pos_values(p_in))  # the positions alone
    assert np.all(_state_values(s_out) == STATE_POISON)
    assert ff(ac.obj, t, zoffs.data_ptr(), F_FLOWS, 0, si, so, g, 3, 1, e, n, c, s, None, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_state_values(s_out), _state_values(s_in))
    assert ev.total() == 0
    ev.assert_guard(0)
    # NULL d_pos_in: every flow at byte 0; NULL d_stream_groups: every stream on all groups
    fresh = oracle_per_stream("et", data, offs)
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    for all_matches in (True, False):
        want = expected_windows("et", fresh, offs, None, _ones(F_FLOWS), 1, all_matches)
        assert len(want[0]) > 0
        got = _batch_windows(rt, torch, data, offs, None, 1, all_matches, Ev(torch, len(want[0])))
        _assert_complete(rt, got, want, f"batch, no stream masks, all {all_matches}")
        got = _flow_windows(ac, torch, data, offs, zero, None, None, None, None, 1, all_matches,
                            Ev(torch, len(want[0])))
        _assert_complete(ac, got, want, f"flows, no stream masks, no positions, all {all_matches}")


# ---- 7. host forms and Python, the relaunch forced ---------------------------------------------
def _read_raw(m, flows, data, offs, state, pos, sg, min_len, all_matches, cap):
    """The C host form: (rc, events as filled + 8 guard slots, total)."""
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(0)
    head = (m.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), len(offs) - 1)
    tail = (None if sg is None else sg.ctypes.data_as(U32P), min_len, int(all_matches), ev.ctypes.data_as(U64P), cap,
            ctypes.byref(total))
    if flows:
        rc = m.lib.pm_hip_read_flows_windows(*head, None if state is None else state.ctypes.data_as(U32P),
                                             None if pos is None else pos.ctypes.data_as(U64P), *tail)
    else:
        rc = m.lib.pm_hip_read_batch_windows(*head, *tail)
    return rc, ev, total.value


def test_batch_windows_host_forms():
    text, offs, exp = input_t("et")
    sg = stream_masks(len(offs) - 1)
    m = wmatcher("et", "rt")
    try:
        for cap_opt in (0, 16):  # 16: the first launch's list is too short, the second one's complete
            assert m.set_option("events_cap", cap_opt) == 0
            for all_matches in (True, False):
                want = expected_windows("et", exp, offs, None, sg, 3, all_matches)
                total = len(want[0])
                _assert_host_list(m.read_batch_windows(text, offs, sg, all_matches=all_matches), want)
                assert m.kernel_last == pm.KIND_RT
                rc, ev, t = _read_raw(m, False, text, offs, None, None, sg, 3, all_matches, total)
                assert rc == 0 and t == total and np.all(ev[total:] == POISON64)
                assert np.all(ev[1:total] > ev[:total - 1])
                _assert_list(m, ev[:total], want, f"events_cap {cap_opt}")
                cap = total // 3
                rc, short, t = _read_raw(m, False, text, offs, None, None, sg, 3, all_matches, cap)
                assert rc == 0 and t == total
                assert np.array_equal(short[:cap], ev[:cap]) and np.all(short[cap:] == POISON64)
        # read_many_windows: per stream, positions inside it (events_cap is 16: every call relaunches)
        bufs = [text[a:b] for a, b in zip(offs[:-1], offs[1:])]
        many = m.read_many_windows(bufs, sg, min_len=1)
        assert len(many) == len(bufs)
        for j, ((p, c), a, b) in enumerate(zip(many, offs[:-1], offs[1:])):
            _assert_host_list((p, c), expected_windows("et", exp[a:b], [0, b - a], None, sg[j:j + 1], 1, True))
        # no stream masks: all groups
        _assert_host_list(m.read_batch_windows(text, offs, min_len=1),
                          expected_windows("et", exp, offs, None, _ones(len(offs) - 1), 1, True))
        # count only, and refused inputs: -2, nothing written
        total = len(expected_windows("et", exp, offs, None, sg, 3, True)[0])
        rc, ev, t = _read_raw(m, False, text, offs, None, None, sg, 3, True, 0)
        assert rc == 0 and t == total and np.all(ev == POISON64)
        bad = np.array([0, 10, 5, len(text)], dtype=np.int64)
        rc, ev, t = _read_raw(m, False, text, bad, None, None, sg, 3, True, 8)
        assert rc == -2 and np.all(ev == POISON64)
        rc, ev, t = _read_raw(m, False, text, offs, None, None, sg, 0, True, 8)
        assert rc == -2 and np.all(ev == POISON64)
        with pytest.raises(ValueError, match="stream_groups"):
            m.read_batch_windows(text, offs, sg[:-1])
    finally:
        m.set_option("events_cap", 0)


def test_flow_windows_host_forms():
    F = input_f("et")
    m = wmatcher("et", "ac")
    sg = stream_masks(F_FLOWS)
    calls = F.calls[:12]
    try:
        runs = {}
        for cap_opt in (0, 16):
            assert m.set_option("events_cap", cap_opt) == 0
            state, pos, out = None, None, []
            for r, (data, offs, exp) in enumerate(calls):
                all_matches = bool(r & 1)
                p, c, new, npos = m.read_flows_windows(data, offs, sg, state, pos, all_matches=all_matches)
                _assert_host_list((p, c), expected_windows("et", exp, offs, f_pos_in(F, r), sg, 3, all_matches))
                assert new is not state and new.dtype == np.uint32 and new.shape == (F_FLOWS,)
                assert npos is not pos and npos.dtype == np.uint64
                assert np.array_equal(npos, f_pos_in(F, r + 1)), r
                state, pos = new, npos
                out.append(new)
            runs[cap_opt] = out
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        # the states are those of the dense host form, relaunch or not
        state = None
        for r, (data, offs, exp) in enumerate(calls):
            _, state = m.read_flows_gids(data, offs, state)
            assert np.array_equal(state, runs[0][r]) and np.array_equal(state, runs[16][r]), r
        # (events_cap is 16 from here on: every call below relaunches)
        # the C form from given states and positions: sorted, the true total, both arrays overwritten
        data, offs, exp = F.calls[12]
        want = expected_windows("et", exp, offs, f_pos_in(F, 12), sg, 3, True)
        st, ps = runs[0][11].copy(), f_pos_in(F, 12).copy()
        cap = len(want[0]) // 2
        assert cap > 4
        rc, ev, total = _read_raw(m, True, data, offs, st, ps, sg, 3, True, cap)
        assert rc == 0 and total == len(want[0])
        assert np.all(ev[1:cap] > ev[:cap - 1]) and np.all(ev[cap:] == POISON64)
        gp, gg = pm.unpack_events(ev[:cap])
        assert np.array_equal(gp, want[0][:cap])
        _, dense = m.read_flows_gids(data, offs, runs[0][11])
        assert np.array_equal(st, dense) and np.array_equal(ps, f_pos_in(F, 13))
        # NULL pos: every flow at byte 0, nothing returned
        fresh = oracle_per_stream("et", data, offs)
        rc, ev, total = _read_raw(m, True, data, offs, None, None, sg, 3, True, len(data))
        assert rc == 0
        _assert_list(m, ev[:total], expected_windows("et", fresh, offs, None, sg, 3, True), "no state, no pos")
        # a wild state: -2, nothing written
        wild = runs[0][11].copy()
        wild[5] = m.flow_states
        keep, ps = wild.copy(), f_pos_in(F, 12).copy()
        rc, ev, total = _read_raw(m, True, data, offs, wild, ps, sg, 3, True, 8)
        assert rc == -2 and np.all(ev == POISON64) and np.array_equal(wild, keep)
        assert np.array_equal(ps, f_pos_in(F, 12))
    finally:
        m.set_option("events_cap", 0)


def test_flow_table_scan_windows_across_mixed_calls():
    """FlowTable keeps a byte count per key whichever scan method saw the
    packet: scan(), scan_groups() and scan_windows() in turn, the flows in
    another order every call."""
    F = input_f("et")
    m = wmatcher("et", "ac")
    flows = pm.FlowTable(m)
    rng = np.random.default_rng(3)
    plain = pm.FlowTable(m)
    windows_seen = 0
    for r, (data, offs, exp) in enumerate(F.calls[:10]):
        order = rng.permutation(F_FLOWS)
        pk = [(("flow", int(f)), data[offs[f]:offs[f + 1]]) for f in order]
        pk3 = [(k, b, TABLE[k[1] % 14]) for k, b in pk]
        ref = plain.scan(pk)
        if r % 3 == 0:
            got = flows.scan(pk)
            assert all(np.array_equal(a, b) for a, b in zip(got, ref))
            continue
        if r % 3 == 1:
            flows.scan_groups(pk3)
            continue
        all_matches = bool(r & 2)
        with_masks = r != 5
        got = flows.scan_windows(pk3 if with_masks else pk, min_len=2, all_matches=all_matches)
        before = f_pos_in(F, r)
        for f, (p, c) in zip(order.tolist(), got):
            a, b = int(offs[f]), int(offs[f + 1])
            want = expected_windows("et", exp[a:b], [0, b - a], before[f:f + 1],
                                    [TABLE[f % 14] if with_masks else ALL_GROUPS], 2, all_matches)
            _assert_host_list((p, c), want)
            windows_seen += len(p)
        assert flows.states == plain.states
    assert windows_seen > 0
    assert len(flows) == F_FLOWS and ("flow", 3) in flows
    assert flows.bytes[("flow", 3)] == int(f_pos_in(F, 10)[3])
    flows.end(("flow", 3))
    assert ("flow", 3) not in flows and ("flow", 3) not in flows.bytes and len(flows) == F_FLOWS - 1
    with pytest.raises(ValueError, match="twice"):
        flows.scan_windows([("a", b"xx"), ("a", b"yy")])


def test_set_windows_again_replaces_the_table_in_place():
    """A rule reload: the second table's lists hold and table_bytes grew once."""
    text, offs, exp = input_t("et")
    m = fresh_matcher("et", "auto")
    try:
        tb = m.table_bytes
        npat = len(m._dict.patterns())
        first, second = windows_by_index(m._dict), windows_by_index(m._dict, reversed_window)
        assert np.count_nonzero((first[0] != second[0]) | (first[1] != second[1])) > npat // 4
        for fn, win in ((window_of, first), (reversed_window, second), (window_of, first)):
            m.set_windows(*win)
            assert m.table_bytes == tb + 16 * (npat + 1)
            gid = int(np.nonzero(m._codes == m._dict.codes()[7])[0][0])
            assert m.pattern_window(gid) == (int(win[0][7]), int(win[1][7]))
            for all_matches in (True, False):
                want = expected_windows("et", exp, offs, None, None, 1, all_matches, fn)
                _assert_host_list(m.read_batch_windows(text, offs, None, 1, all_matches), want)
                p, c, _, _ = m.read_flows_windows(text, offs, None, None, None, 1, all_matches)
                _assert_host_list((p, c), want)
    finally:
        m.free()


# ---- 8. cross-check, device against device ------------------------------------------------------
def test_unbounded_windows_are_the_groups_calls():
    torch = _torch()
    text, offs, exp = input_t("merged")
    sg = stream_masks(len(offs) - 1)
    rt = wmatcher("merged", "rt", unbounded)
    for min_len in (1, 4):
        for all_matches in (True, False):
            sib = _batch_groups(rt, torch, text, offs, sg, min_len, all_matches, Ev(torch, 2 * len(text)))
            got = _batch_windows(rt, torch, text, offs, sg, min_len, all_matches, Ev(torch, 2 * len(text)))
            assert got.total() == sib.total() > 0
            assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))
    F = input_f("merged")
    ac = wmatcher("merged", "ac", unbounded)
    data, offs, _ = F.calls[16]
    sg = stream_masks(F_FLOWS)
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    far = _pos(torch, np.full(F_FLOWS, (1 << 40) + 7, np.uint64))  # a flow past 2^32 bytes: still unbounded
    for min_len in (1, 4):
        for all_matches in (True, False):
            sib = _flow_groups(ac, torch, data, offs, zero, None, sg, min_len, all_matches, Ev(torch, 2 * len(data)))
            got = _flow_windows(ac, torch, data, offs, zero, None, far, None, sg, min_len, all_matches,
                                Ev(torch, 2 * len(data)))
            assert got.total() == sib.total() > 0
            assert np.array_equal(np.sort(got.slots()[:got.total()]), np.sort(sib.slots()[:sib.total()]))
