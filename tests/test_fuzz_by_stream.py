"""Per-stream sets behind every list scan (pm_hip_events_by_stream_device;
csrc/pm_bystream.hip): over the random dictionaries of tests/fuzz_inputs.py
each list scan is enqueued and the by-stream call follows on the same stream
with no synchronize and no host read between, once per flag value, each on a
fresh list and fresh guarded outputs.

Cases unary, many, no_short, seed0 (2 symbols) and seed5 (256 symbols), one
auto object each.  Batched over text A: events and matches at min_len 1,
groups (all matches and longest) under stream_masks, windows under
fuzz_window_of; as flows over B from the states and positions of a call over
A (call 2: every stream continues, the list holds events of patterns that
began in call 1): the same five forms.  The forms alternate between
rt_small_max -1 and 0 and between flow_seg 0 and 16
(test_fuzz_by_stream_cpu.launch_option).  One batched and one flow call of
the nocase scans over nocase_inputs.fuzz_dictionary(0).  For unary and seed0
the all-matches scans into a list of half the room, then the call on what the
scan's waves got in.

Expected stream_ptr and ranges come from the oracle's lists alone
(by_stream_inputs.grouped_from_list; nocase: nocase_inputs.brute): neither
the library's twin nor its list takes part, except for the truncated lists,
whose content only the device knows (the twin of exactly those slots).
Ranges are compared exactly after sorting each, as (position, code) keys.
test_fuzz_by_stream_cpu.py keeps the inputs from being vacuous.

Running time (pytest --durations=0, one run of the whole GPU suite on an
MI355X; the yardstick is the slowest test_fuzz_lists parameter of that run,
unary-auto, 0.77 s): unary 0.66 s, many 0.47 s, seed5 0.14 s, no_short 0.13 s,
seed0 0.09 s, the nocase test 0.13 s.  No case or form was dropped.  The new
tests of test_by_stream.py in that run: the grid test's parameters 0.65 s
(distinct_keys), 0.25, 0.23, 0.15 and 0.14 s, the served read_block test
0.26 s, the captured chain 0.12 s, the others below 0.005 s.
"""
import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import first_difference, first_range_difference, grouped_from_list, list_keys
from fuzz_inputs import N, case
from group_inputs import masks_by_index, stream_masks
from nocase_inputs import brute, call_events, flag_of, fuzz_dictionary, fuzz_text, stream_offsets
from oracle_lib import dict_paths
from test_batch import _dev, _stream
from test_by_stream import Out, _call, _sorted_ranges
from test_events import POISON64, Ev, _text_dev
from test_flows import STATE_POISON, _states
from test_fuzz_by_stream_cpu import CASES, FORMS, GROUP_MIN_LEN, TRUNCATED_CASES, launch_option, want
from test_gpu_parity import _torch
from test_nocase import _flow as _nocase_flow
from test_nocase import _u64, build, gids_of
from test_windows import POS_POISON, _flow_windows, _pos
from window_inputs import fuzz_window_of, windows_by_index

pytestmark = pytest.mark.gpu

SMALL_MAX = (-1, 0)  # "rt_small_max": the one-tile-per-workgroup form, and one workgroup per CU
FLOW_SEG = (0, 16)  # "flow_seg": the default lane segment, and the shortest


# ---- the scans, enqueued only ---------------------------------------------------------
def _enqueue_batch(m, torch, form, d_text, d_offs, d_sg, nseg, n, ev):
    t, o, e = d_text.data_ptr(), d_offs.data_ptr(), (ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    if form == "events":
        m.scan_batch_events_device(t, o, nseg, n, 1, *e)
    elif form == "matches":
        m.scan_batch_matches_device(t, o, nseg, n, 1, *e)
    elif form == "windows":
        m.scan_batch_windows_device(t, o, nseg, n, d_sg.data_ptr(), 1, True, *e)
    else:
        m.scan_batch_groups_device(t, o, nseg, n, d_sg.data_ptr(), GROUP_MIN_LEN, form == "groups_all", *e)


def _enqueue_flow(m, torch, form, d_text, d_offs, d_sg, nseg, n, st_in, pos_in, ev):
    t, o, e = d_text.data_ptr(), d_offs.data_ptr(), (ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    if form == "events":
        m.scan_flows_events_device(t, o, nseg, n, st_in.data_ptr(), None, 1, *e)
    elif form == "matches":
        m.scan_flows_matches_device(t, o, nseg, n, st_in.data_ptr(), None, 1, *e)
    elif form == "windows":
        m.scan_flows_windows_device(t, o, nseg, n, st_in.data_ptr(), None, d_sg.data_ptr(), 1, True, *e,
                                    pos_in.data_ptr(), None)
    else:
        m.scan_flows_groups_device(t, o, nseg, n, st_in.data_ptr(), None, d_sg.data_ptr(), GROUP_MIN_LEN,
                                   form == "groups_all", *e)


# ---- the assertions of one call ----------------------------------------------------------
def _assert_grouped(codes, ev, o, offs, pos, wcodes, flags, what):
    """After the synchronize: the scan's cursor, stream_ptr, the sorted ranges
    as (position, code) keys, the slots past the kept events, the guards."""
    total = len(pos)
    assert ev.total() == total, f"{what}: cursor {ev.total()}, expected {total}"
    ev.assert_guard(min(total, ev.cap))
    ptr, out = o.result()  # (the three guards of the outputs and the scratch are checked there)
    exp_ptr, exp_keys = grouped_from_list(pos, wcodes, offs, bool(flags))
    assert ptr[0] == 0
    diff = first_difference(ptr, exp_ptr)
    assert not diff, f"{what}: stream_ptr: {diff}"
    p, g = pm.unpack_events(out[:ptr[-1]])
    assert g.size == 0 or int(g.max()) < len(codes), f"{what}: a gid the dictionary does not have"
    got = _sorted_ranges(ptr, list_keys(p, codes[g]))
    diff = first_range_difference(ptr, got, exp_keys)
    assert not diff, f"{what}: {diff}"
    assert np.all(out[ptr[-1]:] == POISON64), f"{what}: a slot past the kept events was written"
    if flags == 0:
        assert ptr[-1] == total, f"{what}: plain mode kept {ptr[-1]} of the cursor's {total} events"


def _chained(m, torch, codes, enqueue, w, offs, d_offs, what):
    """enqueue(ev), then the by-stream call, then one synchronize; per flag."""
    nseg = len(offs) - 1
    for flags in (0, 1):
        ev = Ev(torch, len(w[0]))
        o = Out(torch, m, ev.cap, nseg, flags, ev.cap)
        enqueue(ev)
        _call(m, torch, ev, d_offs, nseg, flags, o)
        torch.cuda.synchronize()
        _assert_grouped(codes, ev, o, offs, w[0], w[1], flags, f"{what}, flags {flags}")


def _truncated(m, torch, codes, enqueue, w, offs, d_offs, what):
    """A list with room for half the scan's events: the cursor ends above cap,
    the call groups the cap slots the scan's waves got in -- known only
    afterwards, so the expected value is the twin's on exactly those."""
    nseg = len(offs) - 1
    total = len(w[0])
    full = list_keys(*w)  # ascending
    assert total >= 128
    for flags in (0, 1):
        ev = Ev(torch, total // 2)
        o = Out(torch, m, ev.cap, nseg, flags, ev.cap)
        enqueue(ev)
        _call(m, torch, ev, d_offs, nseg, flags, o)
        torch.cuda.synchronize()
        tag = f"{what}, truncated, flags {flags}"
        assert ev.total() == total, f"{tag}: cursor {ev.total()}, expected {total}"
        ev.assert_guard(ev.cap)
        slots = ev.slots()[:ev.cap]
        ptr, out = o.result()
        exp_ptr, exp_ev = pm.events_by_stream_host(slots, offs, unique=bool(flags))
        diff = first_difference(ptr, exp_ptr)
        assert not diff, f"{tag}: stream_ptr: {diff}"
        diff = first_range_difference(ptr, _sorted_ranges(ptr, out), exp_ev)
        assert not diff, f"{tag}: {diff}"
        assert np.all(out[ptr[-1]:] == POISON64), tag
        if flags == 0:
            assert ptr[-1] == ev.cap, tag
        p, g = pm.unpack_events(out[:ptr[-1]])
        kept = list_keys(p, codes[g])
        at = np.minimum(np.searchsorted(full, kept), total - 1)
        assert np.array_equal(full[at], kept), f"{tag}: a kept event that is not in the scan's list"


@pytest.mark.parametrize("name", CASES)
def test_fuzz_by_stream(name):
    torch = _torch()
    c = case(name)
    assert len(c.A) == len(c.B) == N
    offs, nseg = c.offs, c.nseg
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        codes = np.asarray(m._codes, dtype=np.uint32)
        # a code names one gid: the (stream, code) reference is the (stream, gid) contract
        assert len(np.unique(codes[1:])) == len(codes) - 1
        m.set_windows(*windows_by_index(m._dict, fuzz_window_of))
        m.set_groups(masks_by_index(m._dict))
        sg = stream_masks(nseg)
        d_a, d_b, d_offs, d_sg = _text_dev(torch, c.A), _text_dev(torch, c.B), _dev(torch, offs), _states(torch, sg)
        # the states and positions a call over A leaves
        s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        p1 = _pos(torch, np.full(nseg, POS_POISON, np.uint64))
        _flow_windows(m, torch, c.A, offs, None, s1, None, p1, sg, 1, True, Ev(torch, 0))
        assert np.array_equal(p1.cpu().numpy().view(np.uint64), np.diff(offs).astype(np.uint64))
        for form in FORMS:
            k = launch_option(name, form)
            assert m.set_option("rt_small_max", SMALL_MAX[k]) == 0 and m.set_option("flow_seg", FLOW_SEG[k]) == 0
            _chained(m, torch, codes, lambda ev: _enqueue_batch(m, torch, form, d_a, d_offs, d_sg, nseg, N, ev),
                     want(c, "a", form), offs, d_offs, f"{name}, batch {form}, rt_small_max {SMALL_MAX[k]}")
            assert m.kernel_last == pm.KIND_RT
            _chained(m, torch, codes, lambda ev: _enqueue_flow(m, torch, form, d_b, d_offs, d_sg, nseg, N, s1, p1, ev),
                     want(c, "b", form), offs, d_offs, f"{name}, flow {form} call 2, flow_seg {FLOW_SEG[k]}")
            assert m.kernel_last == pm.KIND_AC
        if name in TRUNCATED_CASES:
            k = 1 - launch_option(name, "matches")  # the launch shape the complete list did not have
            assert m.set_option("rt_small_max", SMALL_MAX[k]) == 0 and m.set_option("flow_seg", FLOW_SEG[k]) == 0
            _truncated(m, torch, codes, lambda ev: _enqueue_batch(m, torch, "matches", d_a, d_offs, d_sg, nseg, N, ev),
                       want(c, "a", "matches"), offs, d_offs, f"{name}, batch matches")
            _truncated(m, torch, codes,
                       lambda ev: _enqueue_flow(m, torch, "matches", d_b, d_offs, d_sg, nseg, N, s1, p1, ev),
                       want(c, "b", "matches"), offs, d_offs, f"{name}, flow matches call 2")
    finally:
        for option, value in (("rt_small_max", -1), ("flow_seg", 0)):
            m.set_option(option, value)
        m.free()


def test_nocase_lists_by_stream():
    """One batched call over A and one flow call over B continuing A of the
    nocase scans (fuzz_dictionary(0), flags crc32 & 1, all matches at min_len
    1), each with the by-stream call behind it.  The expected lists are the
    brute force's: positions and gids, no codes."""
    torch = _torch()
    pats = fuzz_dictionary(0)
    flags_nc = [flag_of(p) for p in pats]
    m = build(pats, "auto", flags_nc)
    try:
        gid = gids_of(m, len(pats))
        own = np.arange(len(pats) + 1, dtype=np.uint32)  # a gid is its own code
        A, B = fuzz_text(pats, 0, 49152), fuzz_text(pats, 50, 49152)
        offs = stream_offsets(len(A), 0)
        nseg, n, lens = len(offs) - 1, len(A), np.diff(offs)
        whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
        rows, stats = brute(pats, flags_nc, whole, gid, 1)
        want_a, _ = call_events(rows, offs, np.zeros(nseg, np.int64))  # fresh flows answer as streams
        want_b, straddle = call_events(rows, offs, lens)
        assert straddle > 0 and stats["rejected"] > 0 and len(want_a) > nseg and len(want_b) > nseg
        d_a, d_b, d_offs = _text_dev(torch, A), _text_dev(torch, B), _dev(torch, offs)
        s = _stream(torch)

        def batch(ev):
            m.scan_batch_nocase_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, n, None, 1, True, ev.buf.data_ptr(),
                                       ev.cap, ev.nev.data_ptr(), s)
        _chained(m, torch, own, batch, pm.unpack_events(want_a), offs, d_offs, "nocase, batch")
        _, st, _, hist = _nocase_flow(m, torch, A, offs, None, None, None, None, 1, True)
        W = m.case_words
        st_out = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        pos_out = _u64(torch, np.full(nseg, POS_POISON, np.uint64))
        hist_out = _u64(torch, np.zeros(max(nseg * W, 1), np.uint64))

        def flow(ev):
            m.scan_flows_nocase_device(d_b.data_ptr(), d_offs.data_ptr(), nseg, n, st.data_ptr(), st_out.data_ptr(),
                                       None, 1, True, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), s, None,
                                       pos_out.data_ptr(), hist.data_ptr() if W else None, hist_out.data_ptr())
        _chained(m, torch, own, flow, pm.unpack_events(want_b), offs, d_offs, "nocase, flow call 2")
    finally:
        m.free()
