"""The three rule calls behind every list form (pm_hip_rules_by_stream_device,
pm_hip_seq_rules_by_stream_device, pm_hip_flow_rules_device): over the random
dictionaries of tests/fuzz_inputs.py each list scan of test_fuzz_by_stream.py
is enqueued and one rule call follows on the same stream with no synchronize
and no host read between, each on a fresh list and fresh guarded outputs.

Cases unary, many, no_short, seed0 and seed5, one auto object each; per form
(events, matches, groups all and longest, windows; rt_small_max and flow_seg
alternating as test_fuzz_by_stream_cpu.launch_option says) the batched scan
over A and the flow scan over B continuing A, each followed by the rules call
and, on a second list, by the ordered-rules call; then the flow rules in two
calls: behind the flow scan of A from zeroed rows, and behind the flow scan of
B on the same device rows (a fixed random permutation), a PM_FLOW_RULES_KEEP
call first.  One nocase test (fuzz_dictionary(0), flags crc32 & 1) and one
ordered-rules call behind unary's all-matches lists with half the room.

Expected rule_ptr and hits come from text_rule_inputs.py alone: the
occurrences as byte ranges of the text (lengths from the oracle's patterns,
nocase: the brute force's starts), the rules built from what selected streams
hold (text_rule_inputs.derived_rules) and random ones; neither the library's
twins, nor its lists, nor pm_hip_pattern_len take part, except for the
truncated lists, whose content only the device knows.  The longest-only forms
take their rows from the longest-only list: rules see only what the list
holds.  test_text_rules_cpu.py keeps the inputs from being vacuous.

Running time (pytest --durations=0, one run of the whole GPU suite on an
MI355X; the yardstick is the slowest test_fuzz_lists parameter of that run,
unary-auto, 0.75 s): unary 2.20 s, many 0.83 s, seed0 0.62 s, no_short 0.49 s,
seed5 0.36 s, the nocase test 0.27 s, the truncated lists 0.16 s.  Most of it
is the Python reference (unary's all-matches lists hold a million occurrences
each); the expected values are made once per (case, text, form) in
text_rule_inputs.expected and shared with the CPU file.  No case, form or
derived kind was dropped; the random rules are 100 per call, the low end of
what was asked.
"""
import numpy as np
import pytest

import patternmatching_amd as pm
from event_inputs import code_lengths
from fuzz_inputs import N, case
from group_inputs import masks_by_index, stream_masks
from nocase_inputs import flag_of, fuzz_dictionary
from oracle_lib import dict_paths
from test_batch import _dev, _stream
from test_events import POISON64, Ev, _text_dev
from test_flow_rules import KEEP, Sets
from test_flow_rules import Out as FlowOut
from test_flow_rules import _call as flow_call
from test_flows import STATE_POISON, _states
from test_fuzz_by_stream import FLOW_SEG, SMALL_MAX, _enqueue_batch, _enqueue_flow
from test_fuzz_by_stream_cpu import CASES, FORMS, GROUP_MIN_LEN, launch_option
from test_gpu_parity import _torch
from test_nocase import _flow as _nocase_flow
from test_nocase import _u64, build, gids_of
from test_rules import Out as RulesOut
from test_rules import _assert_equal
from test_rules import _call as rules_call
from test_seq_rules import Out as SeqOut
from test_seq_rules import _call as seq_call
from test_windows import POS_POISON, _flow_windows, _pos
from text_rule_inputs import CASE_PAIR, expected, expected_flow, expected_nocase
from window_inputs import fuzz_window_of, windows_by_index

pytestmark = pytest.mark.gpu

CALLS = (("rules", rules_call, RulesOut), ("ordered rules", seq_call, SeqOut))


def _behind(torch, m, enqueue, call, out_class, total, exp, d_offs, nseg, what):
    """enqueue(ev) on a fresh list with room for exactly the expected events,
    the rule call on fresh outputs with room for exactly the expected hits,
    one synchronize; the cursor, rule_ptr, every sorted range, every guard."""
    ev = Ev(torch, total)
    o = out_class(torch, m, ev.cap, nseg, len(exp[1]))
    enqueue(ev)
    call(m, torch, ev, d_offs, nseg, o)
    torch.cuda.synchronize()
    assert ev.total() == total, f"{what}: cursor {ev.total()}, expected {total}"
    ev.assert_guard(total)
    ptr, hits = o.result()  # (the guards of the hits, rule_ptr and the scratch are checked there)
    _assert_equal(ptr, hits, exp[0], exp[1], what)
    return len(exp[1])


def _enqueue_fresh_flow(m, torch, form, d_text, d_offs, d_sg, nseg, n, st_out, ev):
    """The flow scan of a form over flows that begin here (no state, no
    position in), leaving their states."""
    t, o, e = d_text.data_ptr(), d_offs.data_ptr(), (ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    if form == "events":
        m.scan_flows_events_device(t, o, nseg, n, None, st_out.data_ptr(), 1, *e)
    elif form == "matches":
        m.scan_flows_matches_device(t, o, nseg, n, None, st_out.data_ptr(), 1, *e)
    elif form == "windows":
        m.scan_flows_windows_device(t, o, nseg, n, None, st_out.data_ptr(), d_sg.data_ptr(), 1, True, *e, None, None)
    else:
        m.scan_flows_groups_device(t, o, nseg, n, None, st_out.data_ptr(), d_sg.data_ptr(), GROUP_MIN_LEN,
                                   form == "groups_all", *e)


def _flow_pair(torch, m, f, scan_a, scan_b, totals, d_offs, nseg, what):
    """Call 1 behind scan_a from zeroed rows, committing; behind scan_b a
    PM_FLOW_RULES_KEEP call, then, on a fresh list, the committing call 2; one
    synchronize at the end.  The rows are copied on the device in between."""
    m.set_flow_rules(f["rules"])
    W = m.flow_rule_words
    rows = f["d_rows"]
    d_rows = _dev(torch, rows)
    sets = Sets(torch, np.zeros((nseg, W), dtype=np.uint64))
    evs = [Ev(torch, totals[0]), Ev(torch, totals[1]), Ev(torch, totals[1])]
    outs = [FlowOut(torch, m, ev.cap, nseg, len(f["calls"][k][1])) for ev, k in zip(evs, (0, 1, 1))]
    scan_a(evs[0])
    flow_call(m, torch, evs[0], d_offs, nseg, sets, nseg, d_rows, 0, outs[0])
    after_1 = sets.t.clone()
    scan_b(evs[1])
    flow_call(m, torch, evs[1], d_offs, nseg, sets, nseg, d_rows, KEEP, outs[1])
    after_keep = sets.t.clone()
    scan_b(evs[2])
    flow_call(m, torch, evs[2], d_offs, nseg, sets, nseg, d_rows, 0, outs[2])
    torch.cuda.synchronize()
    hits = 0
    for ev, o, k, tag in zip(evs, outs, (0, 1, 1), ("call 1", "call 2 kept", "call 2")):
        assert ev.total() == totals[k], f"{what}, {tag}: cursor {ev.total()}, expected {totals[k]}"
        ev.assert_guard(totals[k])
        ptr, got = o.result()
        _assert_equal(ptr, got, f["calls"][k][0], f["calls"][k][1], f"{what}, {tag}")
        hits += len(got)
    assert bool((after_1 == after_keep).all()), f"{what}: the PM_FLOW_RULES_KEEP call changed the rows"
    want = np.zeros((nseg, W), dtype=np.uint64)
    for j, gids in enumerate(f["held"]):
        for g in gids:
            b = m.flow_rule_bit(g)
            assert b >= 0
            want[rows[j], b >> 6] |= np.uint64(1 << (b & 63))
    assert want.any() and np.array_equal(sets.get(), want), f"{what}: the rows are not the patterns the flows' texts hold"
    return hits


@pytest.mark.parametrize("name", CASES)
def test_text_rules(name):
    torch = _torch()
    c = case(name)
    assert len(c.A) == len(c.B) == N
    offs, nseg = c.offs, c.nseg
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        codes = np.asarray(m._codes, dtype=np.uint32)
        m.set_windows(*windows_by_index(m._dict, fuzz_window_of))
        m.set_groups(masks_by_index(m._dict))
        sg = stream_masks(nseg)
        d_a, d_b, d_offs, d_sg = _text_dev(torch, c.A), _text_dev(torch, c.B), _dev(torch, offs), _states(torch, sg)
        # the states and positions a call over A leaves
        s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        p1 = _pos(torch, np.full(nseg, POS_POISON, np.uint64))
        _flow_windows(m, torch, c.A, offs, None, s1, None, p1, sg, 1, True, Ev(torch, 0))
        s_tmp = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        compared = {}
        for form in FORMS:
            k = launch_option(name, form)
            assert m.set_option("rt_small_max", SMALL_MAX[k]) == 0 and m.set_option("flow_seg", FLOW_SEG[k]) == 0
            scans = {"a": lambda ev: _enqueue_batch(m, torch, form, d_a, d_offs, d_sg, nseg, N, ev),
                     "b": lambda ev: _enqueue_flow(m, torch, form, d_b, d_offs, d_sg, nseg, N, s1, p1, ev)}
            totals = []
            for which in ("a", "b"):
                x = expected(c, which, form, codes)  # (to_gids asserts there that a code names one gid)
                d = x["derived"]
                m.set_rules(d["rules"], d["fast"])
                m.set_seq_rules(d["seq"], d["seq_fast"])
                totals.append(len(x["rows"]))
                for (tag, call, out_class), exp in zip(CALLS, (x["rules"], x["seq"])):
                    what = f"{name}, {form}, text {which}, {tag}, launch option {k}"
                    compared[(form, which, tag)] = _behind(torch, m, scans[which], call, out_class, totals[-1], exp,
                                                           d_offs, nseg, what)
                assert m.kernel_last == (pm.KIND_RT if which == "a" else pm.KIND_AC)
            compared[(form, "flow rules")] = _flow_pair(
                torch, m, expected_flow(c, form, codes),
                lambda ev: _enqueue_fresh_flow(m, torch, form, d_a, d_offs, d_sg, nseg, N, s_tmp, ev), scans["b"], totals,
                d_offs, nseg, f"{name}, {form}, flow rules, flow_seg {FLOW_SEG[k]}")
        print(f"hits compared, {name}: {compared}")
        assert min(compared.values()) > 0
    finally:
        for option, value in (("rt_small_max", -1), ("flow_seg", 0)):
            m.set_option(option, value)
        m.free()


def test_ordered_rules_behind_a_truncated_list():
    """unary, whose (stream, pattern) ranges run to hundreds of positions (the
    sort leaves the one-lane path behind a real scan): the all-matches scans
    into a list of half the room, the ordered-rules call behind them; the
    cursor ends above cap and the call equals the twin on exactly the cap slots
    the scan's waves got in, with the oracle's pattern lengths."""
    torch = _torch()
    name = "unary"
    c = case(name)
    offs, nseg = c.offs, c.nseg
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        codes = np.asarray(m._codes, dtype=np.uint32)
        cl, ll = code_lengths(name)
        plen = np.concatenate([[0], ll[np.searchsorted(cl, codes[1:])]]).astype(np.uint32)
        d_a, d_b, d_offs = _text_dev(torch, c.A), _text_dev(torch, c.B), _dev(torch, offs)
        s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        none = Ev(torch, 0)
        m.scan_flows_matches_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, N, None, s1.data_ptr(), 1, none.buf.data_ptr(),
                                    0, none.nev.data_ptr(), _stream(torch))
        k = 1 - launch_option(name, "matches")  # the launch shape the complete list did not have
        assert m.set_option("rt_small_max", SMALL_MAX[k]) == 0 and m.set_option("flow_seg", FLOW_SEG[k]) == 0
        scans = {"a": lambda ev: _enqueue_batch(m, torch, "matches", d_a, d_offs, None, nseg, N, ev),
                 "b": lambda ev: _enqueue_flow(m, torch, "matches", d_b, d_offs, None, nseg, N, s1, None, ev)}
        for which in ("a", "b"):
            x = expected(c, which, "matches", codes)
            rules = x["derived"]["seq"]
            m.set_seq_rules(rules, x["derived"]["seq_fast"])
            total = len(x["rows"])
            ev = Ev(torch, total // 2)
            o = SeqOut(torch, m, ev.cap, nseg, 2 * len(x["seq"][1]))
            scans[which](ev)
            seq_call(m, torch, ev, d_offs, nseg, o)
            torch.cuda.synchronize()
            tag = f"unary, text {which}, truncated"
            assert ev.total() == total > ev.cap, f"{tag}: cursor {ev.total()}, expected {total}"
            ev.assert_guard(ev.cap)
            exp_ptr, exp_hits = pm.seq_rules_by_stream_host(ev.slots()[:ev.cap], offs, rules, plen)
            ptr, hits = o.result()
            assert 0 < exp_ptr[-1] <= o.hits_cap and not np.array_equal(exp_ptr, x["seq"][0]), tag
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, tag)
            assert np.all(hits[ptr[-1]:] == POISON64), tag
    finally:
        for option, value in (("rt_small_max", -1), ("flow_seg", 0)):
            m.set_option(option, value)
        m.free()


def test_nocase_lists():
    """The rules call and the ordered-rules call behind the batched nocase scan
    of A and the nocase flow call over B continuing A.  "GET" and "get" are
    two gids: the derived rules pair patterns that are equal up to case and
    differ in their nocase flag."""
    torch = _torch()
    pats = fuzz_dictionary(0)
    m = build(pats, "auto", [flag_of(p) for p in pats])
    try:
        x = expected_nocase(gids_of(m, len(pats)))
        assert x["pats"] == pats and len(x["pairs"]) >= 2 and x["began_before"] > 0
        A, B, offs = x["A"], x["B"], x["offs"]
        nseg, n = len(offs) - 1, len(A)
        d_a, d_b, d_offs = _text_dev(torch, A), _text_dev(torch, B), _dev(torch, offs)
        s = _stream(torch)
        _, st, _, hist = _nocase_flow(m, torch, A, offs, None, None, None, None, 1, True)
        W = m.case_words
        st_out = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        pos_out = _u64(torch, np.full(nseg, POS_POISON, np.uint64))
        hist_out = _u64(torch, np.zeros(max(nseg * W, 1), np.uint64))

        def batch(ev):
            m.scan_batch_nocase_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, n, None, 1, True, ev.buf.data_ptr(),
                                       ev.cap, ev.nev.data_ptr(), s)

        def flow(ev):
            m.scan_flows_nocase_device(d_b.data_ptr(), d_offs.data_ptr(), nseg, n, st.data_ptr(), st_out.data_ptr(),
                                       None, 1, True, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), s, None,
                                       pos_out.data_ptr(), hist.data_ptr() if W else None, hist_out.data_ptr())
        for which, scan in (("a", batch), ("b", flow)):
            y = x[which]
            d = y["derived"]
            assert len(y["rows"]) > nseg and any(kind in CASE_PAIR for kind, _, _, _ in d["plan"] + d["seq_plan"])
            m.set_rules(d["rules"], d["fast"])
            m.set_seq_rules(d["seq"], d["seq_fast"])
            for (tag, call, out_class), e in zip(CALLS, (y["rules"], y["seq"])):
                assert _behind(torch, m, scan, call, out_class, len(y["rows"]), e, d_offs, nseg,
                               f"nocase, text {which}, {tag}")
    finally:
        m.free()
