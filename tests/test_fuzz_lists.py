"""The batch, flow and match-list scans over the random dictionaries of
tests/fuzz_inputs.py: dense ids, events, all matches and pattern groups, the
batched forms over text A and the flow forms over A then B continuing every
stream, against lists derived from the oracle's codes and pattern bytes alone
(event_inputs, match_inputs, group_inputs).  Lists are compared as sorted
(position, code) arrays, exactly, and the cursor is the expected total.
test_fuzz_lists_cpu.py keeps the inputs from being vacuous: a dictionary
without short patterns and one with nothing else (ev_keep's compare with
n_short), more than 4,095 patterns (the coded DFA's inline and escaped
answers in one launch), a unary chain 48 deep with an event-dense stream (the
expansion rounds, the stage flushed inside them), head densities above 0.9
(the flow kernels' direct path from the heads alone) and below 0.05, and the
bytes 0x00 and 0xFF inside patterns and at stream starts."""
import numpy as np
import pytest

import patternmatching_amd as pm
from event_inputs import expected_events
from fuzz_inputs import FAMILIES, GPU_CASES, N, case
from group_inputs import all_ones, expected_groups, masks_by_index, stream_masks
from match_inputs import expected_matches
from oracle_lib import dict_paths
from test_batch import _assert_codes, _batch
from test_events import Ev, _batch_events, _flow_events
from test_flows import STATE_POISON, _flows, _state_values, _states
from test_gpu_parity import _torch
from test_groups import _assert_host_list, _batch_groups, _flow_groups
from test_matches import _batch_matches, _flow_matches

pytestmark = pytest.mark.gpu

PARAMS = [(name, kind) for name in GPU_CASES for kind in ("auto", "rt", "ac")]
EVENT_MIN_LENS = (1, 2, 3, 4)
MATCH_MIN_LENS = (1, 3)
GROUP_MIN_LENS = (2, 3)

_want = {}


def want(c, which, form, min_len):
    """The expected (positions, codes, keys) of text `which` ("a": A from every
    stream's first byte, "b": B continuing A) in a form: "events", "matches",
    "groups_all", "groups_longest" (pattern_mask and stream_masks); cached."""
    k = (c.key, which, form, min_len)
    if k not in _want:
        exp = c.ea if which == "a" else c.eb
        if form == "events":
            _want[k] = expected_events(c.key, exp, min_len)
        elif form == "matches":
            _want[k] = expected_matches(c.key, exp, min_len)
        else:
            _want[k] = expected_groups(c.key, exp, c.offs, stream_masks(c.nseg), min_len, form == "groups_all")
        _want[k] += (_keys(*_want[k]),)
    return _want[k]


def _keys(pos, codes):
    """(position, code) pairs as u64 keys, position << 32 | code: their
    ascending order is the pairs' order by (position, code)."""
    return (np.asarray(pos).astype(np.uint64) << np.uint64(32)) | np.asarray(codes).astype(np.uint64)


def _got_keys(m, events):
    pos, gid = pm.unpack_events(events)
    return np.sort(_keys(pos, m._codes[gid]))


def _assert_complete(m, ev, w, what):
    """The cursor is the expected total, the list sorted by (position, code)
    is the expected one, exactly, and the slots past it are untouched."""
    total = len(w[2])
    assert total <= ev.cap
    assert ev.total() == total, f"{what}: cursor {ev.total()}, expected {total}"
    got = _got_keys(m, ev.slots()[:total])
    bad = np.nonzero(got != w[2])[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {total} sorted events differ, the first at position "
                           f"{int(w[0][bad[0]])}")
    ev.assert_guard(total)


def _truncated(m, torch, run, full, what):
    """One call with room for half the list: the cursor still counts every
    event, what was written belongs to the list, nothing twice, and the slots
    past cap are untouched."""
    total = len(full[0])
    if total == 0:
        return
    ev = run(Ev(torch, total // 2))
    assert ev.total() == total, f"{what}: cursor {ev.total()}, expected {total}"
    got = _got_keys(m, ev.slots()[:ev.cap])
    assert np.all(got[1:] > got[:-1]), f"{what}: an event twice"
    assert np.array_equal(full[2][np.minimum(np.searchsorted(full[2], got), total - 1)], got), \
        f"{what}: an event that is not in the list"
    ev.assert_guard(ev.cap)


def _first_positive(c, which, form, min_lens):
    return next((k for k in min_lens if len(want(c, which, form, k)[0])), min_lens[0])


# ---- the batched family, text A ----------------------------------------------------
def _batch_family(torch, m, c):
    A, offs, sg = c.A, c.offs, stream_masks(c.nseg)
    masks, ones = masks_by_index(m._dict), masks_by_index(m._dict, all_ones)
    hits = int(np.count_nonzero(c.ea))
    for small_max in (-1, 0):  # the one-tile-per-workgroup form, and one workgroup per CU
        assert m.set_option("rt_small_max", small_max) == 0
        tag = f"batch, rt_small_max {small_max}"
        for width in (4, 2):
            gids, cnt = _batch(m, torch, A, offs, width)
            _assert_codes(m, gids, c.ea, f"{tag}, u{8 * width}")
            assert cnt == hits, tag
        assert _batch(m, torch, A, offs, want_out=False) == (None, hits), tag
        assert m.kernel_last == pm.KIND_RT
        for min_len in EVENT_MIN_LENS:
            w = want(c, "a", "events", min_len)
            _assert_complete(m, _batch_events(m, torch, A, offs, min_len, ev=Ev(torch, len(w[0]))), w,
                             f"{tag}, events, min_len {min_len}")
        for min_len in MATCH_MIN_LENS:
            w = want(c, "a", "matches", min_len)
            _assert_complete(m, _batch_matches(m, torch, A, offs, min_len, Ev(torch, len(w[0]))), w,
                             f"{tag}, matches, min_len {min_len}")
        m.set_groups(masks)
        for min_len in GROUP_MIN_LENS:
            for all_matches in (True, False):
                w = want(c, "a", "groups_all" if all_matches else "groups_longest", min_len)
                ev = _batch_groups(m, torch, A, offs, sg, min_len, all_matches, Ev(torch, len(w[0])))
                _assert_complete(m, ev, w, f"{tag}, groups, all {all_matches}, min_len {min_len}")
    m.set_option("rt_small_max", -1)
    # all-ones pattern masks, no stream masks: the matches list and the events list
    m.set_groups(ones)
    for min_len in GROUP_MIN_LENS:
        for all_matches, form in ((True, "matches"), (False, "events")):
            w = want(c, "a", form, min_len)
            ev = _batch_groups(m, torch, A, offs, None, min_len, all_matches, Ev(torch, len(w[0])))
            _assert_complete(m, ev, w, f"batch, all-ones groups, all {all_matches}, min_len {min_len}")
    k = _first_positive(c, "a", "events", (3, 1))
    _truncated(m, torch, lambda ev: _batch_events(m, torch, A, offs, k, ev=ev), want(c, "a", "events", k),
               "batch events, truncated")
    _truncated(m, torch, lambda ev: _batch_matches(m, torch, A, offs, k, ev), want(c, "a", "matches", k),
               "batch matches, truncated")
    m.set_groups(masks)
    for all_matches, form in ((True, "groups_all"), (False, "groups_longest")):
        _truncated(m, torch, lambda ev: _batch_groups(m, torch, A, offs, sg, 2, all_matches, ev), want(c, "a", form, 2),
                   f"batch groups, all {all_matches}, truncated")


# ---- the flow family, A then B -------------------------------------------------------
def _poison(torch, c):
    return _states(torch, np.full(c.nseg, STATE_POISON, np.uint32))


def _flow_family(torch, m, c):
    A, B, offs, sg = c.A, c.B, c.offs, stream_masks(c.nseg)
    masks, ones = masks_by_index(m._dict), masks_by_index(m._dict, all_ones)
    # every stream's A and B as one stream: the states a single call leaves
    joined = np.concatenate([np.concatenate([A[a:b], B[a:b]]) for a, b in zip(offs[:-1], offs[1:])])
    for seg in (0, 16):
        assert m.set_option("flow_seg", seg) == 0
        s1, s2, s12 = _poison(torch, c), _poison(torch, c), _poison(torch, c)
        gids, cnt = _flows(m, torch, A, offs, None, s1)
        _assert_codes(m, gids, c.ea, f"flows, seg {seg}, call 1")
        assert cnt == int(np.count_nonzero(c.ea))
        gids, cnt = _flows(m, torch, B, offs, s1, s2)
        _assert_codes(m, gids, c.eb, f"flows, seg {seg}, call 2")
        assert cnt == int(np.count_nonzero(c.eb))
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
        _flows(m, torch, joined, 2 * offs, None, s12)
        final = _state_values(s12)
        assert np.all(final < m.flow_states)
        assert np.array_equal(_state_values(s2), final), f"flows, seg {seg}: the states after A then B"
    m.set_option("flow_seg", 0)

    def two_calls(form, min_len, run):
        """run(text, st_in, st_out, ev) over A then B; both lists and the states."""
        s1, s2 = _poison(torch, c), _poison(torch, c)
        wa, wb = want(c, "a", form, min_len), want(c, "b", form, min_len)
        _assert_complete(m, run(A, None, s1, Ev(torch, len(wa[0]))), wa, f"flows, {form}, min_len {min_len}, call 1")
        _assert_complete(m, run(B, s1, s2, Ev(torch, len(wb[0]))), wb, f"flows, {form}, min_len {min_len}, call 2")
        assert np.array_equal(_state_values(s2), final), (form, min_len)

    for min_len in EVENT_MIN_LENS:
        two_calls("events", min_len, lambda t, si, so, ev: _flow_events(m, torch, t, offs, si, so, min_len, ev=ev))
    for min_len in MATCH_MIN_LENS:
        two_calls("matches", min_len, lambda t, si, so, ev: _flow_matches(m, torch, t, offs, si, so, min_len, ev))
    m.set_groups(masks)
    for min_len in GROUP_MIN_LENS:
        for all_matches, form in ((True, "groups_all"), (False, "groups_longest")):
            two_calls(form, min_len,
                      lambda t, si, so, ev: _flow_groups(m, torch, t, offs, si, so, sg, min_len, all_matches, ev))
    m.set_groups(ones)
    s1 = _poison(torch, c)
    _flows(m, torch, A, offs, None, s1)
    for min_len in GROUP_MIN_LENS:
        for all_matches, form in ((True, "matches"), (False, "events")):
            w = want(c, "b", form, min_len)
            ev = _flow_groups(m, torch, B, offs, s1, None, None, min_len, all_matches, Ev(torch, len(w[0])))
            _assert_complete(m, ev, w, f"flows, all-ones groups, all {all_matches}, min_len {min_len}")
    # truncated, on call 2 (from call 1's states)
    k = _first_positive(c, "b", "events", (3, 1))
    _truncated(m, torch, lambda ev: _flow_events(m, torch, B, offs, s1, None, k, ev=ev), want(c, "b", "events", k),
               "flow events, truncated")
    _truncated(m, torch, lambda ev: _flow_matches(m, torch, B, offs, s1, None, k, ev), want(c, "b", "matches", k),
               "flow matches, truncated")
    m.set_groups(masks)
    for all_matches, form in ((True, "groups_all"), (False, "groups_longest")):
        _truncated(m, torch, lambda ev: _flow_groups(m, torch, B, offs, s1, None, sg, 2, all_matches, ev),
                   want(c, "b", form, 2), f"flow groups, all {all_matches}, truncated")


# ---- the host forms, the four families ---------------------------------------------------
def _host_forms(m, c, kind):
    A, B, offs, sg = c.A, c.B, c.offs, stream_masks(c.nseg)
    if kind != "ac":
        for min_len in MATCH_MIN_LENS:
            _assert_host_list(m.read_batch_matches(A, offs, min_len=min_len), want(c, "a", "matches", min_len)[:2])
    if kind != "rt":
        m.set_groups(masks_by_index(m._dict))
        for all_matches, form in ((True, "groups_all"), (False, "groups_longest")):
            p, codes, st = m.read_flows_groups(A, offs, sg, None, 2, all_matches)
            _assert_host_list((p, codes), want(c, "a", form, 2)[:2])
            p, codes, _ = m.read_flows_groups(B, offs, sg, st, 2, all_matches)
            _assert_host_list((p, codes), want(c, "b", form, 2)[:2])
        for min_len in (1, 3):
            flows = pm.FlowTable(m)
            for which, text in (("a", A), ("b", B)):
                got = flows.scan_events([(j, text[a:b]) for j, (a, b) in enumerate(zip(offs[:-1], offs[1:]))],
                                        min_len=min_len)
                assert len(got) == c.nseg
                w = want(c, which, "events", min_len)
                assert np.array_equal(np.concatenate([p + a for (p, _), a in zip(got, offs[:-1])]), w[0])
                assert np.array_equal(np.concatenate([codes for _, codes in got]), w[1])


@pytest.mark.parametrize("name,kind", PARAMS)
def test_fuzz_lists(name, kind):
    torch = _torch()
    c = case(name)
    assert len(c.A) == len(c.B) == N
    m = pm.HipMatcher(kind)
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        if kind != "ac":
            _batch_family(torch, m, c)
        if kind != "rt":
            _flow_family(torch, m, c)
        if name in FAMILIES:
            _host_forms(m, c, kind)
    finally:
        for option, value in (("rt_small_max", -1), ("flow_seg", 0)):
            m.set_option(option, value)
        m.free()
