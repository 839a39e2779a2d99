"""The window scans over the random dictionaries of tests/fuzz_inputs.py
(rt_batch_windows_kernel, dfa_flow_windows_kernel), and the nocase flow kernel
with flow positions past 2^32 (dfa_flow_nocase_kernel, the second copy of the
position arithmetic).

Batched over text A and as flows over A then B with window tables scaled to
the fuzz streams (window_inputs.fuzz_window_of): the families and the small
alphabets bring suffix chains up to 48 deep with a member at every depth, so
the kernels' chain folds (win[g].z / .w) meet members whose windows their
heads do not share.  Then the flow form from positions around 2^32, at 2^40
and at 2^62 (far_pos_in, far_window_of): E saturates at a stream's last byte,
in mid-stream and inside a 16-byte block, and pos_out keeps its high word.
Expected lists come from the oracle's codes, its pattern bytes and the tests'
own tables in 64-bit arithmetic; they are compared exactly, as sorted
(position, code) keys, and the cursor is the expected total.
test_fuzz_windows_cpu.py keeps the inputs from being vacuous.

The batched kernels' E counts from the stream's first byte of the call, so
their saturation needs a stream of 4 GiB: it is not reached here."""
import numpy as np
import pytest

import patternmatching_amd as pm
from fuzz_inputs import GPU_CASES, N, case
from group_inputs import ALL_GROUPS, masks_by_index, stream_masks
from nocase_inputs import brute, call_events, stream_groups
from oracle_lib import dict_paths
from test_events import Ev
from test_flows import STATE_POISON, _flows, _state_values, _states
from test_fuzz_lists import _assert_complete, _keys, _truncated
from test_fuzz_windows_cpu import nocase_far_inputs
from test_gpu_parity import _torch
from test_nocase import _flow as _nocase_flow
from test_nocase import _list, _u64, build, gids_of
from test_windows import POS_POISON, _batch_windows, _flow_windows, _pos, _pos_values
from window_inputs import expected_windows, far_pos_in, far_window_of, fuzz_window_of, windows_by_index

pytestmark = pytest.mark.gpu

PARAMS = [(name, kind) for name in GPU_CASES for kind in ("auto", "rt", "ac")]
MIN_LENS = (1, 3)

_want = {}


def want(c, which, pos_in, masked, min_len, all_matches, fn):
    """The expected (positions, codes, keys) of text `which` ("a" / "b") with
    the streams at pos_in ("zero", "lens", "far", "far+lens") under the window
    table fn; masked: stream_masks, else every stream on all groups; cached."""
    k = (c.key, which, pos_in, masked, min_len, all_matches, fn)
    if k not in _want:
        lens = np.diff(c.offs).astype(np.uint64)
        pos = {"zero": None, "lens": lens, "far": far_pos_in(c.offs), "far+lens": far_pos_in(c.offs) + lens}[pos_in]
        sg = stream_masks(c.nseg) if masked else np.full(c.nseg, ALL_GROUPS, np.uint32)
        w = expected_windows(c.key, c.ea if which == "a" else c.eb, c.offs, pos, sg, min_len, all_matches, fn=fn)
        _want[k] = w + (_keys(*w),)
    return _want[k]


def want_plain(c, min_len, all_matches):
    """Text A on an object without group tables: every pattern in every group."""
    w = expected_windows(c.key, c.ea, c.offs, None, None, min_len, all_matches, fn=fuzz_window_of)
    return w + (_keys(*w),)


def _poison(torch, c):
    return _states(torch, np.full(c.nseg, STATE_POISON, np.uint32))


def _pos_poison(torch, c):
    return _pos(torch, np.full(c.nseg, POS_POISON, np.uint64))


# ---- the batched form, text A -------------------------------------------------------------
def _batch_plain(torch, m, c):
    for all_matches in (True, False):
        w = want_plain(c, 1, all_matches)
        ev = _batch_windows(m, torch, c.A, c.offs, None, 1, all_matches, Ev(torch, len(w[0])))
        _assert_complete(m, ev, w, f"batch, no group tables, all {all_matches}")


def _batch_family(torch, m, c):
    A, offs, sg = c.A, c.offs, stream_masks(c.nseg)
    for k, small_max in enumerate((-1, 0)):  # the one-tile-per-workgroup form, and one workgroup per CU
        assert m.set_option("rt_small_max", small_max) == 0
        for all_matches in (True, False):
            for masked in (True, False):
                # every (form, masks) pair meets both min_len, one per launch form (the full cross
                # took longer than test_fuzz_lists.py's slowest parameter)
                min_len = MIN_LENS[(k + all_matches + masked) % 2]
                w = want(c, "a", "zero", masked, min_len, all_matches, fuzz_window_of)
                ev = _batch_windows(m, torch, A, offs, sg if masked else None, min_len, all_matches,
                                    Ev(torch, len(w[0])))
                _assert_complete(m, ev, w, f"batch, rt_small_max {small_max}, min_len {min_len}, "
                                 f"all {all_matches}, masks {masked}")
                assert m.kernel_last == pm.KIND_RT
    m.set_option("rt_small_max", -1)
    _truncated(m, torch, lambda ev: _batch_windows(m, torch, A, offs, sg, 1, True, ev),
               want(c, "a", "zero", True, 1, True, fuzz_window_of), "batch windows, truncated")


# ---- the flow form, A then B from zero ----------------------------------------------------
def _dense_states(torch, m, c):
    s1, s2 = _poison(torch, c), _poison(torch, c)
    _flows(m, torch, c.A, c.offs, None, s1)
    _flows(m, torch, c.B, c.offs, s1, s2)
    return _state_values(s1), _state_values(s2)


def _flow_plain(torch, m, c):
    w = want_plain(c, 1, True)
    ev = _flow_windows(m, torch, c.A, c.offs, None, None, None, None, None, 1, True, Ev(torch, len(w[0])))
    _assert_complete(m, ev, w, "flows, no group tables")


def _flow_family(torch, m, c, dense):
    A, B, offs, sg = c.A, c.B, c.offs, stream_masks(c.nseg)
    lens = np.diff(offs).astype(np.uint64)
    empty = lens == 0
    assert empty.any()
    for k, seg in enumerate((0, 16)):
        assert m.set_option("flow_seg", seg) == 0
        for all_matches in (True, False):
            # every form meets both min_len and runs with and without stream masks, one per segment length
            min_len = MIN_LENS[(k + all_matches) % 2]
            masked = all_matches == (k == 0)
            what = f"flows, seg {seg}, min_len {min_len}, all {all_matches}, masks {masked}"
            s1, s2, p1, p2 = _poison(torch, c), _poison(torch, c), _pos_poison(torch, c), _pos_poison(torch, c)
            wa = want(c, "a", "zero", masked, min_len, all_matches, fuzz_window_of)
            ev = _flow_windows(m, torch, A, offs, None, s1, None, p1, sg if masked else None, min_len,
                               all_matches, Ev(torch, len(wa[0])))
            _assert_complete(m, ev, wa, what + ", call 1")
            assert np.array_equal(_pos_values(p1), lens), what
            wb = want(c, "b", "lens", masked, min_len, all_matches, fuzz_window_of)
            ev = _flow_windows(m, torch, B, offs, s1, s2, p1, p2, sg if masked else None, min_len, all_matches,
                               Ev(torch, len(wb[0])))
            _assert_complete(m, ev, wb, what + ", call 2")
            assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
            assert np.array_equal(_pos_values(p2), 2 * lens), what
            assert np.array_equal(_pos_values(p2)[empty], np.zeros(int(empty.sum()), np.uint64)), what
            assert np.array_equal(_state_values(s1), dense[0]), what
            assert np.array_equal(_state_values(s2), dense[1]), what
    m.set_option("flow_seg", 0)


# ---- the flow form, far positions ---------------------------------------------------------
def _flow_far(torch, m, c, dense):
    """A from far_pos_in, B from A's pos_out.  The empty streams come with a
    state of their own (1) and must keep it, and their position, through both
    calls; the others begin at the root as above."""
    A, B, offs, sg = c.A, c.B, c.offs, stream_masks(c.nseg)
    lens = np.diff(offs).astype(np.uint64)
    empty = lens == 0
    far = far_pos_in(offs)
    assert m.flow_states > 1
    first = np.where(empty, 1, 0).astype(np.uint32)
    for seg in (0, 16):
        assert m.set_option("flow_seg", seg) == 0
        for all_matches in (True, False):
            masked = all_matches == (seg == 0)
            what = f"far flows, seg {seg}, all {all_matches}, masks {masked}"
            s1, s2, p1, p2 = _poison(torch, c), _poison(torch, c), _pos_poison(torch, c), _pos_poison(torch, c)
            wa = want(c, "a", "far", masked, 1, all_matches, far_window_of)
            ev = _flow_windows(m, torch, A, offs, _states(torch, first), s1, _pos(torch, far), p1,
                               sg if masked else None, 1, all_matches, Ev(torch, len(wa[0])))
            _assert_complete(m, ev, wa, what + ", call 1")
            got = _pos_values(p1)
            assert got.dtype == np.uint64 and np.array_equal(got, far + lens), what
            wb = want(c, "b", "far+lens", masked, 1, all_matches, far_window_of)
            ev = _flow_windows(m, torch, B, offs, s1, s2, p1, p2, sg if masked else None, 1, all_matches,
                               Ev(torch, len(wb[0])))
            _assert_complete(m, ev, wb, what + ", call 2")
            got = _pos_values(p2)
            assert np.array_equal(got, far + 2 * lens), what
            assert int(got.max()) >= 1 << 62 and np.array_equal(got[empty], far[empty])
            for s, d in ((s1, dense[0]), (s2, dense[1])):
                s = _state_values(s)
                assert np.all(s[empty] == 1) and np.array_equal(s[~empty], d[~empty]), what
    m.set_option("flow_seg", 0)
    # truncated, on call 2 (from the states and positions of call 1)
    s1, p1 = _poison(torch, c), _pos_poison(torch, c)
    _flow_windows(m, torch, A, offs, None, s1, _pos(torch, far), p1, sg, 1, True, Ev(torch, 0))
    _truncated(m, torch, lambda ev: _flow_windows(m, torch, B, offs, s1, None, p1, None, sg, 1, True, ev),
               want(c, "b", "far+lens", True, 1, True, far_window_of), "far flow windows, truncated")


@pytest.mark.parametrize("name,kind", PARAMS)
def test_fuzz_windows(name, kind):
    torch = _torch()
    c = case(name)
    assert len(c.A) == len(c.B) == N
    m = pm.HipMatcher(kind)
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        near, far = windows_by_index(m._dict, fuzz_window_of), windows_by_index(m._dict, far_window_of)
        m.set_windows(*near)
        # before pm_hip_set_groups: an object without group tables
        if kind != "ac":
            _batch_plain(torch, m, c)
        if kind != "rt":
            _flow_plain(torch, m, c)
        m.set_groups(masks_by_index(m._dict))
        if kind != "ac":
            _batch_family(torch, m, c)
        if kind != "rt":
            dense = _dense_states(torch, m, c)
            _flow_family(torch, m, c, dense)
            m.set_windows(*far)
            _flow_far(torch, m, c, dense)
    finally:
        for option, value in (("rt_small_max", -1), ("flow_seg", 0)):
            m.set_option(option, value)
        m.free()


# ---- the nocase flow kernel, far positions ------------------------------------------------
def test_nocase_flow_far_positions():
    """fuzz_dictionary(1) with case flags, groups and far_window_of's windows:
    A from far_pos_in, B from A's pos_out, both forms, against the brute force
    with the streams' earlier bytes counted in Python ints."""
    torch = _torch()
    pats, flags, groups, windows, A, B, offs, far = nocase_far_inputs()
    m = build(pats, "ac", flags)
    try:
        gid = gids_of(m, len(pats))
        m.set_groups(groups)
        m.set_windows(*windows)
        nseg = len(offs) - 1
        lens = np.diff(offs)
        sg = stream_groups(nseg)
        whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
        base = [int(x) for x in far]
        for all_matches in (True, False):
            rows, _ = brute(pats, flags, whole, gid, 1, groups, sg, windows, all_matches, base=base)
            open_rows, _ = brute(pats, flags, whole, gid, 1, groups, sg, None, all_matches)
            assert 0 < len(rows) < len(open_rows)
            ev, st, pos, hist = _nocase_flow(m, torch, A, offs, None, _u64(torch, far), None, sg, 1, all_matches)
            assert np.array_equal(_list(ev), call_events(rows, offs, np.zeros(nseg, np.int64))[0]), ("A", all_matches)
            assert pos.cpu().numpy().view(np.uint64).tolist() == [b + int(n) for b, n in zip(base, lens)]
            ev, _, pos2, _ = _nocase_flow(m, torch, B, offs, st, pos, hist, sg, 1, all_matches)
            assert np.array_equal(_list(ev), call_events(rows, offs, lens)[0]), ("B", all_matches)
            assert pos2.cpu().numpy().view(np.uint64).tolist() == [b + 2 * int(n) for b, n in zip(base, lens)]
    finally:
        m.free()
