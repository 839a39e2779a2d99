"""The ten device list calls, pm_hip_scan_{batch,flows}_{events,matches,groups,
windows,nocase}_device, share one argument check: every one of them rejects the
same bad pointers and counts with -2 before anything is written or launched,
and a valid call on the same tiny input returns the list of the matching host
form (pm_hip_read_*), compared exactly as sorted u64."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from nocase_inputs import HAND, HAND_TEXTS
from test_batch import _dev, _stream
from test_events import I64P, U8P, U32P, U64P, Ev, _text_dev
from test_flows import STATE_POISON, _state_values, _states
from test_gpu_parity import _torch
from test_nocase import _u64

pytestmark = pytest.mark.gpu

FORMS = ("events", "matches", "groups", "windows", "nocase")
TEXT = np.frombuffer((b" ".join(HAND_TEXTS) * 2)[:64], np.uint8)  # 64 bytes
OFFS = np.array([0, 29, 64], np.int64)                            # in 2 streams
NSEG = 2
MASKS = np.array([1, 3], np.uint32)
CURSOR = 12345  # the cursor a rejected call must leave as it found it
OUT64 = 0xDDDDDDDDDDDDDDDD

_cache = {}


def matcher():
    """An auto object (both images) with group, window and nocase tables, so
    that every form gets past its own check and every pointer has a reader."""
    if "m" not in _cache:
        m = pm.HipMatcher("auto")
        for p, _ in HAND:
            m.add_pattern(p)
        m.compile()
        m.set_groups(np.array([1 + (k & 1) for k in range(len(HAND))], np.uint32))
        m.set_windows(np.zeros(len(HAND), np.uint32), np.full(len(HAND), 0xFFFFFFFF, np.uint32))
        m.set_nocase(np.array([f for _, f in HAND], np.uint8))
        assert m.case_words == 1
        _cache["m"] = m
    return _cache["m"]


def _args(form, flows, a):
    """The argument list of one entry point from the superset a."""
    out = [a["t"], a["o"], a["nseg"], a["n"]]
    if flows:
        out += [a["si"], a["so"]]
    out += [a["min_len"]] if form in ("events", "matches") else [a["g"], a["min_len"], 1]
    out += [a["e"], a["cap"], a["c"], a["s"]]
    if flows and form in ("windows", "nocase"):
        out += [a["pi"], a["po"]]
    if flows and form == "nocase":
        out += [a["ci"], a["co"]]
    return out


def _host_list(m, form, flows):
    """The matching host form on the same input, fresh flows: sorted u64 events."""
    fn = getattr(m.lib, f"pm_hip_read_{'flows' if flows else 'batch'}_{form}")
    ev, total = np.zeros(4096, np.uint64), ctypes.c_size_t(0)
    st, ps, cs = np.zeros(NSEG, np.uint32), np.zeros(NSEG, np.uint64), np.zeros(NSEG * m.case_words, np.uint64)
    args = [m.obj, TEXT.ctypes.data_as(U8P), OFFS.ctypes.data_as(I64P), NSEG]
    if flows:
        args.append(st.ctypes.data_as(U32P))
        if form in ("windows", "nocase"):
            args.append(ps.ctypes.data_as(U64P))
        if form == "nocase":
            args.append(cs.ctypes.data_as(U64P))
    args += [1] if form in ("events", "matches") else [MASKS.ctypes.data_as(U32P), 1, 1]
    assert fn(*args, ev.ctypes.data_as(U64P), len(ev), ctypes.byref(total)) == 0
    assert 0 < total.value <= len(ev)
    return ev[:total.value]  # the host forms sort


@pytest.mark.parametrize("layout", ("batch", "flows"))
@pytest.mark.parametrize("form", FORMS)
def test_list_entry_point_rejects_alike_then_runs(form, layout):
    torch = _torch()
    m = matcher()
    flows = layout == "flows"
    W = m.case_words
    fn = getattr(m.lib, f"pm_hip_scan_{layout}_{form}_device")
    d_text, d_offs, d_sg = _text_dev(torch, TEXT), _dev(torch, OFFS), _states(torch, MASKS)
    s_in = _states(torch, np.zeros(NSEG, np.uint32))
    s_out = _states(torch, np.full(NSEG, STATE_POISON, np.uint32))
    p_in, p_out = _u64(torch, np.zeros(NSEG, np.uint64)), _u64(torch, np.full(NSEG, OUT64, np.uint64))
    c_in, c_out = _u64(torch, np.zeros(NSEG * W, np.uint64)), _u64(torch, np.full(NSEG * W, OUT64, np.uint64))
    bad_ev = Ev(torch, 64, cursor=CURSOR)
    good = dict(t=d_text.data_ptr(), o=d_offs.data_ptr(), nseg=NSEG, n=len(TEXT), si=s_in.data_ptr(),
                so=s_out.data_ptr(), g=d_sg.data_ptr(), min_len=1, e=bad_ev.buf.data_ptr(), cap=bad_ev.cap,
                c=bad_ev.nev.data_ptr(), s=_stream(torch), pi=p_in.data_ptr(), po=p_out.data_ptr(),
                ci=c_in.data_ptr(), co=c_out.data_ptr())
    # the last launch was the other layout's kernel, so one from a rejected call would show
    if flows:
        m.read_batch_gids(TEXT, OFFS)
    else:
        m.read_flows_gids(TEXT, OFFS)
    last = m.kernel_last
    assert last == (pm.KIND_RT if flows else pm.KIND_AC)

    bad = [dict(t=good["t"] + 1), dict(o=good["o"] + 4), dict(e=good["e"] + 4), dict(nseg=-1), dict(n=-1),
           dict(min_len=0), dict(c=None), dict(e=None, cap=4)]
    if flows:
        bad += [dict(si=good["si"] + 2), dict(so=good["so"] + 2), dict(si=good["so"])]
        if form in ("windows", "nocase"):
            bad += [dict(pi=good["pi"] + 4), dict(po=good["po"] + 4), dict(pi=good["po"])]
        if form == "nocase":
            bad += [dict(ci=good["ci"] + 4), dict(co=good["co"] + 4), dict(ci=good["co"])]
    for b in bad:
        assert fn(m.obj, *_args(form, flows, {**good, **b})) == -2, b
        assert b"bad arguments" in m.lib.pm_hip_last_error(), b
        assert m.kernel_last == last, b
    torch.cuda.synchronize()
    assert bad_ev.total() == CURSOR
    bad_ev.assert_guard(0)
    assert np.all(_state_values(s_out) == STATE_POISON)
    for out in (p_out, c_out):
        assert np.all(out.cpu().numpy().view(np.uint64) == OUT64)

    ev = Ev(torch, 4096)
    ok = {**good, "e": ev.buf.data_ptr(), "cap": ev.cap, "c": ev.nev.data_ptr()}
    assert fn(m.obj, *_args(form, flows, ok)) == 0
    torch.cuda.synchronize()
    assert m.kernel_last == (pm.KIND_AC if flows else pm.KIND_RT)
    total = ev.total()
    assert np.array_equal(np.sort(ev.slots()[:total]), _host_list(m, form, flows))
    ev.assert_guard(total)
