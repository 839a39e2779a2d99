"""The flow scan (pm_hip_scan_flows_device*, pm_hip_read_flows*): the batched
layout with a carried DFA state per stream, so a flow's packets arriving in
separate calls give the answers of the flow scanned in one piece.  Expected
values come from the oracle over each whole flow (tests/flow_inputs.py) and,
for the states, from the host step pm_flat_host_scan_flows.  Bit-exact."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from flow_inputs import F_FLOWS, input_f, precondition
from oracle_lib import dict_paths, oracle_for
from test_batch import POISON, _assert_codes, _batch, _dev, _ids, _poisoned, _stream
from test_flows_cpu import host_flows
from test_gpu_parity import SHIP, _torch, matcher
from test_tables_cpu import image

pytestmark = pytest.mark.gpu

U8P = ctypes.POINTER(ctypes.c_uint8)
U32P = ctypes.POINTER(ctypes.c_uint32)
I64P = ctypes.POINTER(ctypes.c_int64)
STATE_POISON = 0xEEEEEEEE


def _states(torch, values):
    return torch.from_numpy(np.asarray(values, dtype=np.uint32).view(np.int32).copy()).cuda()


def _state_values(t):
    return t.cpu().numpy().view(np.uint32)


def _flows(m, torch, text, offs, st_in, st_out, width=4, want_out=True):
    """One device flow call: (gids or None, count).  st_in / st_out: device
    int32 tensors of nseg values, or None."""
    n = len(text)
    d_text = _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, np.asarray(offs, dtype=np.int64))
    out = _poisoned(torch, n, width) if want_out else None
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.scan_flows_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, n,
                        None if st_in is None else st_in.data_ptr(), None if st_out is None else st_out.data_ptr(),
                        out.data_ptr() if want_out else None, cnt.data_ptr(), _stream(torch), out_width=width)
    torch.cuda.synchronize()
    return (_ids(out, n, width) if want_out else None), int(cnt.item())


@pytest.mark.parametrize("out_width", [4, 2])
@pytest.mark.parametrize("kind", ["ac", "auto"])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_flows_equal_oracle_per_flow(key, kind, out_width):
    torch = _torch()
    differ, deep = precondition(key)
    assert differ >= 5000 and deep >= 2000
    F = input_f(key)
    m = matcher(key, kind)
    ping = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    for r, (data, offs, exp) in enumerate(F.calls):
        gids, cnt = _flows(m, torch, data, offs, ping[r & 1], ping[1 - (r & 1)], out_width)
        _assert_codes(m, gids, exp, f"call {r}")
        assert cnt == int(np.count_nonzero(exp)), r
        assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
    assert np.all(_state_values(ping[len(F.calls) & 1]) < m.flow_states)


def test_flows_states_equal_host_step():
    torch = _torch()
    F = input_f("et")
    d, img, tab = image("et", pm.KIND_AC)
    m = matcher("et", "ac")
    assert m.flow_states == img.lib.pm_flat_flow_states(img.h)
    ping = [_states(torch, np.zeros(F_FLOWS, np.uint32)), _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))]
    h_state = np.zeros(F_FLOWS, np.uint32)
    for r, (data, offs, exp) in enumerate(F.calls):
        rc, h_gids, h_state = host_flows(img, data, offs, h_state)
        assert rc == 0
        gids, _ = _flows(m, torch, data, offs, ping[r & 1], ping[1 - (r & 1)])
        assert np.array_equal(gids, h_gids), r
        assert np.array_equal(_state_values(ping[1 - (r & 1)]), h_state), r


def _seam_offsets(n):
    k = np.arange(1, 65, dtype=np.int64) * 1024
    k32 = np.arange(3000, 3064, dtype=np.int64) * 32
    big = 200000
    offs = np.unique(np.concatenate([[0], k - 1, k, k + 1, k32 - 1, k32, k32 + 1, 100000 + np.arange(2049),
                                     [big, big + 300 * 1024], [n]]))
    assert offs[0] == 0 and offs[-1] == n and np.count_nonzero(np.diff(offs) == 1) >= 2048
    assert offs[np.searchsorted(offs, big) + 1] == big + 300 * 1024
    return offs


def _oracle_two_calls(key, A, B, offs):
    """The codes of A_j + B_j per stream j, split back into A's and B's."""
    o = oracle_for(key)
    ea, eb = np.zeros(len(A), np.uint32), np.zeros(len(B), np.uint32)
    for a, b in zip(offs[:-1].tolist(), offs[1:].tolist()):
        if b > a:
            o.reset()
            both = o.scan_codes(np.concatenate([A[a:b], B[a:b]]))
            ea[a:b], eb[a:b] = both[:b - a], both[b - a:]
    o.reset()
    return ea, eb


def test_flows_segment_seams():
    """Streams ending at, just before and just after 64 multiples of 1,024 and
    64 multiples of 32 (lane segment and 16-byte block edges), 2,048 one-byte
    streams, one 300 KiB stream (most of its lanes warm up from the root), with
    the lane segment forced to 16, 32, 48, 512, 4,096 and the launcher's own;
    two chained calls, on a shallow text and on dense deep matches."""
    torch = _torch()
    n = 600 * 1024
    offs = _seam_offsets(n)
    nseg = len(offs) - 1
    assert (oracle_for("snort").max_len - 1) * 8 < 300 * 1024
    d = pm.Dictionary(dict_paths("snort"))
    texts = [(pm.gen_stream(n, seed=9, mode=0), pm.gen_stream(n, seed=10, mode=0)),
             (d.gen_lines(n, 9), d.gen_lines(n, 10))]
    expect = [_oracle_two_calls("snort", A, B, offs) for A, B in texts]
    m = matcher("snort", "ac")
    try:
        for seg in (16, 32, 48, 512, 4096, 0):
            assert m.set_option("flow_seg", seg) == 0
            for (A, B), (ea, eb) in zip(texts, expect):
                s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
                gids, cnt = _flows(m, torch, A, offs, None, s1)
                _assert_codes(m, gids, ea, f"seg {seg} call 1")
                assert cnt == int(np.count_nonzero(ea)), seg
                assert np.all(_state_values(s1) < m.flow_states), seg
                gids, cnt = _flows(m, torch, B, offs, s1, s2)
                _assert_codes(m, gids, eb, f"seg {seg} call 2")
                assert cnt == int(np.count_nonzero(eb)), seg
    finally:
        m.set_option("flow_seg", 0)
    for bad in (8, 17, 4112, -16):
        assert m.set_option("flow_seg", bad) == -1


def test_flows_fresh_equals_batch():
    torch = _torch()
    text, offs, exp = input_t("merged")
    m = matcher("merged", "auto")
    ref, ref_cnt = _batch(m, torch, text, offs)
    assert m.kernel_last == pm.KIND_RT
    gids, cnt = _flows(m, torch, text, offs, None, None)
    assert m.kernel_last == pm.KIND_AC
    assert np.array_equal(gids, ref) and cnt == ref_cnt
    _assert_codes(m, gids, exp, "fresh")


def test_flows_count_only_and_null_state_out():
    torch = _torch()
    F = input_f("et")
    m = matcher("et", "ac")
    (d0, o0, e0), (d1, o1, e1) = F.calls[7], F.calls[8]
    zero = _states(torch, np.zeros(F_FLOWS, np.uint32))
    # the states after call 7 from fresh flows, ids wanted and not
    s_a = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    s_b = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    gids, cnt = _flows(m, torch, d0, o0, zero, s_a)
    none, cnt0 = _flows(m, torch, d0, o0, None, s_b, want_out=False)
    assert none is None and cnt0 == cnt == int(np.count_nonzero(gids))
    assert np.array_equal(_state_values(s_a), _state_values(s_b))
    # call 8 from those states: no state out, then neither ids nor state out
    o = oracle_for("et")
    exp = np.zeros(len(d1), np.uint32)
    for j in range(F_FLOWS):
        o.reset()
        both = o.scan_codes(np.concatenate([d0[o0[j]:o0[j + 1]], d1[o1[j]:o1[j + 1]]]))
        exp[o1[j]:o1[j + 1]] = both[o0[j + 1] - o0[j]:]
    o.reset()
    gids, cnt = _flows(m, torch, d1, o1, s_a, None)
    _assert_codes(m, gids, exp, "no state out")
    assert cnt == int(np.count_nonzero(exp))
    none, cnt = _flows(m, torch, d1, o1, s_a, None, want_out=False)
    assert cnt == int(np.count_nonzero(exp))
    # every stream empty: the states are handed on, nothing else is written
    s_c = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    gids, cnt = _flows(m, torch, np.zeros(0, np.uint8), np.zeros(F_FLOWS + 1, np.int64), s_a, s_c)
    assert cnt == 0 and np.array_equal(_state_values(s_c), _state_values(s_a))
    # no stream at all: nothing launched, the states untouched
    s_d = _states(torch, np.full(4, STATE_POISON, np.uint32))
    _flows(m, torch, np.zeros(0, np.uint8), np.zeros(1, np.int64), s_a, s_d)
    assert np.all(_state_values(s_d) == STATE_POISON)


def test_flows_host_forms():
    F = input_f("merged")
    m = matcher("merged", "ac")
    state = None
    gid_calls = []
    for r, (data, offs, exp) in enumerate(F.calls):
        if r % 2:
            codes, new = m.read_flows_codes(data, offs, state)
        else:
            gids, new = m.read_flows_gids(data, offs, state)
            codes = m._codes[gids]
            gid_calls.append((r, gids, state))
        assert np.array_equal(codes, exp), r
        assert new is not state and new.dtype == np.uint32 and new.shape == (F_FLOWS,)
        state = new
    assert m.kernel_last == pm.KIND_AC and m.dfa_form_last == 1
    assert m.scratch_bytes >= max(len(c[0]) for c in F.calls) * 5 + (F_FLOWS + 1) * 8 + 2 * F_FLOWS * 4
    # read_flows: the add_pattern ids of the gids
    size = ctypes.sizeof(pm._lib.PmPattern)
    P = m.lib.pm_hip_n_patterns(m.obj)
    pid = m.gid_codes(np.uint64(m._dict.pattern_ptr(0)) + np.arange(P, dtype=np.uint64) * np.uint64(size))
    r, gids, st = gid_calls[3]
    ids, _ = m.read_flows_id_array(F.calls[r][0], F.calls[r][1], st)
    assert np.array_equal(ids.astype(np.uint64), pid[gids])
    # FlowTable: the same packets, the flows in a different order every call
    flows = pm.FlowTable(m)
    rng = np.random.default_rng(3)
    for r, (data, offs, exp) in enumerate(F.calls):
        order = rng.permutation(F_FLOWS)
        got = flows.scan([(("flow", int(f)), data[offs[f]:offs[f + 1]]) for f in order])
        for f, codes in zip(order.tolist(), got):
            assert np.array_equal(codes, exp[offs[f]:offs[f + 1]]), (r, f)
    assert len(flows) == F_FLOWS
    # inputs the host form refuses: -2, nothing written
    data, offs, _ = F.calls[9]
    n = len(data)
    fn = m.lib.pm_hip_read_flows_gid
    good_state = np.zeros(F_FLOWS, np.uint32)

    def call(o, st):
        out = np.full(n, POISON, dtype=np.uint32)
        o = np.array(o, dtype=np.int64)
        before = st.copy()
        rc = fn(m.obj, data.ctypes.data_as(U8P), o.ctypes.data_as(I64P), len(o) - 1, st.ctypes.data_as(U32P),
                out.ctypes.data_as(U32P))
        assert np.all(out == POISON) and np.array_equal(st, before)
        return rc

    assert call([1, n], good_state[:1].copy()) == -2
    assert call([0, 10, 5, n], good_state[:3].copy()) == -2
    wild = good_state.copy()
    wild[200] = m.flow_states
    assert call(offs, wild) == -2
    with pytest.raises(RuntimeError):
        m.read_flows_gids(data, offs, wild)
    wild[200] = m.flow_states - 1  # the largest valid state is accepted
    m.read_flows_gids(data, offs, wild)


@pytest.mark.parametrize("kind", ["ac", "auto"])
def test_flows_leave_carried_state_alone(kind):
    F = input_f("et")
    data, offs, _ = F.calls[3]
    m = matcher("et", kind)
    fresh, st = m.read_flows_codes(data, offs)
    whole = m.read_block_codes(SHIP)
    h = len(SHIP) // 2
    m.reset()
    first = m.read_block_codes(SHIP[:h])
    again, st2 = m.read_flows_codes(data, offs)
    assert np.array_equal(again, fresh) and np.array_equal(st2, st)
    second = m.read_block_codes(SHIP[h:])
    assert np.array_equal(np.concatenate([first, second]), whole)
    # read_char after a flow call continues the stream
    m.reset()
    head = m.read_block_codes(SHIP[:700])
    again, _ = m.read_flows_codes(data, offs)
    assert np.array_equal(again, fresh)
    tail = [m.lib.pm_pattern_code(m.read_char(int(c))) for c in SHIP[700:1000].tolist()]
    assert np.array_equal(head, whole[:700]) and tail == whole[700:1000].tolist()


def test_flows_unsupported_on_rt():
    torch = _torch()
    F = input_f("et")
    data, offs, _ = F.calls[3]
    n = len(data)
    m = matcher("et", "rt")
    assert m.flow_states == 0
    d_text = _dev(torch, np.concatenate([data, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, offs)
    out = _poisoned(torch, n, 4)
    s_in = _states(torch, np.zeros(F_FLOWS, np.uint32))
    s_out = _states(torch, np.full(F_FLOWS, STATE_POISON, np.uint32))
    args = (m.obj, d_text.data_ptr(), d_offs.data_ptr(), F_FLOWS, n, s_in.data_ptr(), s_out.data_ptr(), out.data_ptr(),
            None, _stream(torch))
    m.read_block_codes(SHIP[:4096])
    last = m.kernel_last
    assert m.lib.pm_hip_scan_flows_device(*args) == -6
    msg = m.lib.pm_hip_last_error()
    assert b"DFA image" in msg and b"ac" in msg and b"auto" in msg
    out16 = _poisoned(torch, n, 2)
    assert m.lib.pm_hip_scan_flows_device16(*(args[:7] + (out16.data_ptr(),) + args[8:])) == -6
    h_out = np.full(n, POISON, dtype=np.uint32)
    h_state = np.zeros(F_FLOWS, np.uint32)
    rc = m.lib.pm_hip_read_flows_gid(m.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS,
                                     h_state.ctypes.data_as(U32P), h_out.ctypes.data_as(U32P))
    assert rc == -6 and np.all(h_out == POISON) and not h_state.any()
    ids = np.zeros(n, dtype=np.uintp)
    rc = m.lib.pm_hip_read_flows(m.obj, data.ctypes.data_as(ctypes.c_char_p), offs.ctypes.data_as(I64P), F_FLOWS,
                                 None, ids.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)))
    assert rc == -6 and not ids.any()
    with pytest.raises(RuntimeError, match="DFA image"):
        m.scan_flows_device(*args[1:])
    torch.cuda.synchronize()
    assert np.all(_ids(out, n, 4) == POISON) and np.all(_ids(out16, n, 2) == (POISON & 0xFFFF))
    assert np.all(_state_values(s_out) == STATE_POISON)
    assert m.kernel_last == last  # nothing launched
    # before compile(): -1
    raw = pm.HipMatcher("ac")
    raw.add_pattern(b"abc")
    assert raw.lib.pm_hip_scan_flows_device(*((raw.obj,) + args[1:])) == -1
    assert raw.lib.pm_hip_read_flows_gid(raw.obj, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), F_FLOWS,
                                         h_state.ctypes.data_as(U32P), h_out.ctypes.data_as(U32P)) == -1
    assert raw.flow_states == 0
    raw.free()


def test_flows_bad_arguments():
    torch = _torch()
    F = input_f("et")
    data, offs, _ = F.calls[3]
    n = len(data)
    m = matcher("et", "ac")
    d_text = _dev(torch, np.concatenate([data, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, np.concatenate([offs, np.zeros(1, np.int64)]))
    out = _poisoned(torch, n + 16, 4)
    s_in = _states(torch, np.zeros(F_FLOWS + 4, np.uint32))
    s_out = _states(torch, np.full(F_FLOWS + 4, STATE_POISON, np.uint32))
    fn, s = m.lib.pm_hip_scan_flows_device, _stream(torch)
    t, o, d, si, so = d_text.data_ptr(), d_offs.data_ptr(), out.data_ptr(), s_in.data_ptr(), s_out.data_ptr()
    assert fn(m.obj, t + 1, o, F_FLOWS, n - 1, si, so, d, None, s) == -2
    assert fn(m.obj, t, o, F_FLOWS, n, si, so, d + 4, None, s) == -2
    assert fn(m.obj, t, o + 4, F_FLOWS, n, si, so, d, None, s) == -2
    assert fn(m.obj, t, o, F_FLOWS, n, si + 2, so, d, None, s) == -2
    assert fn(m.obj, t, o, F_FLOWS, n, si, so + 1, d, None, s) == -2
    assert fn(m.obj, t, o, -1, n, si, so, d, None, s) == -2
    assert fn(m.obj, t, o, F_FLOWS, -1, si, so, d, None, s) == -2
    assert fn(m.obj, t, o, F_FLOWS, n, so, so, d, None, s) == -2
    assert m.lib.pm_hip_scan_flows_device16(m.obj, t, o, F_FLOWS, n, si, so, d + 2, None, s) == -2
    with pytest.raises(RuntimeError, match="bad arguments"):
        m.scan_flows_device(t, o, F_FLOWS, n, so, so, d, None, s)
    torch.cuda.synchronize()
    assert np.all(_ids(out, n + 16, 4) == POISON)
    assert np.all(_state_values(s_out) == STATE_POISON)


@pytest.mark.slow
def test_flows_uncoded_automaton():
    """More than 2^20 states: plain transition words (dfa_flow_kernel<.,
    false>).  64 KiB of the dictionary's patterns back to back, as 200 streams
    that begin where a pattern begins; every stream is cut at a random point,
    call 1 scans the first parts, call 2 the second parts from call 1's
    states.  Checked against one read_block_codes of the uncut text by the same
    object (no occurrence straddles a stream's start: the patterns are random
    strings of 20 to 39 bytes)."""
    torch = _torch()
    rng = np.random.default_rng(21)
    pats = [bytes(rng.integers(0x20, 0x7F, size=int(L), dtype=np.uint8)) for L in rng.integers(20, 40, size=40000)]
    ac = pm.HipMatcher("ac")
    ac.add_dictionary(pm.Dictionary(patterns=pats))
    ac.compile()
    assert ac.flow_states > 1 << 20
    n = 1 << 16
    chosen = [pats[int(k)] for k in rng.integers(0, len(pats), size=n // 20)]
    text = np.frombuffer(b"".join(chosen), np.uint8)[:n].copy()
    starts = np.cumsum([0] + [len(p) for p in chosen])
    starts = starts[starts < n]
    whole = ac.read_block_codes(text)
    ac.reset()
    assert np.count_nonzero(whole) >= len(starts) - 1
    edges = np.unique(np.concatenate([[0, n], rng.choice(starts[1:], size=199, replace=False)]))
    nseg = len(edges) - 1
    cut = np.array([rng.integers(a, b + 1) for a, b in zip(edges[:-1], edges[1:])], dtype=np.int64)
    assert np.count_nonzero((cut > edges[:-1]) & (cut < edges[1:])) > nseg // 2
    parts1 = [text[a:c] for a, c in zip(edges[:-1], cut)]
    parts2 = [text[c:b] for c, b in zip(cut, edges[1:])]
    exp1 = np.concatenate([whole[a:c] for a, c in zip(edges[:-1], cut)])
    exp2 = np.concatenate([whole[c:b] for c, b in zip(cut, edges[1:])])
    s1 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
    s2 = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
    for width in (4, 2):
        gids, cnt = _flows(ac, torch, np.concatenate(parts1), pm.batch_offsets(parts1), None, s1, width)
        _assert_codes(ac, gids, exp1, f"call 1 width {width}")
        assert cnt == int(np.count_nonzero(exp1))
        gids, cnt = _flows(ac, torch, np.concatenate(parts2), pm.batch_offsets(parts2), s1, s2, width)
        _assert_codes(ac, gids, exp2, f"call 2 width {width}")
        assert cnt == int(np.count_nonzero(exp2))
        assert np.all(_state_values(s2) < ac.flow_states)
    # call 2 without call 1's states misses the patterns the cuts straddle
    gids, _ = _flows(ac, torch, np.concatenate(parts2), pm.batch_offsets(parts2), None, None)
    assert np.count_nonzero(ac._codes[gids] != exp2) > nseg // 4
    ac.free()
