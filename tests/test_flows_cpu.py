"""The flow scan's contract without a device: input F's precondition, the
host step pm_flat_host_scan_flows over the dense rows of the flattened DFA
image, and FlowTable's bookkeeping.  CPU only."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from flow_inputs import F_FLOW_BYTES, F_FLOWS, input_f, precondition, shape_figures
from test_tables_cpu import image

U8P = ctypes.POINTER(ctypes.c_uint8)
U32P = ctypes.POINTER(ctypes.c_uint32)
I64P = ctypes.POINTER(ctypes.c_int64)

# (positions that differ from per-packet reset, those >= 8 bytes into their packet)
F_FIGURES = {"et": (10866, 4286), "snort": (11118, 4170), "merged": (12557, 4574)}


def host_flows(img, data, offs, state_in=None, want_state=True):
    """pm_flat_host_scan_flows: (rc, gids, state_out)."""
    data = np.ascontiguousarray(data, dtype=np.uint8)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    gids = np.zeros(max(len(data), 1), dtype=np.uint32)
    st_in = None if state_in is None else np.ascontiguousarray(state_in, dtype=np.uint32)
    st_out = np.full(max(nseg, 1), 0xFFFFFFFF, dtype=np.uint32)
    rc = img.lib.pm_flat_host_scan_flows(img.h, data.ctypes.data_as(U8P), offs.ctypes.data_as(I64P), nseg,
                                         None if st_in is None else st_in.ctypes.data_as(U32P),
                                         st_out.ctypes.data_as(U32P) if want_state else None, gids.ctypes.data_as(U32P))
    return rc, gids[:len(data)], st_out[:nseg]


def test_input_f_shape():
    assert shape_figures() == (46, 31, 784)


@pytest.mark.parametrize("key", ["et", "snort", "merged"])
def test_input_f_precondition(key):
    differ, deep = precondition(key)
    assert differ >= 5000 and deep >= 2000
    assert (differ, deep) == F_FIGURES[key]


def test_host_scan_flows_chained_calls():
    d, img, tab = image("et", pm.KIND_AC)
    F = input_f("et")
    states = img.lib.pm_flat_flow_states(img.h)
    assert states == len(img.array("out")) and states > 1
    state = None
    for r, (data, offs, exp) in enumerate(F.calls):
        rc, gids, out = host_flows(img, data, offs, state)
        assert rc == 0
        bad = np.nonzero(tab[gids] != exp)[0]
        assert bad.size == 0, f"call {r}: {bad.size} mismatches, first at {bad[:8]}"
        assert np.all(out < states)
        # empty streams return their incoming state
        empty = np.diff(offs) == 0
        prev = np.zeros(F_FLOWS, np.uint32) if state is None else state
        assert np.array_equal(out[empty], prev[empty]), r
        state = out
    assert sum(int(np.count_nonzero(np.diff(o) == 0)) for _, o, _ in F.calls) > 784  # the run-outs too
    # the final state of each flow: one call over the flow's whole 4,096 bytes
    whole = np.arange(F_FLOWS + 1, dtype=np.int64) * F_FLOW_BYTES
    rc, gids, final = host_flows(img, F.text, whole)
    assert rc == 0 and np.array_equal(tab[gids], F.exp)
    assert np.array_equal(state, final)
    assert np.count_nonzero(final) > F_FLOWS // 2  # deep text: most flows end inside a pattern


def test_host_scan_flows_state_rules():
    d, img, tab = image("et", pm.KIND_AC)
    F = input_f("et")
    states = img.lib.pm_flat_flow_states(img.h)
    data, offs = F.text[:4096], np.array([0, 0, 100, 100, 100, 1000, 4096, 4096], dtype=np.int64)
    # no state in: every stream from the root; no state out wanted
    rc, fresh, st_fresh = host_flows(img, data, offs)
    assert rc == 0
    rc, gids, _ = host_flows(img, data, offs, want_state=False)
    assert rc == 0 and np.array_equal(gids, fresh)
    rc, gids, st = host_flows(img, data, offs, np.zeros(7, np.uint32))
    assert rc == 0 and np.array_equal(gids, fresh) and np.array_equal(st, st_fresh)
    # a state >= pm_flat_flow_states behaves as 0, for empty streams too
    wild = np.array([states, 0xFFFFFFFF, states + 7, 1 << 20, 1 << 31, states, states], dtype=np.uint32)
    rc, gids, st = host_flows(img, data, offs, wild)
    assert rc == 0 and np.array_equal(gids, fresh) and np.array_equal(st, st_fresh)
    assert st[0] == 0 and st[2] == 0 and st[3] == 0 and st[6] == 0
    # a carried state changes the answers: the second half of a split equals the whole
    cut = int(offs[5]) + 37
    rc, head, st_head = host_flows(img, data[:cut], [0, cut])
    rc2, tail, st_tail = host_flows(img, data[cut:4096], [0, 4096 - cut], st_head)
    rc3, whole, st_whole = host_flows(img, data, [0, 4096])
    assert rc == 0 and rc2 == 0 and rc3 == 0
    assert np.array_equal(np.concatenate([head, tail]), whole) and st_tail[0] == st_whole[0]
    assert not np.array_equal(tail, host_flows(img, data[cut:4096], [0, 4096 - cut])[1])
    # in place: state_out may be state_in
    buf = st_head.copy()
    gids2 = np.zeros(4096 - cut, np.uint32)
    tail_data = np.ascontiguousarray(data[cut:4096])
    o2 = np.array([0, 4096 - cut], dtype=np.int64)
    rc = img.lib.pm_flat_host_scan_flows(img.h, tail_data.ctypes.data_as(U8P), o2.ctypes.data_as(I64P), 1,
                                         buf.ctypes.data_as(U32P), buf.ctypes.data_as(U32P), gids2.ctypes.data_as(U32P))
    assert rc == 0 and np.array_equal(gids2, tail) and buf[0] == st_whole[0]


def test_host_scan_flows_refuses_the_rt_image():
    d, img, tab = image("et", pm.KIND_RT)
    assert img.lib.pm_flat_flow_states(img.h) == 0
    rc, gids, st = host_flows(img, np.zeros(16, np.uint8), [0, 16])
    assert rc == -1 and not gids.any() and np.all(st == 0xFFFFFFFF)


class _StubMatcher:
    """read_flows_codes of a matcher whose 'state' is the number of bytes the
    flow has had, and whose codes are that count per position."""

    def __init__(self):
        self.calls = []

    def read_flows_codes(self, data, offsets, state=None):
        self.calls.append((bytes(data), offsets.tolist(), state.tolist()))
        codes = np.zeros(len(data), np.uint32)
        out = state.copy()
        for j, (a, b) in enumerate(zip(offsets[:-1].tolist(), offsets[1:].tolist())):
            codes[a:b] = int(state[j]) + 1 + np.arange(b - a)
            out[j] = state[j] + (b - a)
        return codes, out


def test_flow_table_bookkeeping():
    stub = _StubMatcher()
    flows = pm.FlowTable(stub)
    assert flows.scan([]) == [] and stub.calls == [] and len(flows) == 0
    got = flows.scan([("a", b"xyz"), (7, np.frombuffer(b"12", np.uint8)), (("t", 1), b"")])
    assert [g.tolist() for g in got] == [[1, 2, 3], [1, 2], []]
    assert stub.calls[-1] == (b"xyz12", [0, 3, 5, 5], [0, 0, 0])
    assert flows.states == {"a": 3, 7: 2, ("t", 1): 0} and "a" in flows and len(flows) == 3
    # one call per scan(), known flows continued, new ones fresh, any order
    got = flows.scan([(7, bytearray(b"q")), ("new", b"ab"), ("a", b"k")])
    assert len(stub.calls) == 2 and [g.tolist() for g in got] == [[3], [1, 2], [4]]
    assert stub.calls[-1][2] == [2, 0, 3]
    # a key twice in one call: refused before anything is scanned or recorded
    before = dict(flows.states)
    with pytest.raises(ValueError, match="twice"):
        flows.scan([("a", b"1"), ("b", b"2"), ("a", b"3")])
    assert len(stub.calls) == 2 and flows.states == before
    # end(): the key starts a fresh flow; an unknown key is not an error
    flows.end("a")
    flows.end("never seen")
    assert "a" not in flows
    assert flows.scan([("a", b"zz")])[0].tolist() == [1, 2] and flows.states["a"] == 2
