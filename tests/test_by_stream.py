"""Per-stream sets on the device (pm_hip_events_by_stream_device,
pm_hip_events_by_stream; include/pm_hip.h "per-stream sets"): a match list
grouped by stream in CSR form, optionally one event per (stream, gid).
Expected values come from the host twin (pm_flat_events_by_stream), which
test_by_stream_cpu.py pins to numpy; the device's ranges are compared after
sorting each.  Every output buffer and the scratch carry poisoned guard slots
past their end, which must stay untouched."""
import collections
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from by_stream_inputs import (distinct_keys, first_difference, first_range_difference, mixed_offsets, pack, scan_like,
                              scattered)
from flow_inputs import input_f
from test_batch import _dev, _stream
from test_events import GUARD, POISON64, Ev, _text_dev
from oracle_lib import dict_paths
from test_gpu_parity import SHIP, _torch, fresh_matcher, matcher

pytestmark = pytest.mark.gpu

B = 1024  # the scan block's width (csrc/pm_bystream.h PM_BS_SCAN_BLOCK)
PTR_POISON = -0x5A5A5A5A5A5A5A5B
SCRATCH_GUARD = 256  # poisoned bytes past the scratch
NONE = ctypes.c_size_t(-1).value


_own = {}


def own_matcher():
    """An auto object over et of this module's own, for the HOST forms: they
    grow the object's staging, and tests of other modules measure that growth
    on the shared objects of `matcher`.  Same dictionary, so the same gids."""
    if "m" not in _own:
        m = pm.HipMatcher("auto")
        m.add_dictionary(pm.Dictionary(dict_paths("et")))
        m.compile()
        _own["m"] = m
    return _own["m"]


def _i64(torch, n, value):
    return torch.full((n,), value, dtype=torch.int64, device="cuda")


class Out:
    """The outputs and scratch of one device call, each in front of a guard."""

    def __init__(self, torch, m, cap, nseg, flags, out_cap, scratch_short=0):
        self.out_cap, self.nseg = out_cap, nseg
        self.out = _i64(torch, out_cap + GUARD, POISON64 - (1 << 64))
        self.ptr = _i64(torch, nseg + 1 + GUARD, PTR_POISON)
        self.bytes = m.lib.pm_hip_by_stream_scratch_bytes(cap, nseg, flags) - scratch_short
        self.scratch = torch.full((self.bytes + SCRATCH_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched(self):
        return (np.all(self.out.cpu().numpy().view(np.uint64) == POISON64)
                and np.all(self.ptr.cpu().numpy() == PTR_POISON) and np.all(self.scratch.cpu().numpy() == 0xA5))

    def result(self):
        """(stream_ptr, the out_cap slots) after the guards were checked."""
        ptr, out = self.ptr.cpu().numpy(), self.out.cpu().numpy().view(np.uint64)
        assert np.all(ptr[self.nseg + 1:] == PTR_POISON), "stream_ptr guard"
        assert np.all(out[self.out_cap:] == POISON64), "out guard"
        assert np.all(self.scratch.cpu().numpy()[self.bytes:] == 0xA5), "scratch guard"
        return ptr[:self.nseg + 1], out[:self.out_cap]


def _list_dev(torch, events, cap, cursor):
    """A device list of cap slots (+ guard) holding `events` first, poison
    after them, and its cursor."""
    ev = Ev(torch, cap, cursor=cursor)
    k = min(len(events), cap)
    if k:
        ev.buf[:k] = torch.from_numpy(np.ascontiguousarray(events[:k]).view(np.int64)).cuda()
    return ev


def _call(m, torch, ev, d_offs, nseg, flags, o):
    m.events_by_stream_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg, flags,
                              o.out.data_ptr(), o.out_cap, o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes,
                              _stream(torch))


def _sorted_ranges(ptr, out):
    """out[:ptr[-1]] with each stream's range ascending."""
    seg = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    body = out[:ptr[-1]]
    return body[np.lexsort((body, seg))]


def _assert_equals_twin(ptr, out, exp_ptr, exp_ev, what):
    """stream_ptr and the sorted ranges against the twin's; a difference names
    the first differing stream and its expected and observed counts."""
    diff = first_difference(ptr, exp_ptr)
    assert not diff, f"{what}: stream_ptr: {diff}"
    assert ptr[0] == 0 and ptr[-1] == exp_ptr[-1], what
    diff = first_range_difference(ptr, _sorted_ranges(ptr, out), exp_ev)
    assert not diff, f"{what}: {diff}"


def _run(events, offs, cap=None, cursor=None, out_cap=None, flags=(0, 1), key="et", kind="rt", m=None):
    """The device call on a hand-made list against the twin on the events it
    has to use, for each flag value (m: an object of the caller's own)."""
    torch = _torch()
    m = matcher(key, kind) if m is None else m
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    cap = len(events) if cap is None else cap
    cursor = len(events) if cursor is None else cursor
    used = events[:min(cursor, cap)]
    d_offs = _dev(torch, offs)
    res = {}
    for f in flags:
        exp_ptr, exp_ev = pm.events_by_stream_host(used, offs, unique=bool(f))
        ev = _list_dev(torch, events, cap, cursor)
        o = Out(torch, m, cap, nseg, f, cap if out_cap is None else out_cap)
        _call(m, torch, ev, d_offs, nseg, f, o)
        torch.cuda.synchronize()
        ptr, out = o.result()
        ev.assert_guard(cap)
        assert ev.total() == cursor
        _assert_equals_twin(ptr, out, exp_ptr, exp_ev, f"flags {f}")
        assert np.all(out[ptr[-1]:] == POISON64), f"flags {f}: a slot past the kept events was written"
        res[f] = (ptr, exp_ev)
    return res


# ---- 1. the hash ---------------------------------------------------------------
def test_one_key_4096_positions():
    rng = np.random.default_rng(1)
    pos = rng.permutation(np.arange(100, 100 + 4096))
    res = _run(pack(pos, np.full(4096, 7)), [0, 50, 5000, 6000])
    ptr, ev = res[1]
    assert ptr.tolist() == [0, 0, 1, 1] and ev.tolist() == pack([100], [7]).tolist()
    assert res[0][0].tolist() == [0, 0, 4096, 4096]


def test_4096_distinct_keys():
    rng = np.random.default_rng(2)
    ev = pack(rng.integers(0, 3000, size=4096), np.arange(1, 4097))
    res = _run(ev, np.arange(0, 3001, 100))
    assert res[1][0][-1] == 4096


@pytest.mark.parametrize("cap", [1023, 1024, 1025])
def test_cap_around_a_table_size_step(cap):
    lib = pm.load()
    assert lib.pm_hip_by_stream_scratch_bytes(1024, 1, 1) < lib.pm_hip_by_stream_scratch_bytes(1025, 1, 1)
    rng = np.random.default_rng(cap)
    ev = pack(rng.integers(0, 640, size=cap), rng.integers(1, 200, size=cap))
    _run(ev, np.arange(0, 641, 64))


def test_cursor_above_cap_uses_cap_events():
    rng = np.random.default_rng(3)
    ev = pack(rng.integers(0, 500, size=1500), rng.integers(1, 9, size=1500))
    _run(ev, [0, 100, 250, 500], cap=1500, cursor=1500 + 100000)


def test_cursor_below_cap_leaves_poison_unread():
    """The slots past the cursor hold 0xA5..: as an event, position
    0xA5A5A5A5A5 -- inside the last stream here, so reading one would show."""
    rng = np.random.default_rng(4)
    ev = pack(rng.integers(0, 500, size=700), rng.integers(1, 9, size=700))
    res = _run(ev, [0, 100, 250, 1 << 40], cap=2000, cursor=700)
    assert res[0][0][-1] == 700


# ---- 2. the lookup -----------------------------------------------------------------
def test_streams_of_0_and_1_byte():
    offs = np.array([3, 3, 4, 5, 5, 5, 6, 7, 7], dtype=np.int64)
    rng = np.random.default_rng(5)
    _run(pack(rng.integers(0, 10, size=1000), rng.integers(1, 4, size=1000)), offs)


def test_64_consecutive_events_in_64_streams():
    offs = np.arange(0, 65 * 10, 10)
    pos = np.arange(64) * 10 + 3
    res = _run(pack(np.concatenate([pos, pos[::-1], pos]), np.full(192, 5)), offs)
    assert np.all(np.diff(res[1][0]) == 1) and np.all(np.diff(res[0][0]) == 3)


def test_all_events_in_the_last_stream():
    offs = np.arange(0, 3001)  # 3,000 one-byte streams
    res = _run(pack(np.full(500, 2999), np.arange(1, 501)), offs)
    assert res[1][0][-2] == 0 and res[1][0][-1] == 500


def test_positions_above_2_32():
    base = (1 << 32) + 12345
    offs = base + np.array([0, 1000, 1000, 5000, 5001, 9000], dtype=np.int64)
    rng = np.random.default_rng(6)
    pos = base + rng.integers(-50, 9050, size=5000)
    res = _run(pack(pos, rng.choice([1, 2, (1 << 24) - 1], size=5000)), offs)
    assert 0 < res[0][0][-1] < 5000


def test_unsorted_offsets_stay_inside_the_arrays():
    """Offsets that are no offsets give an unspecified grouping; the guards and
    stream_ptr's shape hold whatever they are."""
    torch = _torch()
    m = matcher("et", "rt")
    rng = np.random.default_rng(10)
    events = pack(rng.integers(0, 5000, size=3000), rng.integers(1, 50, size=3000))
    for offs in (np.arange(5000, -1, -50), rng.integers(-100, 6000, size=300), np.zeros(40, np.int64)):
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        nseg = len(offs) - 1
        for flags in (0, 1):
            ev = _list_dev(torch, events, len(events), len(events))
            o = Out(torch, m, len(events), nseg, flags, len(events))
            _call(m, torch, ev, _dev(torch, offs), nseg, flags, o)
            torch.cuda.synchronize()
            ptr, out = o.result()
            assert ptr[0] == 0 and np.all(np.diff(ptr) >= 0) and ptr[-1] <= len(events)
            assert np.all(out[ptr[-1]:] == POISON64)


# ---- 3. counts and scatter -----------------------------------------------------------
def test_one_stream_holds_every_event_and_plain_keeps_the_multiset():
    rng = np.random.default_rng(7)
    n = 20000
    ev = pack(rng.integers(1000, 1200, size=n), rng.integers(1, 4, size=n))  # every event many times over
    res = _run(ev, [0, 1000, 2000, 2000])
    assert res[0][0].tolist() == [0, 0, n, n]
    assert collections.Counter(res[0][1].tolist()) == collections.Counter(ev.tolist())
    assert res[1][0].tolist() == [0, 0, 3, 3]


# ---- 4. the scan ---------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [1, B - 1, B, B + 1, B * B + 1])
def test_scan_sizes(nseg):
    """One-byte streams; events in the first, the last and random streams, so
    every level of the scan carries something (B * B + 1: the middle level
    takes a second turn)."""
    offs = np.arange(nseg + 1, dtype=np.int64) + 17
    rng = np.random.default_rng(nseg)
    pos = 17 + np.concatenate([[0, 0, nseg - 1, nseg - 1, nseg, -1], rng.integers(0, nseg, size=3000)])  # 2 outside
    res = _run(pack(pos, rng.integers(1, 3, size=len(pos))), offs)
    assert res[0][0][-1] == len(pos) - 2


# ---- 5. out_cap and scratch ------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, 1])
def test_out_cap_one_short(flags):
    torch = _torch()
    m = matcher("et", "rt")
    rng = np.random.default_rng(8)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 40, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    exp_ptr, exp_ev = pm.events_by_stream_host(events, offs, unique=bool(flags))
    kept = int(exp_ptr[-1])
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, flags, kept - 1)
    _call(m, torch, ev, _dev(torch, offs), nseg, flags, o)
    torch.cuda.synchronize()
    ptr, out = o.result()  # (the guard behind out_cap is checked there)
    assert np.array_equal(ptr, exp_ptr)
    # every stored slot holds an event of its stream's expected range, none more often than expected
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = collections.Counter(zip(seg.tolist(), exp_ev.tolist()))
    got = collections.Counter(zip(seg[:kept - 1].tolist(), out.tolist()))
    assert sum(got.values()) == kept - 1 and not got - want


def test_scratch_one_byte_short():
    torch = _torch()
    m = matcher("et", "rt")
    events = pack([1, 2, 3], [1, 1, 2])
    offs = np.array([0, 2, 4], dtype=np.int64)
    for flags in (0, 1):
        ev = _list_dev(torch, events, 3, 3)
        o = Out(torch, m, 3, 2, flags, 3, scratch_short=1)
        with pytest.raises(RuntimeError, match="bad arguments"):
            _call(m, torch, ev, _dev(torch, offs), 2, flags, o)
        torch.cuda.synchronize()
        assert o.untouched()
    _run(events, offs)  # exactly pm_hip_by_stream_scratch_bytes, in front of a guard: every _run


# ---- 6. chained behind real scans --------------------------------------------------------
def _chained(m, torch, scan, n, offs, min_len=3):
    """scan(ev) enqueues a list scan into ev; the by-stream call follows with
    no synchronize and no host read between, once per flag value (each on a
    fresh list).  Returns {flags: (list, stream_ptr, sorted ranges)}."""
    nseg = len(offs) - 1
    d_offs = _dev(torch, offs)
    res = {}
    for flags in (0, 1):
        ev = Ev(torch, 4 * n)
        o = Out(torch, m, ev.cap, nseg, flags, ev.cap)
        scan(ev, d_offs)
        _call(m, torch, ev, d_offs, nseg, flags, o)
        torch.cuda.synchronize()
        total = ev.total()
        assert 0 < total <= ev.cap
        lst = ev.slots()[:total]
        ev.assert_guard(total)
        ptr, out = o.result()
        exp_ptr, exp_ev = pm.events_by_stream_host(lst, offs, unique=bool(flags))
        assert np.array_equal(ptr, exp_ptr), flags
        assert np.array_equal(_sorted_ranges(ptr, out), exp_ev), flags
        assert np.all(out[ptr[-1]:] == POISON64)
        res[flags] = (lst, ptr, exp_ev)
    assert res[0][1][-1] == len(res[0][0])  # every event of a scan lies in a stream
    return res


def _assert_code_sets(m, res, offs, pos, codes):
    """Each stream's UNIQUE codes == the set of codes in its slice of the host list."""
    _, ptr, ev = res[1]
    got = m._codes[pm.unpack_events(ev)[1]]
    cut = np.searchsorted(pos, offs)
    assert ptr[-1] < len(pos), "the input has no pattern twice in a stream: UNIQUE is not exercised"
    for j in range(len(offs) - 1):
        assert np.array_equal(np.sort(got[ptr[j]:ptr[j + 1]]), np.unique(codes[cut[j]:cut[j + 1]])), j


def test_chained_after_batch_matches():
    torch = _torch()
    text, offs, _ = input_t("et")
    m = matcher("et", "rt")
    d_text = _text_dev(torch, text)

    def scan(ev, d_offs):
        m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(text), 3,
                                    ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    res = _chained(m, torch, scan, len(text), offs)
    pos, codes = own_matcher().read_batch_matches(text, offs, 3)
    assert len(pos) == len(res[0][0])
    _assert_code_sets(m, res, offs, pos, codes)


def test_chained_after_flow_matches():
    torch = _torch()
    data, offs, _ = input_f("et").calls[0]
    m = matcher("et", "ac")
    d_text = _text_dev(torch, data)

    def scan(ev, d_offs):
        m.scan_flows_matches_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, len(data), None, None, 3,
                                    ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    res = _chained(m, torch, scan, len(data), offs)
    pos, codes, _ = own_matcher().read_flows_matches(data, offs, None, 3)
    assert len(pos) == len(res[0][0])
    _assert_code_sets(m, res, offs, pos, codes)


# ---- 7. the host form and Python -----------------------------------------------------------
def test_host_form_equals_the_twin():
    m = own_matcher()
    rng = np.random.default_rng(9)
    offs = np.concatenate([[5], 5 + np.cumsum(rng.integers(0, 30, size=2500))]).astype(np.int64)
    events = pack(rng.integers(0, offs[-1] + 10, size=30000), rng.integers(1, 6, size=30000))
    for unique in (False, True):
        exp_ptr, exp_ev = pm.events_by_stream_host(events, offs, unique=unique)
        ptr, ev = m.events_by_stream(events, offs, unique=unique)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(ev, exp_ev)
    # the staging is counted: the list in and out, stream_ptr, the call's scratch
    assert m.scratch_bytes >= 16 * len(events) + 8 * len(offs) + m.by_stream_scratch_bytes(len(events), len(offs) - 1)
    ptr, ev = m.events_by_stream(np.empty(0, np.uint64), offs)
    assert not ptr.any() and len(ptr) == len(offs) and len(ev) == 0
    # out_cap short on the host form: stream_ptr complete, the first out_cap of the sorted ranges
    exp_ptr, exp_ev = pm.events_by_stream_host(events, offs, unique=True)
    out, ptr = np.full(100 + 8, POISON64, np.uint64), np.zeros(len(offs), np.int64)
    u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
    assert m.lib.pm_hip_events_by_stream(m.obj, events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p),
                                         len(offs) - 1, 1, out.ctypes.data_as(u64p), 100, ptr.ctypes.data_as(i64p)) == 0
    assert np.array_equal(ptr, exp_ptr) and np.array_equal(out[:100], exp_ev[:100]) and np.all(out[100:] == POISON64)


def test_read_many_sets():
    m = own_matcher()
    text, offs, _ = input_t("et")
    buffers = [bytes(text[offs[j]:offs[j + 1]]) for j in (0, 8, 11, 12, 20, 21, 22)] + [b"", b"x"]
    sets = m.read_many_sets(buffers, min_len=3)
    lists = m.read_many_matches(buffers, min_len=3)
    assert len(sets) == len(lists) == len(buffers)
    shrunk = 0
    for (spos, scodes), (pos, codes) in zip(sets, lists):
        uniq, first = np.unique(codes, return_index=True)  # pos ascends: the first index is the first position
        assert sorted(zip(scodes.tolist(), spos.tolist())) == list(zip(uniq.tolist(), pos[first].tolist()))
        shrunk += len(codes) - len(uniq)
    assert shrunk > 0
    longest = m.read_many_sets(buffers, min_len=3, all_matches=False)
    assert sum(len(c) for _, c in longest) <= sum(len(c) for _, c in sets)


# ---- 8. return codes ---------------------------------------------------------------------------
def test_return_codes_and_nothing_written():
    torch = _torch()
    m = matcher("et", "rt")
    lib = m.lib
    events = pack([1, 2, 3, 3], [1, 1, 2, 2])
    offs = np.array([0, 2, 4], dtype=np.int64)
    d_offs = _dev(torch, offs)
    ev = _list_dev(torch, events, 4, 4)
    for flags in (0, 1):
        o = Out(torch, m, 4, 2, flags, 4)
        good = dict(e=ev.buf.data_ptr(), cap=4, c=ev.nev.data_ptr(), o=d_offs.data_ptr(), nseg=2, f=flags,
                    out=o.out.data_ptr(), out_cap=4, p=o.ptr.data_ptr(), s=o.scratch.data_ptr(), sb=o.bytes,
                    st=_stream(torch))
        order = ("e", "cap", "c", "o", "nseg", "f", "out", "out_cap", "p", "s", "sb", "st")
        bad = [dict(e=None), dict(c=None), dict(o=None), dict(out=None), dict(p=None), dict(s=None),
               dict(e=good["e"] + 4), dict(c=good["c"] + 4), dict(o=good["o"] + 4), dict(out=good["out"] + 4),
               dict(p=good["p"] + 4), dict(s=good["s"] + 8), dict(nseg=-1), dict(nseg=1 << 31),
               dict(cap=(1 << 40) + 1), dict(f=flags | 2), dict(f=flags | (1 << 31)), dict(out=good["e"]),
               dict(sb=o.bytes - 1), dict(sb=0)]
        for b in bad:
            assert lib.pm_hip_events_by_stream_device(m.obj, *[{**good, **b}[k] for k in order]) == -2, b
            assert b"bad arguments" in lib.pm_hip_last_error(), b
        torch.cuda.synchronize()
        assert o.untouched()
        # nseg == 0: nothing launched or written, whatever the other pointers are
        assert lib.pm_hip_events_by_stream_device(m.obj, *[{**good, "nseg": 0, "o": None, "s": None, "sb": 0}[k]
                                                           for k in order]) == 0
        # cap == 0 with streams: an all-zero stream_ptr, nothing else
        assert lib.pm_hip_events_by_stream_device(m.obj, *[{**good, "cap": 0, "e": None}[k] for k in order]) == 0
        torch.cuda.synchronize()
        ptr, out = o.result()
        assert ptr.tolist() == [0, 0, 0] and np.all(out == POISON64)
    # before compile()
    fresh = pm.HipMatcher("rt")
    fresh.add_pattern(b"abc")
    o = Out(torch, m, 4, 2, 0, 4)
    args = [ev.buf.data_ptr(), 4, ev.nev.data_ptr(), d_offs.data_ptr(), 2, 0, o.out.data_ptr(), 4, o.ptr.data_ptr(),
            o.scratch.data_ptr(), o.bytes, _stream(torch)]
    assert lib.pm_hip_events_by_stream_device(fresh.obj, *args) == -1
    u64p, i64p = ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)
    out, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
    host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, 0, out.ctypes.data_as(u64p), 4,
            ptr.ctypes.data_as(i64p)]
    assert lib.pm_hip_events_by_stream(fresh.obj, *host) == -1
    torch.cuda.synchronize()
    assert o.untouched() and np.all(out == POISON64) and np.all(ptr == PTR_POISON)
    fresh.free()
    # the host form's -2 cases
    for k, v in ((0, None), (2, None), (7, None), (5, None), (3, 1 << 31), (1, (1 << 40) + 1), (4, 2),
                 (5, events.ctypes.data_as(u64p))):
        a = list(host)
        a[k] = v
        assert lib.pm_hip_events_by_stream(m.obj, *a) == -2, k
        assert b"bad arguments" in lib.pm_hip_last_error(), k
    assert np.all(out == POISON64) and np.all(ptr == PTR_POISON)
    assert lib.pm_hip_by_stream_scratch_bytes(1, -1, 0) == NONE


# ---- 9. past one grid, far positions, an empty list, the wave leaders --------------------------
_grid = {}


def _grid_inputs():
    """(lanes of one full grid, stream offsets, a scan_like list of two such
    grids and a wave, the generator behind it); made once."""
    if not _grid:
        lanes = 8 * 256 * _torch().cuda.get_device_properties(0).multi_processor_count  # bs_grid's cap
        rng = np.random.default_rng(11)
        offs = mixed_offsets(rng)
        assert {0, 1} <= set(np.diff(offs).tolist()) and np.diff(offs).max() >= 100000
        _grid["in"] = (lanes, offs, scan_like(2 * lanes + 64, offs, np.arange(1, 9), rng), rng)
    return _grid["in"]


@pytest.mark.parametrize("which", ["scan_like", "scattered", "distinct_keys", "a_wave_past_a_turn",
                                   "a_wave_short_of_a_turn"])
def test_more_events_than_one_grid(which):
    """A launch is capped at 8 workgroups of 256 lanes per CU (bs_grid): a list
    of two full turns of that grid and a ragged third, so that the grid-stride
    loops of all four event and table kernels turn again -- a wave meets a
    stream's count twice, the rounded tail of invalid lanes sits in the last
    turn, and UNIQUE's table has 2^21 slots or more (distinct_keys: exactly
    half full).  Streams of 0, 1, about 1,500 and one of about 100,000
    positions; gids 1..8, so nearly every event is a duplicate.  Then the
    scan_like list ending one wave past and one wave short of a whole turn.
    (One parameter per list: together they took 1.5 s, most of it the twin's.)"""
    lanes, offs, like, rng = _grid_inputs()
    n = 2 * lanes + 37
    if which == "scan_like":
        res = _run(like[:n], offs)
        assert res[0][0][-1] > n - n // 100 and res[1][0][-1] <= 8 * (len(offs) - 1)
    elif which == "scattered":
        _run(scattered(n, offs, np.arange(1, 9), rng), offs)
    elif which == "distinct_keys":
        pow2 = 1 << (n - 1).bit_length()
        assert pm.load().pm_hip_by_stream_scratch_bytes(pow2, 1, 1) >= 20 * max(2 * pow2, 1 << 21)
        res = _run(distinct_keys(pow2, offs, rng), offs)
        assert res[1][0][-1] == res[0][0][-1] == pow2  # nothing outside a stream, no key twice
    elif which == "a_wave_past_a_turn":
        _run(like, offs)
    else:
        _run(like[:2 * lanes - 64], offs)


def test_positions_up_to_2_40():
    """test_positions_above_2_32 at the top of the position field: the last
    stream ends at 2^40 and holds an event at 2^40 - 1, of a gid of its own so
    that UNIQUE keeps it too; the other gids include the largest."""
    top, gid_max = 1 << 40, (1 << 24) - 1
    base = top - 9100
    offs = base + np.array([0, 1000, 1000, 5000, 5001, 9100], dtype=np.int64)
    rng = np.random.default_rng(12)
    pos = np.append(base + rng.integers(-50, 9100, size=5000), top - 1)
    gid = np.append(rng.choice([1, 2, gid_max], size=5000), gid_max - 1)
    res = _run(pack(pos, gid), offs)
    assert 0 < res[0][0][-1] < 5001
    for f in (0, 1):
        kept_pos, kept_gid = pm.unpack_events(res[f][1])
        assert int(kept_pos.max()) == top - 1 and int(kept_gid.max()) == gid_max


def test_cursor_zero_with_room():
    """A list of 2,000 poisoned slots behind a cursor of 0: nothing is read
    (as an event the poison lies inside the last stream), stream_ptr is all
    zero and out untouched."""
    res = _run(np.empty(0, np.uint64), [0, 100, 250, 1 << 40], cap=2000, cursor=0)
    for f in (0, 1):
        assert res[f][0].tolist() == [0, 0, 0, 0] and len(res[f][1]) == 0  # (_run: every out slot is poison)


def test_wave_leaders():
    """Four waves (64 events at aligned indices) whose lane 0, the lane
    bs_stream_of searches for once per wave, is 1. below offsets[0]; 2. at
    offsets[nseg]; 3. in the last stream with every other lane in stream 0 (far
    below the leader: the search from the start); 4. in an interior stream with
    the other lanes alternating between the stream before and the one after."""
    offs = np.array([100, 110, 110, 130, 150, 170, 200], dtype=np.int64)  # stream 1 is empty
    lane = np.arange(64)
    w1 = np.where(lane == 0, 99, 110 + lane % 20)  # 63 events in stream 2
    w2 = np.where(lane == 0, 200, np.where(lane < 32, 250, 130 + lane % 20))  # 32 in stream 3, 32 outside
    w3 = np.where(lane == 0, 199, 100 + lane % 10)  # 1 in stream 5, 63 in stream 0
    w4 = np.where(lane == 0, 140, np.where(lane % 2 == 1, 129 - lane % 20, 150 + lane % 20))  # 1 / 32 / 31 in 3 / 2 / 4
    pos = np.concatenate([w1, w2, w3, w4])
    res = _run(pack(pos, 1 + np.tile(lane, 4) % 3), offs)
    assert res[0][0].tolist() == [0, 63, 63, 158, 191, 222, 223]
    assert res[1][0].tolist() == [0, 3, 3, 6, 9, 12, 13]


# ---- 10. captured behind a scan, and between served read_block calls ---------------------------
def test_captured_behind_a_scan_and_replayed():
    """scan_batch_matches_device, the by-stream call with flags 0 and, on
    outputs and scratch of its own, with flags 1, captured as one chain on a
    side stream and replayed three times, text B copied over the text in place
    before the second: every replay groups that replay's list; the scratch and
    stream_ptr are not reset between replays, so what one leaves behind (the
    counts, the table) would show in the next."""
    torch = _torch()
    text, offs, _ = input_t("et")
    other = np.ascontiguousarray(text[::-1])
    n, nseg = len(text), len(offs) - 1
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        d_text, d_offs = _text_dev(torch, text), _dev(torch, offs)
        ev = Ev(torch, 4 * n)
        outs = [Out(torch, m, ev.cap, nseg, flags, ev.cap) for flags in (0, 1)]
        # the scan alone once outside the capture: what it sets up on its first launch is set up
        m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, 3, ev.buf.data_ptr(), ev.cap,
                                    ev.nev.data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, 3, ev.buf.data_ptr(), ev.cap,
                                        ev.nev.data_ptr(), st.cuda_stream)
            for flags, o in enumerate(outs):
                m.events_by_stream_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg, flags,
                                          o.out.data_ptr(), o.out_cap, o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes,
                                          st.cuda_stream)
        torch.cuda.synchronize()
        seen = []
        for replay in range(3):
            if replay == 1:
                d_text[:n].copy_(torch.from_numpy(other))
            ev.nev.zero_()
            for o in outs:
                o.out[:o.out_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            total = ev.total()
            assert 0 < total <= ev.cap
            lst = ev.slots()[:total]
            seen.append([])
            for flags, o in enumerate(outs):
                ptr, out = o.result()
                exp_ptr, exp_ev = pm.events_by_stream_host(lst, offs, unique=bool(flags))
                _assert_equals_twin(ptr, out, exp_ptr, exp_ev, f"replay {replay}, flags {flags}")
                assert np.all(out[ptr[-1]:] == POISON64)
                seen[-1].append((ptr.copy(), exp_ev))
            assert seen[-1][0][0][-1] == total and seen[-1][1][0][-1] < total
        for flags in (0, 1):
            assert not np.array_equal(seen[0][flags][0], seen[1][flags][0])  # another text, another grouping
            assert np.array_equal(seen[1][flags][0], seen[2][flags][0])
            assert np.array_equal(seen[1][flags][1], seen[2][flags][1])
    finally:
        m.free()


def test_call_between_served_read_blocks():
    """Small read_block calls of an rt object go to its resident server grid;
    a by-stream device call after every third asks the grid to leave the
    device first, like every device launch, and the next small call launches
    it again: the gids equal one large call's, every by-stream result the
    twin's."""
    m = fresh_matcher("snort", "rt")
    try:
        sizes = [100 << 10] * 9
        text = np.tile(SHIP, 1 + sum(sizes) // len(SHIP))[:sum(sizes)]
        cuts = np.cumsum([0] + sizes)
        m.reset()
        whole = m.read_block_gids(text)  # > 256 Ki positions: the pipeline, not the server
        m.reset()
        s0 = m.serve_stats()
        rng = np.random.default_rng(13)
        offs = np.concatenate([[3], 3 + np.cumsum(rng.integers(0, 30, size=300))]).astype(np.int64)
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(m.read_block_gids(text[a:b]))
            if k % 3 == 2:
                events = pack(rng.integers(0, offs[-1] + 10, size=3000), rng.integers(1, 6, size=3000))
                _run(events, offs, m=m)
        assert np.array_equal(np.concatenate(parts), whole)
        s1 = m.serve_stats()
        assert s1["calls"] - s0["calls"] == len(sizes)
        assert s1["launches"] - s0["launches"] >= 3  # the first call, and the call after each stop
    finally:
        m.free()
