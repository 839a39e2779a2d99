"""Per-stream sets on the host: pm_flat_events_by_stream (the twin of
pm_hip_events_by_stream_device, include/pm_hip.h "per-stream sets") against a
dozen lines of numpy and a plain dict.  The function is pure in (events,
offsets), so positions sit near 2^40 and gids at 2^24 - 1 at no cost.  No
device."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import GID_MAX, pack, reference

U64P = ctypes.POINTER(ctypes.c_uint64)
I64P = ctypes.POINTER(ctypes.c_int64)
POISON64 = 0xA5A5A5A5A5A5A5A5
PTR_POISON = -0x5A5A5A5A5A5A5A5B


def twin_raw(events, offsets, flags, out_cap, guard=8):
    """One raw call: (rc, stream_ptr, out with `guard` poisoned slots past out_cap)."""
    ev = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offsets, dtype=np.int64)
    out = np.full(out_cap + guard, POISON64, dtype=np.uint64)
    ptr = np.full(len(offs), PTR_POISON, dtype=np.int64)
    rc = pm.load().pm_flat_events_by_stream(ev.ctypes.data_as(U64P), len(ev), offs.ctypes.data_as(I64P), len(offs) - 1,
                                            flags, out.ctypes.data_as(U64P), out_cap, ptr.ctypes.data_as(I64P))
    return rc, ptr, out


def check(events, offsets):
    for unique in (False, True):
        exp_ptr, exp_ev = reference(events, offsets, unique)
        rc, ptr, out = twin_raw(events, offsets, int(unique), len(events))
        assert rc == 0
        assert np.array_equal(ptr, exp_ptr), unique
        assert np.array_equal(out[:len(exp_ev)], exp_ev), unique
        assert np.all(out[len(exp_ev):] == POISON64), unique
        ptr2, ev2 = pm.events_by_stream_host(events, offsets, unique=unique)
        assert np.array_equal(ptr2, exp_ptr) and np.array_equal(ev2, exp_ev)
    return exp_ptr, exp_ev


def test_hand_case():
    ev = pack([5, 3, 12, 100, 10, 3], [7, 7, 2, 1, 7, 7])
    offs = [0, 10, 10, 20]
    ptr, out = pm.events_by_stream_host(ev, offs, unique=False)
    assert ptr.tolist() == [0, 3, 3, 5]
    assert out.tolist() == pack([3, 3, 5, 10, 12], [7, 7, 7, 7, 2]).tolist()
    ptr, out = pm.events_by_stream_host(ev, offs, unique=True)
    assert ptr.tolist() == [0, 1, 1, 3]
    assert out.tolist() == pack([3, 10, 12], [7, 7, 2]).tolist()
    check(ev, offs)


def test_positions_near_2_40_and_largest_gid():
    top = (1 << 40) - 1
    offs = np.array([top - 1000, top - 500, top - 500, top - 3, top + 1], dtype=np.int64)
    rng = np.random.default_rng(1)
    pos = np.append(rng.integers(top - 1100, top + 1, size=4000), top)  # some before offsets[0]
    gid = np.append(rng.choice([1, 2, GID_MAX], size=4000), GID_MAX)
    check(pack(pos, gid), offs)
    ptr, ev = pm.events_by_stream_host(pack(pos, gid), offs, unique=False)
    assert ptr[-1] > 0 and (ev & np.uint64(GID_MAX)).max() == GID_MAX and (ev >> np.uint64(24)).max() == top


def test_empty_streams_first_middle_last_and_one_byte_streams():
    offs = np.array([7, 7, 7, 8, 9, 9, 9, 10, 40, 40, 40], dtype=np.int64)  # 1-byte streams at 7, 8 and 9
    rng = np.random.default_rng(2)
    pos = rng.integers(0, 50, size=3000)  # below 7 and from 40 on: outside every stream
    events = pack(pos, rng.integers(1, 5, size=3000))
    check(events, offs)
    ptr, ev = pm.events_by_stream_host(events, offs, unique=False)
    assert np.all(np.diff(ptr)[[0, 1, 4, 5, 8, 9]] == 0) and np.all(np.diff(ptr)[[2, 3, 6, 7]] > 0)
    kept_pos = (ev >> np.uint64(24)).astype(np.int64)
    assert kept_pos.min() == 7 and kept_pos.max() == 39


def test_every_event_outside():
    ptr, ev = check(pack([0, 1, 30, 31, 1 << 39], [1, 2, 3, 4, 5]), [2, 10, 30])
    assert ptr.tolist() == [0, 0, 0] and len(ev) == 0


def test_no_events_and_no_streams():
    ptr, ev = check(np.empty(0, np.uint64), [0, 5, 9])
    assert ptr.tolist() == [0, 0, 0] and len(ev) == 0
    rc, ptr, out = twin_raw(pack([1], [1]), [0], 0, 4)  # nseg == 0: nothing written
    assert rc == 0 and ptr.tolist() == [PTR_POISON] and np.all(out == POISON64)


@pytest.mark.parametrize("unique", (False, True))
def test_out_cap_one_short(unique):
    rng = np.random.default_rng(3)
    ev = pack(rng.integers(0, 900, size=2000), rng.integers(1, 4, size=2000))
    offs = np.arange(0, 1001, 100)
    exp_ptr, exp_ev = reference(ev, offs, unique)
    rc, ptr, out = twin_raw(ev, offs, int(unique), len(exp_ev) - 1)
    assert rc == 0 and np.array_equal(ptr, exp_ptr)  # complete whatever out_cap is
    assert np.array_equal(out[:len(exp_ev) - 1], exp_ev[:-1])
    assert np.all(out[len(exp_ev) - 1:] == POISON64)
    rc, ptr, out = twin_raw(ev, offs, int(unique), 0)
    assert rc == 0 and np.array_equal(ptr, exp_ptr) and np.all(out == POISON64)


def test_bad_arguments():
    lib = pm.load()
    ev = pack([1, 2], [1, 1])
    offs = np.array([0, 4], dtype=np.int64)
    out = np.full(4, POISON64, dtype=np.uint64)
    ptr = np.full(2, PTR_POISON, dtype=np.int64)
    e, o, t, p = ev.ctypes.data_as(U64P), offs.ctypes.data_as(I64P), out.ctypes.data_as(U64P), ptr.ctypes.data_as(I64P)
    good = dict(events=e, nevents=2, offsets=o, nseg=1, flags=0, out=t, out_cap=4, stream_ptr=p)
    order = ("events", "nevents", "offsets", "nseg", "flags", "out", "out_cap", "stream_ptr")
    assert lib.pm_flat_events_by_stream(*[good[k] for k in order]) == 0
    out[:] = POISON64
    ptr[:] = PTR_POISON
    bad = [dict(events=None), dict(offsets=None), dict(stream_ptr=None), dict(out=None), dict(nseg=1 << 31),
           dict(nevents=(1 << 40) + 1), dict(flags=2), dict(flags=3), dict(flags=1 << 31), dict(out=e)]
    for b in bad:
        assert lib.pm_flat_events_by_stream(*[{**good, **b}[k] for k in order]) == -2, b
    assert np.all(out == POISON64) and np.all(ptr == PTR_POISON)
    # a NULL array with a zero count is no error
    assert lib.pm_flat_events_by_stream(None, 0, o, 1, 1, None, 0, p) == 0 and ptr.tolist() == [0, 0]


def test_scratch_bytes_is_the_documented_formula():
    lib = pm.load()

    def r16(b):
        return (b + 15) // 16 * 16
    for cap in (0, 1, 31, 32, 33, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 40):
        for nseg in (0, 1, 1023, 1024, 1025, 1024 * 1024 + 1, (1 << 31) - 1):
            tail = r16(8 * nseg) + r16(8 * ((nseg + 1023) // 1024))
            table = 64
            while table < 2 * cap:
                table *= 2
            assert lib.pm_hip_by_stream_scratch_bytes(cap, nseg, 0) == r16(4 * cap) + tail
            assert lib.pm_hip_by_stream_scratch_bytes(cap, nseg, 1) == 20 * table + tail
    none = ctypes.c_size_t(-1).value
    assert lib.pm_hip_by_stream_scratch_bytes((1 << 40) + 1, 1, 0) == none
    assert lib.pm_hip_by_stream_scratch_bytes(1, -1, 0) == none
    assert lib.pm_hip_by_stream_scratch_bytes(1, 1 << 31, 0) == none
    assert lib.pm_hip_by_stream_scratch_bytes(1, 1, 2) == none


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(seed):
    """nseg in 1..3000, stream lengths 0..40 with runs of empty streams, lists
    that are duplicate-heavy (gids from 3 values, a few hundred positions) or
    duplicate-free, in any order, some events outside every stream."""
    rng = np.random.default_rng(1000 + seed)
    for _ in range(4):
        nseg = int(rng.integers(1, 3001))
        lens = rng.integers(0, 41, size=nseg) * (rng.random(nseg) < 0.7)
        base = int(rng.integers(0, 1 << 39))
        offs = base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        n = int(rng.integers(0, 6000))
        lo, hi = base - 20, int(offs[-1]) + 20
        if rng.random() < 0.5:  # duplicate-heavy
            pos = rng.choice(rng.integers(lo, hi, size=300), size=n)
            ev = pack(pos, rng.choice([1, 77, GID_MAX], size=n))
        else:  # duplicate-free
            ev = np.unique(pack(rng.integers(lo, hi, size=n), rng.integers(1, 1 << 24, size=n)))
            rng.shuffle(ev)
        check(ev, offs)
