"""Ordered rules on the device (pm_hip_set_seq_rules,
pm_hip_seq_rules_by_stream_device, pm_hip_seq_rules_by_stream; include/pm_hip.h
"ordered rules"; csrc/pm_seqrules.hip): rules whose terms must follow one
another at a distance.  Hand-made lists are written straight to the device and
compared with the host twin (pm_flat_seq_rules_by_stream), which
test_seq_rules_cpu.py pins to the feasible-set reference; behind real scans the
expected hits come from the oracle's list through that reference.  The device's
ranges are compared after sorting each.  The hits, rule_ptr and the scratch
carry poisoned guard slots past their end, which must stay untouched; the hits
array has exactly the expected number of slots unless a test says otherwise."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import oracle_per_stream
from by_stream_inputs import first_difference, first_range_difference, mixed_offsets, scan_like
from fuzz_inputs import case as fuzz_case
from match_inputs import expected_matches
from oracle_lib import dict_paths
from rule_inputs import random_offsets, random_rules
from seq_rule_inputs import (KINDS, free_rules, kinds_present, pack, planted_case, random_seq_rules,
                             reference_seq_rules, seq_csr)
from test_batch import _dev, _stream
from test_by_stream import PTR_POISON, SCRATCH_GUARD, _i64, _list_dev, _sorted_ranges
from test_events import GUARD, POISON64, Ev, _text_dev
from test_gpu_parity import SHIP, _torch, fresh_matcher

pytestmark = pytest.mark.gpu

B = 1024  # the scan block's width (csrc/pm_bystream.h PM_BS_SCAN_BLOCK)
LANE = 16  # csrc/pm_seqrules.h PM_SQ_LANE_MAX: a longer range goes on the work list
LDS = 4096  # csrc/pm_seqrules.h PM_SQ_LDS_MAX: a longer range is sorted in parts and merged in global memory
NG = 4200  # the hand-made lists use gids 1..NG, all of them patterns of et
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))

_own = {}


def own_matcher():
    """An auto object over et of this module's own: set_seq_rules changes the
    object, and the host forms grow its staging."""
    if "m" not in _own:
        m = pm.HipMatcher("auto")
        m.add_dictionary(pm.Dictionary(dict_paths("et")))
        m.compile()
        _own["m"] = m
        _own["plen"] = np.array([0] + [m.pattern_len(g) for g in range(1, NG + 1)], dtype=np.uint32)
        assert _own["plen"][1:].min() > 0
    return _own["m"]


def plen():
    own_matcher()
    return _own["plen"]


class Out:
    """The outputs and scratch of one device call, each in front of a guard."""

    def __init__(self, torch, m, cap, nseg, hits_cap, scratch_short=0):
        self.hits_cap, self.nseg = hits_cap, nseg
        self.hits = _i64(torch, hits_cap + GUARD, POISON64 - (1 << 64))
        self.ptr = _i64(torch, nseg + 1 + GUARD, PTR_POISON)
        self.bytes = m.lib.pm_hip_seq_rules_scratch_bytes(cap, nseg) - scratch_short
        self.scratch = torch.full((self.bytes + SCRATCH_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched(self):
        return (np.all(self.hits.cpu().numpy().view(np.uint64) == POISON64)
                and np.all(self.ptr.cpu().numpy() == PTR_POISON) and np.all(self.scratch.cpu().numpy() == 0xA5))

    def result(self):
        """(rule_ptr, the hits_cap slots) after the guards were checked."""
        ptr, hits = self.ptr.cpu().numpy(), self.hits.cpu().numpy().view(np.uint64)
        assert np.all(ptr[self.nseg + 1:] == PTR_POISON), "rule_ptr guard"
        assert np.all(hits[self.hits_cap:] == POISON64), "hits guard"
        assert np.all(self.scratch.cpu().numpy()[self.bytes:] == 0xA5), "scratch guard"
        return ptr[:self.nseg + 1], hits[:self.hits_cap]


def _call(m, torch, ev, d_offs, nseg, o, stream=None):
    m.seq_rules_by_stream_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg,
                                 o.hits.data_ptr(), o.hits_cap, o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes,
                                 _stream(torch) if stream is None else stream)


def _assert_equal(ptr, hits, exp_ptr, exp_hits, what):
    diff = first_difference(ptr, exp_ptr)
    assert not diff, f"{what}: rule_ptr: {diff}"
    assert ptr[0] == 0 and ptr[-1] == exp_ptr[-1] == len(exp_hits), what
    diff = first_range_difference(ptr, _sorted_ranges(ptr, hits), exp_hits)
    assert not diff, f"{what}: {diff}"


def _run(events, offs, rules, fast=None, cap=None, cursor=None, m=None, set_rules=True, lens=None, what=""):
    """The device call on a hand-made list against the twin on the events it
    has to use, with room for exactly the expected hits.  Returns (rule_ptr,
    expected hits)."""
    torch = _torch()
    m = own_matcher() if m is None else m
    lens = plen() if lens is None else lens
    if set_rules:
        m.set_seq_rules(rules, fast)
        assert m.seq_rule_count() == len(rules)
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    cap = len(events) if cap is None else cap
    cursor = len(events) if cursor is None else cursor
    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(events[:min(cursor, cap)], offs, seq_csr(rules), lens)
    ev = _list_dev(torch, events, cap, cursor)
    o = Out(torch, m, cap, nseg, len(exp_hits))
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()
    ev.assert_guard(cap)
    assert ev.total() == cursor
    _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
    return ptr, exp_hits


# ---- 1. range lengths: the lane's sort, the LDS network, the merges in global memory ------
def _range_case(n, seed):
    """One (stream, gid 2) with n events -- three quarters of them distinct
    positions, the rest duplicates -- in shuffled order, behind one gid 1.
    Rules [1, then 2 at distance d] whose link is met by exactly zero bytes at
    the first, a middle and the last distinct position: only the exact lower
    bound in the sorted range gives that position; and one that needs a byte
    more than the last."""
    rng = np.random.default_rng(seed)
    L = int(plen()[2])
    distinct = max(n - n // 4, 1)
    a0 = 1000
    bpos = a0 + L + 5 + 3 * np.sort(rng.permutation(2 * distinct)[:distinct])
    pos = np.concatenate([bpos, bpos[rng.integers(0, distinct, size=n - distinct)]])
    events = np.concatenate([pack([a0], [1]), pack(rng.permutation(pos), np.full(n, 2))])
    want = [int(bpos[0]), int(bpos[distinct // 2]), int(bpos[-1])]
    rules = [[(1, None), (2, w - a0 - L)] for w in want] + [[(1, None), (2, want[-1] - a0 - L + 1)]]
    return events, [900, int(bpos[-1]) + 10], rules, want


@pytest.mark.parametrize("n", [1, 2, LANE - 1, LANE, LANE + 1, LDS - 1, LDS, LDS + 1, 2 * LDS, 2 * LDS + 1, 20000])
def test_range_lengths(n):
    events, offs, rules, want = _range_case(n, n)
    ptr, hits = _run(events, offs, rules, what=f"{n} positions")
    pos, rule = pm.unpack_events(hits)
    assert sorted(zip(rule.tolist(), pos.tolist())) == [(0, want[0]), (1, want[1]), (2, want[2])]


# ---- 2. work-list shapes ---------------------------------------------------------------
def _home(stream, gid, table):
    """The slot a (stream, gid) key hashes to (csrc/pm_bystream_dev.h bs_hash)."""
    key = (int(stream) << 24) | int(gid)
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - (table.bit_length() - 1))


def _aa_events(keys, offs, rng, n=LANE + 1, step=64):
    """Per (stream, gid) key n events at distinct positions step bytes apart,
    shuffled, and the rule gid ... gid whose link only the last one meets, by
    zero bytes (step * (n - 1) is at least every pattern length used)."""
    lens = plen()
    pos, gid, rules = [], [], {}
    for j, g in keys:
        p = int(offs[j]) + 5 + step * rng.permutation(n)
        pos += p.tolist()
        gid += [g] * n
        rules[g] = [(g, None), (g, step * (n - 1) - int(lens[g]))]
    order = rng.permutation(len(pos))
    return pack(np.array(pos)[order], np.array(gid)[order]), rules


def test_a_wave_whose_64_slots_all_hold_work_list_ranges_and_one_where_only_lane_63_does():
    """cap 2,048, so a table of 4,096 slots.  64 keys whose home slots are the
    64 slots of wave 3 and one key at slot 64 * 9 + 63, each with 17
    positions: every key sits at home, so wave 3 reserves 64 work-list entries
    at once and wave 9 one, for its last lane."""
    table, nseg = 4096, 64
    found = {}
    for j in range(nseg):
        for g in range(1, 1000):
            if plen()[g] <= 64 * LANE:
                found.setdefault(_home(j, g, table), (j, g))
    keys, gids = [], set()
    for slot in [3 * 64 + lane for lane in range(64)] + [9 * 64 + 63]:
        assert slot in found
        keys.append(found[slot])
        gids.add(found[slot][1])
    assert len({_home(j, g, table) for j, g in keys}) == len(keys) == 65
    offs = np.arange(nseg + 1, dtype=np.int64) * 2000 + 3
    events, by_gid = _aa_events(keys, offs, np.random.default_rng(31))
    rules = [by_gid[g] for g in sorted(gids)]
    ptr, hits = _run(events, offs, rules, cap=2048)
    assert ptr[-1] == 65
    assert pm.load().pm_hip_seq_rules_scratch_bytes(2048, nseg) >= 24 * table


def test_more_work_list_entries_than_the_sort_has_workgroups_and_none_at_all():
    """A range of 17 positions in each of 2,100 streams: 2,100 work-list
    entries, more than the 8 workgroups per CU of the sort's grid, whose loop
    turns again.  Then the same rules over a list without any long range."""
    torch = _torch()
    nseg = 2100
    assert nseg > 8 * torch.cuda.get_device_properties(0).multi_processor_count
    offs = np.arange(nseg + 1, dtype=np.int64) * 1200 + 7
    rng = np.random.default_rng(32)
    events, by_gid = _aa_events([(j, 5) for j in range(nseg)], offs, rng)
    ptr, hits = _run(events, offs, [by_gid[5]])
    assert ptr[-1] == nseg and np.all(np.diff(ptr) == 1)
    short, _ = _aa_events([(j, 5) for j in range(nseg)], offs, rng, n=LANE)
    ptr, hits = _run(short, offs, [by_gid[5]], set_rules=False)
    assert ptr[-1] == 0  # 16 positions: the last one is 64 bytes short of the link


# ---- 3. rule shapes ------------------------------------------------------------------------
def test_a_chain_of_64_terms():
    lens = plen()
    rule = [(1, None)] + [(g, 1) for g in range(2, 65)]
    p = [500]
    for g in range(2, 65):
        p.append(p[-1] + 1 + int(lens[g]))  # every link is met by exactly zero bytes
    events = pack(p, np.arange(1, 65))
    rng = np.random.default_rng(33)
    ptr, hits = _run(rng.permutation(events), [100, p[-1] + 1], [rule], fast=[40])
    assert hits.tolist() == [(p[-1] << 24)]
    early = events.copy()
    early[50] -= np.uint64(1 << 24)  # one term a byte early: its link fails
    ptr, hits = _run(rng.permutation(early), [100, p[-1] + 1], [rule], fast=[64])
    assert ptr[-1] == 0


def test_a_a_a_and_two_chains_a_free_term_and_a_negation():
    lens = plen()
    L1, L2, L4 = int(lens[1]), int(lens[2]), int(lens[4])
    rules = [[(1, None), (1, 3), (1, 3)],
             [(1, None), (2, 0), (-9, None), (3, None), (4, 2), (5, None)],
             [(1, None), (2, 0), (-8, None), (3, None), (4, 2), (5, None)]]
    s = 3 + L1
    ev = lambda at: [(at + 10, 1), (at + 10 + s - 1, 1), (at + 10 + s, 1), (at + 10 + 2 * s, 1),  # noqa: E731
                     (at + 10 + L2, 2), (at + 300, 3), (at + 300 + 2 + L4, 4), (at + 50, 5)]
    streams = [ev(1000) + [(1900, 8)], ev(2000)[:3] + ev(2000)[4:], ev(3000)[:6] + [(3300 + 1 + L4, 4)] + ev(3000)[7:]]
    pos = [p for st in streams for p, _ in st]
    gid = [g for st in streams for _, g in st]
    rng = np.random.default_rng(34)
    order = rng.permutation(len(pos))
    ptr, hits = _run(pack(np.array(pos)[order], np.array(gid)[order]), [1000, 2000, 3000, 4000], rules)
    hp, hr = pm.unpack_events(hits)
    got = sorted(zip(np.repeat(np.arange(3), np.diff(ptr)).tolist(), hr.tolist(), hp.tolist()))
    # stream 0: gid 8 kills rule 2; stream 1 lacks the third A; stream 2: D is a byte early
    assert got == [(0, 0, 1010 + 2 * s), (0, 1, 1300 + 2 + L4), (1, 1, 2300 + 2 + L4), (1, 2, 2300 + 2 + L4),
                   (2, 0, 3010 + 2 * s)]


def test_distance_0x7fffffff():
    big = 0x7FFFFFFF
    L, L3 = int(plen()[2]), int(plen()[3])
    a = (1 << 33) + 5
    # gid 2 meets the link by zero bytes, gid 3 misses it by one; a second link of that length ends past the stream
    events = pack([a, a + big + L3 - 1, a + big + L, a + 7], [1, 3, 2, 2])
    rules = [[(1, None), (2, big)], [(1, None), (3, big)], [(1, None), (2, big), (1, big)]]
    ptr, hits = _run(events, [1 << 33, (1 << 33) + (1 << 32)], rules)
    assert hits.tolist() == [((a + big + L) << 24)]


@pytest.mark.parametrize("seed", range(3))
def test_planted_kinds(seed):
    """seq_rule_inputs' planted streams with et's own pattern lengths: the
    failing-by-one and passing-by-zero pairs, a later occurrence, overlap, two
    chains, a negation, a neighbouring stream; the reference shows every kind
    and the device gives the reference's hits."""
    events, offs, rules, lens, plan = planted_case(50 + seed, plen=plen()[:13])
    ref = reference_seq_rules(events, offs, rules, lens)
    seen = kinds_present(plan, *ref)
    assert set(seen) == set(KINDS) and all(seen.values()), seen
    ptr, hits = _run(events, offs, rules)
    assert np.array_equal(ptr, ref[0]) and np.array_equal(hits, ref[1])


# ---- 4. the anchor's slot ----------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_one_slot_anchoring_n_rules(n):
    """gid 7 is the PM_RULE_FAST anchor of n rules: 7 following gid 100 + k, or
    the head of a chain, or beside a negation."""
    shapes = (lambda g: [(g, None), (7, 1)], lambda g: [(7, None), (g, 0)], lambda g: [(7, None), (-g, None)])
    rules = [shapes[k % 3](100 + k) for k in range(n)]
    rng = np.random.default_rng(n)
    offs = [5, 4000, 4000, 9000]
    events = pack(rng.integers(5, 9000, size=700), np.concatenate([[7] * 6, rng.integers(100, 100 + n + 5, size=694)]))
    ptr, hits = _run(events, offs, rules, fast=[7] * n, what=f"{n} rules")
    assert ptr[-1] > 0 or n == 1


def test_the_anchor_in_the_middle_and_at_the_end_of_a_chain():
    rng = np.random.default_rng(35)
    offs = random_offsets(rng, 60, max_len=300)
    events = pack(rng.integers(offs[0], offs[-1], size=4000), rng.integers(1, 7, size=4000))
    rules = random_seq_rules(rng, 80, np.arange(1, 7), max_pos=4, follow=0.9, max_gap=10)
    want = None
    for turn in range(3):  # the first, a middle and the last positive term as PM_RULE_FAST: the same hits
        fast = []
        for r in rules:
            positive = [g for g, _ in r if g > 0]
            fast.append(positive[(0, len(positive) // 2, len(positive) - 1)[turn]])
        ptr, hits = _run(events, offs, rules, fast=fast)
        want = (ptr, hits) if want is None else want
        assert ptr[-1] > 0 and np.array_equal(ptr, want[0]) and np.array_equal(hits, want[1])


# ---- 5. streams ----------------------------------------------------------------------------
@pytest.mark.parametrize("nseg", [1, B - 1, B, B + 1, 3000])
def test_scan_sizes(nseg):
    rng = np.random.default_rng(nseg)
    offs = random_offsets(rng, nseg, max_len=30, base=17)
    if offs[-1] == offs[0]:
        offs[-1] += 40
    pos = np.concatenate([[offs[0], offs[-1] - 1, offs[-1] - 1], rng.integers(offs[0] - 2, offs[-1] + 2, size=6000)])
    a, b, c, d = (int(g) for g in np.argsort(plen()[1:200], kind="stable")[:4] + 1)  # the shortest patterns
    events = pack(pos, np.concatenate([[a, a, c], rng.choice([a, b, c, d], size=6000)]))
    rules = [[(a, None)], [(a, None), (c, 0)], [(c, None), (a, 2), (-b, None)], [(b, None), (d, 0), (a, 0)],
             [(a, None), (a, 4)]]
    ptr, hits = _run(events, offs, rules)
    assert ptr[-1] > 0 and np.any(np.diff(offs) == 0) == (nseg > 1)


# ---- 6. list and table sizes ---------------------------------------------------------------
def test_more_slots_than_one_grid():
    """600,000 events: a table of 2^21 slots, more than one grid of lanes, so
    every table pass turns its loop again; eight gids over streams of which
    one is 100,000 bytes long, so ranges of every tier."""
    torch = _torch()
    lanes = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 600000
    assert pm.load().pm_hip_seq_rules_scratch_bytes(n, 1) >= 24 * (1 << 21) and lanes < (1 << 21)
    rng = np.random.default_rng(22)
    offs = mixed_offsets(rng)
    events = scan_like(n, offs, np.arange(1, 9), rng)
    rules = random_seq_rules(rng, 200, np.arange(1, 11), max_gap=40)
    ptr, hits = _run(events, offs, rules)
    assert ptr[-1] > 0


def test_a_half_full_table():
    n = 4096
    rng = np.random.default_rng(21)
    events = pack(100 + rng.integers(0, 50000, size=n), rng.permutation(np.arange(1, n + 1)))
    rules = random_seq_rules(rng, 500, np.arange(1, n + 1), max_pos=5, negated=0.2, max_gap=200)
    ptr, hits = _run(events, [100, 60000], rules, cap=n)
    assert ptr[-1] > 0


def test_cursor_above_cap_and_below_the_list():
    rng = np.random.default_rng(23)
    events = pack(rng.integers(0, 500, size=1500), rng.integers(1, 9, size=1500))
    rules = random_seq_rules(rng, 60, np.arange(1, 10))
    a, _ = _run(events, [0, 100, 250, 500], rules, cap=1500, cursor=1500 + 100000)
    # the slots past the cursor hold poison: as events they lie inside the last stream here
    b, _ = _run(events, [0, 100, 250, 1 << 40], rules, cap=2000, cursor=700, set_rules=False)
    assert a[-1] > 0 and b[-1] > 0
    c, _ = _run(np.empty(0, np.uint64), [0, 100, 250, 1 << 40], rules, cap=2000, cursor=0, set_rules=False)
    assert c.tolist() == [0, 0, 0, 0]


# ---- 7. hits_cap -------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["one", "all", "all_but_one"])
def test_hits_cap_short(short):
    """hits_cap one short of the hits, 0 and 1 (exact: every test through _run)."""
    torch = _torch()
    m = own_matcher()
    rng = np.random.default_rng(24)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 40, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    rules = random_seq_rules(rng, 900, np.arange(1, 42), max_pos=3, follow=0.5)
    m.set_seq_rules(rules)
    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(events, offs, rules, plen())
    total = int(exp_ptr[-1])
    assert total > len(events)  # more hits than events: the count is not bounded by cap
    hits_cap = {"one": total - 1, "all": 0, "all_but_one": 1}[short]
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, hits_cap)
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()  # (the guard behind hits_cap is checked there)
    assert np.array_equal(ptr, exp_ptr)
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = set(zip(seg.tolist(), exp_hits.tolist()))
    got = list(zip(seg[:hits_cap].tolist(), hits.tolist()))
    assert len(set(got)) == len(got) == hits_cap and set(got) <= want


# ---- 8. return codes and rule sets ---------------------------------------------------------
def test_before_set_seq_rules_is_minus_10_and_nothing_is_touched():
    torch = _torch()
    m = fresh_matcher("et", "rt")
    try:
        m.set_rules([[1, 2]])  # the rules' own set does not count
        m.set_flow_rules([[1, 2]])
        assert m.seq_rule_count() == 0 and m.seq_rules_min_len() == 0
        events = pack([1, 2, 3, 3], [1, 1, 2, 2])
        offs = np.array([0, 2, 4], dtype=np.int64)
        ev = _list_dev(torch, events, 4, 4)
        o = Out(torch, m, 4, 2, 4)
        args = [ev.buf.data_ptr(), 4, ev.nev.data_ptr(), _dev(torch, offs).data_ptr(), 2, o.hits.data_ptr(), 4,
                o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes, _stream(torch)]
        assert m.lib.pm_hip_seq_rules_by_stream_device(m.obj, *args) == -10
        assert b"pm_hip_set_seq_rules" in m.lib.pm_hip_last_error()
        hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
        host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, hits.ctypes.data_as(u64p), 4,
                ptr.ctypes.data_as(i64p)]
        assert m.lib.pm_hip_seq_rules_by_stream(m.obj, *host) == -10
        torch.cuda.synchronize()
        assert o.untouched() and np.all(hits == POISON64) and np.all(ptr == PTR_POISON)
        args[4] = -1  # bad arguments come first, as the return codes are ordered
        assert m.lib.pm_hip_seq_rules_by_stream_device(m.obj, *args) == -2
    finally:
        m.free()
    raw = pm.HipMatcher("rt")
    raw.add_pattern(b"abc")
    tptr, terms, gaps = seq_csr([[(1, None)]])
    assert raw.lib.pm_hip_set_seq_rules(raw.obj, tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                        gaps.ctypes.data_as(u32p), 1) == -1
    assert raw.lib.pm_hip_seq_rules_by_stream_device(raw.obj, *args) == -1
    raw.free()


def test_bad_arguments_are_minus_2_and_nothing_is_touched():
    torch = _torch()
    m = own_matcher()
    lib = m.lib
    m.set_seq_rules([[(1, None), (2, 0)], [(2, None)]])
    events = pack([1, 2, 3, 3], [1, 1, 2, 2])
    offs = np.array([0, 2, 4], dtype=np.int64)
    d_offs = _dev(torch, offs)
    ev = _list_dev(torch, events, 4, 4)
    o = Out(torch, m, 4, 2, 4)
    good = dict(e=ev.buf.data_ptr(), cap=4, c=ev.nev.data_ptr(), o=d_offs.data_ptr(), nseg=2, h=o.hits.data_ptr(),
                hits_cap=4, p=o.ptr.data_ptr(), s=o.scratch.data_ptr(), sb=o.bytes, st=_stream(torch))
    order = ("e", "cap", "c", "o", "nseg", "h", "hits_cap", "p", "s", "sb", "st")
    bad = [dict(e=None), dict(c=None), dict(o=None), dict(h=None), dict(p=None), dict(s=None), dict(e=good["e"] + 4),
           dict(c=good["c"] + 4), dict(o=good["o"] + 4), dict(h=good["h"] + 4), dict(p=good["p"] + 4),
           dict(s=good["s"] + 8), dict(nseg=-1), dict(nseg=1 << 31), dict(cap=(1 << 40) + 1), dict(h=good["e"]),
           dict(sb=o.bytes - 1), dict(sb=0), dict(sb=lib.pm_hip_rules_scratch_bytes(4, 2))]
    for b in bad:
        assert lib.pm_hip_seq_rules_by_stream_device(m.obj, *[{**good, **b}[k] for k in order]) == -2, b
        assert b"bad arguments" in lib.pm_hip_last_error(), b
    torch.cuda.synchronize()
    assert o.untouched()
    # nseg == 0: nothing launched or written, whatever the other pointers are
    assert lib.pm_hip_seq_rules_by_stream_device(m.obj, *[{**good, "nseg": 0, "o": None, "s": None, "sb": 0}[k]
                                                          for k in order]) == 0
    torch.cuda.synchronize()
    assert o.untouched()
    # cap == 0 with streams: an all-zero rule_ptr, nothing else
    assert lib.pm_hip_seq_rules_by_stream_device(m.obj, *[{**good, "cap": 0, "e": None}[k] for k in order]) == 0
    torch.cuda.synchronize()
    ptr, hits = o.result()
    assert ptr.tolist() == [0, 0, 0] and np.all(hits == POISON64)
    # the host form's -2 cases
    hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
    host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, hits.ctypes.data_as(u64p), 4,
            ptr.ctypes.data_as(i64p)]
    for k, v in ((0, None), (2, None), (6, None), (4, None), (3, 1 << 31), (1, (1 << 40) + 1),
                 (4, events.ctypes.data_as(u64p))):
        a = list(host)
        a[k] = v
        assert lib.pm_hip_seq_rules_by_stream(m.obj, *a) == -2, k
        assert b"bad arguments" in lib.pm_hip_last_error(), k
    assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON)
    assert lib.pm_hip_seq_rules_scratch_bytes(1, -1) == ctypes.c_size_t(-1).value


def test_every_bad_rule_set_is_minus_2_and_the_rules_stay():
    from test_seq_rules_cpu import bad_seq_rule_sets
    m = own_matcher()
    lib = m.lib
    rules = [[(1, None), (2, 0)], [(2, None), (-3, None)]]
    events = pack([1, 20, 50, 60, 70], [1, 2, 2, 3, 2])
    offs = [0, 40, 60, 90]
    want = _run(events, offs, rules)
    before = m.table_bytes
    npat = next(g for g in range(NG, 1 << 24) if m.pattern_len(g) == 0) - 1
    cases = bad_seq_rule_sets() + [("a gid above the last pattern", seq_csr([[(1, None), (npat + 1, 0)]]), None),
                                   ("gid 0", seq_csr([[(1, None), (0, 0)]]), None),
                                   ("the largest gid", seq_csr([[(1, None), ((1 << 24) - 1, 0)]]), None)]
    for name, (tptr, terms, gaps), nrules in cases:
        n = (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules
        rc = lib.pm_hip_set_seq_rules(m.obj, *[None if a is None else a.ctypes.data_as(u32p) for a in (tptr, terms, gaps)],
                                      n)
        assert rc == -2, name
        msg = lib.pm_hip_last_error()
        for word in (b"2^24", b"64", b"positive", b"twice", b"PM_RULE_FAST", b"negated", b"pattern", b"PM_SEQ_FREE",
                     b"0x7FFFFFFF", b"following"):
            assert word in msg, (name, word)
        assert m.seq_rule_count() == 2 and m.table_bytes == before, name
    got = _run(events, offs, rules, set_rules=False)
    assert want[0][-1] == 3 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_a_reload_replaces_the_rules_and_the_other_rule_sets_are_unaffected():
    m = own_matcher()
    rng = np.random.default_rng(25)
    events = pack(rng.integers(0, 300, size=2000), rng.integers(1, 30, size=2000))
    offs = np.arange(0, 301, 30)
    plain = random_rules(rng, 100, np.arange(1, 31))
    flow = random_rules(rng, 50, np.arange(1, 31), negated=0.0)
    m.set_rules(plain)
    m.set_flow_rules(flow)
    sets = np.zeros((len(offs) - 1, m.flow_rule_words), dtype=np.uint64)
    r0, f0 = m.rules_by_stream(events, offs), m.flow_rules(events, offs, sets, keep=True)
    first = random_seq_rules(rng, 300, np.arange(1, 31))
    second = random_seq_rules(rng, 40, np.arange(1, 31), max_pos=2)
    a, ha = _run(events, offs, first)
    base = m.table_bytes
    assert m.seq_rules_min_len() == min(m.pattern_len(abs(g)) for r in first for g, _ in r)
    b, hb = _run(events, offs, second)
    assert m.seq_rule_count() == 40 and m.table_bytes < base  # the first tables were freed and are no longer counted
    assert not np.array_equal(a, b)
    c, hc = _run(events, offs, first)
    assert np.array_equal(a, c) and np.array_equal(ha, hc) and m.table_bytes == base
    assert m.rule_count() == 100 and m.flow_rule_count() == 50
    r1, f1 = m.rules_by_stream(events, offs), m.flow_rules(events, offs, sets, keep=True)
    assert r0[0][-1] > 0 and f0[0][-1] > 0
    for x, y in ((r0, r1), (f0, f1)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])
    m.set_rules(plain[:10])  # nor does a rules reload touch the ordered rules
    d, hd = _run(events, offs, first, set_rules=False)
    assert np.array_equal(a, d) and np.array_equal(ha, hd)


# ---- 9. every gap free: the rules call ---------------------------------------------------------
def test_every_gap_free_gives_the_rules_calls_hits():
    from test_rules import Out as RulesOut, _call as rules_call
    torch = _torch()
    m = own_matcher()
    rng = np.random.default_rng(36)
    offs = random_offsets(rng, 500)
    events = pack(rng.integers(offs[0], offs[-1], size=20000), rng.integers(1, 25, size=20000))
    rules = random_rules(rng, 400, np.arange(1, 28))
    m.set_rules(rules)
    ptr, exp_hits = _run(events, offs, free_rules(rules))
    ev = _list_dev(torch, events, len(events), len(events))
    o = RulesOut(torch, m, len(events), len(offs) - 1, len(exp_hits))
    rules_call(m, torch, ev, _dev(torch, offs), len(offs) - 1, o)
    torch.cuda.synchronize()
    rptr, rhits = o.result()
    assert ptr[-1] > 0
    _assert_equal(rptr, rhits, ptr, exp_hits, "the rules call")


# ---- 10. fuzz ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(seed):
    rng = np.random.default_rng(200 + seed)
    nseg = int(rng.integers(1, 3001))
    offs = random_offsets(rng, nseg, max_len=int(rng.integers(20, 400)))
    n = int(rng.integers(1, 30000))
    ngid = int(rng.integers(2, 12))
    events = pack(rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n), rng.integers(1, ngid + 1, size=n))
    rules = random_seq_rules(rng, int(rng.integers(1, 400)), np.arange(1, ngid + 4), max_gap=int(rng.integers(0, 60)))
    fast = [None if rng.random() < 0.5 else int(rng.choice([g for g, _ in r if g > 0])) for r in rules]
    cap = n + int(rng.integers(0, 3)) * 100
    _run(events, offs, rules, fast=fast, cap=cap)


# ---- 11. behind real scans -----------------------------------------------------------------
def _planted_text(name):
    """A fuzz dictionary's text A with `P x* Q` and `Q x* P` planted in turn
    into the streams that have room (P, Q two patterns whose codes name one
    gid each, x a filler of 0 to 40 bytes of the text's own); the oracle's
    all-matches list of it at min_len 1 as events over gids; ordered rules
    over P, Q and the list's most frequent gids."""
    c = fuzz_case(name)
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    codes = np.asarray(m._codes, dtype=np.uint32)
    uniq, counts = np.unique(codes[1:], return_counts=True)
    single = set(uniq[counts == 1].tolist())
    lens = np.array([0] + [m.pattern_len(g) for g in range(1, len(codes))], dtype=np.uint32)
    pats = {code: b for _, code, b in __import__("oracle_lib").oracle_for(name).patterns()}
    rng = np.random.default_rng(37)
    cand = [g for g in range(1, len(codes)) if int(codes[g]) in single and 3 <= lens[g] <= 12]
    P, Q = (int(g) for g in rng.choice(cand, size=2, replace=False))
    bp, bq = pats[int(codes[P])], pats[int(codes[Q])]
    assert len(bp) == lens[P] and len(bq) == lens[Q]
    text = c.A.copy()
    planted = 0
    for j in range(c.nseg):
        a, b = int(c.offs[j]), int(c.offs[j + 1])
        gap = int(rng.integers(0, 41))
        if b - a < len(bp) + len(bq) + gap + 4:
            continue
        first, second = (bp, bq) if planted % 2 == 0 else (bq, bp)
        at = a + 2
        text[at:at + len(first)] = np.frombuffer(first, np.uint8)
        at += len(first) + gap
        text[at:at + len(second)] = np.frombuffer(second, np.uint8)
        planted += 1
    assert planted > 20
    exp = oracle_per_stream(name, text, c.offs)
    pos, pcodes = expected_matches(name, exp, 1)
    keep = np.isin(pcodes, uniq[counts == 1])  # the events whose code names one gid: the rules use only those
    order = np.argsort(codes)
    gids = order[np.searchsorted(codes[order], pcodes[keep])]
    assert np.array_equal(codes[gids], pcodes[keep])
    events = pack(pos[keep], gids)
    top = [int(g) for g in np.argsort(-np.bincount(gids))[:6] if g not in (P, Q)]
    rules = [[(P, None), (Q, 0)], [(Q, None), (P, 0)], [(P, None), (Q, 10)], [(Q, None), (P, 25), (-top[0], None)],
             [(P, None), (Q, 0), (P, 0)]] + random_seq_rules(rng, 60, [P, Q] + top, max_gap=30)
    return m, text, c.offs, events, rules, lens


@pytest.mark.parametrize("name", ["no_short", "seed4"])
def test_behind_the_batched_and_the_flow_scan(name):
    torch = _torch()
    m, text, offs, events, rules, lens = _planted_text(name)
    try:
        exp_ptr, exp_hits = reference_seq_rules(events, offs, rules, lens)
        fired = set((exp_hits & np.uint64(0xFFFFFF)).tolist())
        assert {0, 1} <= fired and exp_ptr[-1] > 40
        m.set_seq_rules(rules)
        min_len = m.seq_rules_min_len()
        nseg, n = len(offs) - 1, len(text)
        d_text, d_offs = _text_dev(torch, text), _dev(torch, offs)

        def batch(ev):
            m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, min_len, ev.buf.data_ptr(),
                                        ev.cap, ev.nev.data_ptr(), _stream(torch))

        def flow(ev):
            m.scan_flows_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, None, None, min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
        for what, scan in (("batch", batch), ("flow", flow)):
            ev = Ev(torch, 16 * n)
            o = Out(torch, m, ev.cap, nseg, len(exp_hits))
            scan(ev)
            _call(m, torch, ev, d_offs, nseg, o)  # no synchronize between
            torch.cuda.synchronize()
            assert 0 < ev.total() <= ev.cap, what
            ptr, hits = o.result()
            _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
    finally:
        m.free()


# ---- 12. read_many_seq_rules and the host form -------------------------------------------------
def test_read_many_seq_rules_and_the_host_form():
    m, text, offs, events, rules, lens = _planted_text("seed4")
    try:
        # first, while the staging is small: its hits array is short where the hits outnumber the events
        few = events[:1500]
        many = [[(int(g), None)] for g in np.unique(few & np.uint64(0xFFFFFF))] * 6
        m.set_seq_rules(many)
        p2, h2 = m.seq_rules_by_stream(few, offs)
        e2 = pm.seq_rules_by_stream_host(few, offs, many, lens)
        assert np.array_equal(p2, e2[0]) and np.array_equal(h2, e2[1]) and len(h2) > len(few)
        # hits_cap short on the host form: rule_ptr complete, the first hits_cap of the sorted ranges
        out, rp = np.full(10 + 8, POISON64, np.uint64), np.zeros(len(offs), np.int64)
        assert m.lib.pm_hip_seq_rules_by_stream(m.obj, few.ctypes.data_as(u64p), len(few), offs.ctypes.data_as(i64p),
                                                len(offs) - 1, out.ctypes.data_as(u64p), 10,
                                                rp.ctypes.data_as(i64p)) == 0
        assert np.array_equal(rp, e2[0]) and np.array_equal(out[:10], e2[1][:10]) and np.all(out[10:] == POISON64)
        # the host form on the whole list
        m.set_seq_rules(rules)
        exp_ptr, exp_hits = reference_seq_rules(events, offs, rules, lens)
        ptr, hits = m.seq_rules_by_stream(events, offs)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)
        assert m.scratch_bytes >= 8 * len(events) + m.seq_rules_scratch_bytes(len(events), len(offs) - 1)
        p0, h0 = m.seq_rules_by_stream(np.empty(0, np.uint64), offs)
        assert not p0.any() and len(p0) == len(offs) and len(h0) == 0
        # read_many_seq_rules on the streams with the most hits
        js = [int(j) for j in np.argsort(-np.diff(exp_ptr))[:10]] + [0, 1]
        got = m.read_many_seq_rules([bytes(text[offs[j]:offs[j + 1]]) for j in js])
        fired = 0
        for j, (gpos, grule) in zip(js, got):
            hp, hr = pm.unpack_events(exp_hits[exp_ptr[j]:exp_ptr[j + 1]])
            assert gpos.tolist() == (hp - offs[j]).tolist() and grule.tolist() == hr.tolist(), j
            fired += len(hr)
        assert fired >= 10
    finally:
        m.free()


# ---- 13. captured alone, and between served read_block calls ------------------------------------
def _replayed(n, step, span, noise_events, tight, zero_scratch):
    """The call captured alone on a side stream and replayed over three lists:
    40 ranges of n positions of gid 5, then 3 such ranges of gid 6 and fewer
    events, then 40 of gid 7 -- other table slots every time, so that a
    work-list entry left from an earlier replay names a slot that no longer
    holds the range.  Nothing is reset between the replays but what the call
    resets itself."""
    torch = _torch()
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        lens = plen()
        rng = np.random.default_rng(38)
        nseg = 40
        offs = np.arange(nseg + 1, dtype=np.int64) * span + 11
        noise = pack(rng.integers(offs[0], offs[-1], size=noise_events), rng.choice([1, 2, 3, 4, 8], size=noise_events))
        lists, rules = [], []
        for g, streams, keep in ((5, range(nseg), noise_events), (6, (3, 17, 39), noise_events // 3),
                                 (7, range(nseg), noise_events)):
            events, by_gid = _aa_events([(j, g) for j in streams], offs, rng, n=n, step=step)
            lists.append(np.concatenate([events, noise[:keep]]))
            rules.append(by_gid[g])
        rules += random_seq_rules(rng, 50, np.arange(1, 9), max_gap=100)
        m.set_seq_rules(rules)
        cap = len(lists[0]) + (0 if tight else 50)
        ev = Ev(torch, cap)
        d_offs = _dev(torch, offs)
        o = Out(torch, m, cap, nseg, 20000)
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            _call(m, torch, ev, d_offs, nseg, o, stream=st.cuda_stream)
        torch.cuda.synchronize()
        if zero_scratch:
            o.scratch[:o.bytes].zero_()
        seen = []
        for replay, lst in enumerate(lists):
            ev.buf[:len(lst)] = torch.from_numpy(lst.view(np.int64)).cuda()
            ev.nev.fill_(len(lst))
            o.hits[:o.hits_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            ptr, hits = o.result()
            exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, rules, lens)
            assert 0 < exp_ptr[-1] <= o.hits_cap, replay
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, f"list {replay}")
            assert np.all(hits[ptr[-1]:] == POISON64)
            seen.append(int(np.count_nonzero((exp_hits & np.uint64(0xFFFFFF)) == replay)))
        assert seen == [40, 3, 40]
        return cap
    finally:
        m.free()


def test_captured_alone_and_replayed_over_two_lists():
    """Ranges of 5,000 positions (the merges in global memory), a scratch that
    holds poison before the first replay: a work-list cursor that was not
    reset, or stale ranges, would show."""
    _replayed(n=5000, step=4, span=30000, noise_events=3000, tight=False, zero_scratch=False)


def test_replayed_with_a_cursor_that_starts_at_zero_and_a_work_list_that_is_nearly_full():
    """The same with ranges of 17 positions in a list of 699 events and no slot
    more, so that the work list holds 42 entries, and with a scratch of zeros
    before the first replay: a cursor that the call did not reset would be
    right the first time (0), plausible the second (40: the third of the 3 new
    entries finds no room) and past the list's end the third (43: none of the
    40 new ranges is listed, and the entries left from before name the slots
    of other keys, so none of them is sorted).  Passes with a poisoned scratch
    say nothing about this case: there an unreset cursor is wrong at once."""
    cap = _replayed(n=LANE + 1, step=64, span=2000, noise_events=19, tight=True, zero_scratch=True)
    assert cap == 699 and cap // (LANE + 1) + 1 == 42


def test_call_between_served_read_blocks():
    """Small read_block calls of an rt object go to its resident server grid;
    an ordered-rules call after every third asks the grid to leave the device
    first, like every device launch, and the next small call launches it
    again: the gids equal one large call's, every result the twin's."""
    m = fresh_matcher("snort", "rt")
    try:
        lens = np.array([0] + [m.pattern_len(g) for g in range(1, 8)], dtype=np.uint32)
        assert lens[1:].min() > 0
        sizes = [100 << 10] * 9
        text = np.tile(SHIP, 1 + sum(sizes) // len(SHIP))[:sum(sizes)]
        cuts = np.cumsum([0] + sizes)
        m.reset()
        whole = m.read_block_gids(text)  # > 256 Ki positions: the pipeline, not the server
        m.reset()
        s0 = m.serve_stats()
        rng = np.random.default_rng(28)
        offs = np.concatenate([[3], 3 + np.cumsum(rng.integers(0, 300, size=300))]).astype(np.int64)
        rules = random_seq_rules(rng, 50, np.arange(1, 7), max_gap=20)
        m.set_seq_rules(rules)
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(m.read_block_gids(text[a:b]))
            if k % 3 == 2:
                events = pack(rng.integers(0, offs[-1] + 10, size=3000), rng.integers(1, 6, size=3000))
                ptr, _ = _run(events, offs, rules, m=m, set_rules=False, lens=lens)
                assert ptr[-1] > 0
        assert np.array_equal(np.concatenate(parts), whole)
        s1 = m.serve_stats()
        assert s1["calls"] - s0["calls"] == len(sizes)
        assert s1["launches"] - s0["launches"] >= 3  # the first call, and the call after each stop
    finally:
        m.free()
