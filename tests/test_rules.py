"""Rules on the device (pm_hip_set_rules, pm_hip_rules_by_stream_device,
pm_hip_rules_by_stream; include/pm_hip.h "rules"; csrc/pm_rules.hip): which
multi-pattern rules fire in each stream of a match list.  Hand-made lists are
compared with the host twin (pm_flat_rules_by_stream), which test_rules_cpu.py
pins to the dict-and-set reference; behind real scans the expected hits come
from the oracle's list through that reference.  The device's ranges are
compared after sorting each.  The hits, rule_ptr and the scratch carry poisoned
guard slots past their end, which must stay untouched; the hits array has
exactly the expected number of slots unless a test says otherwise."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream
from by_stream_inputs import first_difference, first_range_difference, mixed_offsets, pack, scan_like
from fuzz_inputs import offsets as fuzz_offsets
from match_inputs import expected_matches
from oracle_lib import dict_paths
from rule_inputs import FAST, NEGATED, csr, random_offsets, random_rules, reference_rules
from test_batch import _dev, _stream
from test_by_stream import PTR_POISON, SCRATCH_GUARD, _i64, _list_dev, _sorted_ranges
from test_events import GUARD, POISON64, Ev, _text_dev
from test_gpu_parity import SHIP, _torch, fresh_matcher

pytestmark = pytest.mark.gpu

B = 1024  # the scan block's width (csrc/pm_bystream.h PM_BS_SCAN_BLOCK)
NG = 4200  # the hand-made lists use gids 1..NG, all of them patterns of et and of snort
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))

_own = {}


def own_matcher():
    """An auto object over et of this module's own: set_rules changes the
    object, and the host forms grow its staging."""
    if "m" not in _own:
        m = pm.HipMatcher("auto")
        m.add_dictionary(pm.Dictionary(dict_paths("et")))
        m.compile()
        assert all(m.pattern_len(g) > 0 for g in range(1, NG + 1))
        _own["m"] = m
    return _own["m"]


class Out:
    """The outputs and scratch of one device call, each in front of a guard."""

    def __init__(self, torch, m, cap, nseg, hits_cap, scratch_short=0):
        self.hits_cap, self.nseg = hits_cap, nseg
        self.hits = _i64(torch, hits_cap + GUARD, POISON64 - (1 << 64))
        self.ptr = _i64(torch, nseg + 1 + GUARD, PTR_POISON)
        self.bytes = m.lib.pm_hip_rules_scratch_bytes(cap, nseg) - scratch_short
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
    m.rules_by_stream_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg, o.hits.data_ptr(),
                             o.hits_cap, o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes,
                             _stream(torch) if stream is None else stream)


def _assert_equal(ptr, hits, exp_ptr, exp_hits, what):
    diff = first_difference(ptr, exp_ptr)
    assert not diff, f"{what}: rule_ptr: {diff}"
    assert ptr[0] == 0 and ptr[-1] == exp_ptr[-1] == len(exp_hits), what
    diff = first_range_difference(ptr, _sorted_ranges(ptr, hits), exp_hits)
    assert not diff, f"{what}: {diff}"


def _run(events, offs, rules, fast=None, cap=None, cursor=None, m=None, set_rules=True, what=""):
    """The device call on a hand-made list against the twin on the events it
    has to use, with room for exactly the expected hits.  Returns (rule_ptr,
    expected hits)."""
    torch = _torch()
    m = own_matcher() if m is None else m
    if set_rules:
        m.set_rules(rules, fast)
        assert m.rule_count() == len(rules)
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    cap = len(events) if cap is None else cap
    cursor = len(events) if cursor is None else cursor
    exp_ptr, exp_hits = pm.rules_by_stream_host(events[:min(cursor, cap)], offs, rules)
    ev = _list_dev(torch, events, cap, cursor)
    o = Out(torch, m, cap, nseg, len(exp_hits))
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()
    ev.assert_guard(cap)
    assert ev.total() == cursor
    _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
    return ptr, exp_hits


# ---- 1. the per-lane turns ---------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 255, 256, 257, 1000])
def test_one_slot_anchoring_n_rules(n):
    """gid 7 is the PM_RULE_FAST anchor of n rules [7, g] / [7, -g]: one table
    slot per stream holds it, and its wave verifies them a rule per lane in
    turns of 64 -- one lane, a turn one short, a full turn, a turn and a lane,
    three turns and a partial fourth, then the same edges around four turns
    and 1,000 rules (sixteen turns)."""
    rules = [[7, 100 + k] if k % 3 else [7, -(100 + k)] for k in range(n)]
    rng = np.random.default_rng(n)
    offs = [5, 400, 400, 900]
    events = pack(rng.integers(5, 900, size=500), np.concatenate([[7, 7], rng.integers(100, 100 + n + 5, size=498)]))
    ptr, hits = _run(events, offs, rules, fast=[7] * n, what=f"{n} rules")
    assert ptr[-1] > 0 or n == 1


def _home(stream, gid, table):
    """The slot a (stream, gid) key hashes to (csrc/pm_bystream_dev.h bs_hash)."""
    key = (int(stream) << 24) | int(gid)
    return ((key * 0x9E3779B97F4A7C15) & ((1 << 64) - 1)) >> (64 - (table.bit_length() - 1))


def _keys_by_home(nseg, gids, table):
    """home slot -> one (stream, gid) that hashes there."""
    found = {}
    for j in range(nseg):
        for g in gids:
            found.setdefault(_home(j, g, table), (j, g))
    return found


def test_a_wave_in_which_every_slot_anchors_and_one_in_which_only_lane_63_does():
    """cap 1,024, so a table of 2,048 slots.  64 keys whose home slots are the
    64 slots of wave 3 and are distinct (nothing probes: each sits at home),
    every gid among them the anchor of two rules; one key at slot 64 * 9 + 63,
    the anchor of a rule whose other term's key lies in another wave."""
    table, nseg = 2048, 64
    by_home = _keys_by_home(nseg, range(1, 1000), table)
    assert len(by_home) == table
    full = [by_home[3 * 64 + lane] for lane in range(64)]
    last = by_home[9 * 64 + 63]
    other = next(k for h, k in by_home.items() if h // 64 not in (3, 9) and k[0] == last[0] and k[1] != last[1]
                 and k[1] not in {g for _, g in full})
    assert last[1] not in {g for _, g in full}
    offs = np.arange(nseg + 1, dtype=np.int64) * 10 + 3
    keys = full + [last, other]
    events = pack([offs[j] + (g % 10) for j, g in keys], [g for _, g in keys])
    assert len({_home(j, g, table) for j, g in keys}) == len(keys)  # every key sits at home
    rules = []
    for g in sorted({g for _, g in full}):
        rules += [[g], [g, -4000]]
    rules.append([last[1], other[1]])
    fast = [r[0] for r in rules]
    ptr, hits = _run(events, offs, rules, fast=fast, cap=1024)
    assert ptr[-1] == 2 * 64 + 1
    assert pm.load().pm_hip_rules_scratch_bytes(1024, nseg) >= 16 * table


def test_terms_in_a_long_probe_run():
    """4,096 distinct keys of one stream in a list of cap 4,096: the table's
    8,192 slots are exactly half full, so the probe runs are as long as they
    get.  Rules over those gids, some with a negated gid that is absent and
    some with one that is present."""
    n = 4096
    assert pm.load().pm_hip_rules_scratch_bytes(n, 1) == 16 * 2 * n + 16 + 16
    rng = np.random.default_rng(21)
    events = pack(100 + rng.integers(0, 50000, size=n), rng.permutation(np.arange(1, n + 1)))
    rules = random_rules(rng, 500, np.arange(1, n + 1), max_pos=6, negated=0.0)
    rules += [r + [-(n + 1 + k % 50)] for k, r in enumerate(rules[:100])] + [r + [-int(r[0] % n + 1)] for r in rules[:50]
                                                                            if r[0] % n + 1 not in r]
    ptr, hits = _run(events, [100, 60000], rules, cap=n)
    assert ptr[-1] == 600


# ---- 2. past one grid --------------------------------------------------------------
def test_more_slots_than_one_grid():
    """600,000 events: a table of 2^21 slots, more than one grid of lanes
    (8 workgroups of 256 per CU), so the grid-stride loop of both evaluations
    turns again; rules fire in the first and in the last stream."""
    torch = _torch()
    lanes = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 600000
    assert pm.load().pm_hip_rules_scratch_bytes(n, 1) >= 16 * (1 << 21) and lanes < (1 << 21)
    rng = np.random.default_rng(22)
    offs = mixed_offsets(rng)
    full = np.nonzero(np.diff(offs) > 0)[0]
    first, last = int(full[0]), int(full[-1])
    events = scan_like(n - 4, offs, np.arange(1, 9), rng)
    events = np.concatenate([events, pack([offs[first], offs[first], offs[last + 1] - 1, offs[last + 1] - 1],
                                          [20, 21, 20, 21])])
    rules = random_rules(rng, 200, np.arange(1, 11)) + [[20, 21], [21, 20, -1], [21, 20, -22]]
    ptr, hits = _run(events, offs, rules)
    ends = pm.unpack_events(hits)[1]
    assert 200 in ends[ptr[first]:ptr[first + 1]] and 202 in ends[ptr[last]:ptr[last + 1]]


# ---- 3. the scan's block edges -------------------------------------------------------
@pytest.mark.parametrize("nseg", [1, B - 1, B, B + 1, 3000])
def test_scan_sizes(nseg):
    rng = np.random.default_rng(nseg)
    offs = random_offsets(rng, nseg, max_len=3, base=17)
    if offs[-1] == offs[0]:
        offs[-1] += 2
    pos = np.concatenate([[offs[0], offs[-1] - 1, offs[-1] - 1], rng.integers(offs[0] - 2, offs[-1] + 2, size=4000)])
    events = pack(pos, np.concatenate([[1, 1, 2], rng.integers(1, 6, size=4000)]))
    rules = [[1], [1, 2], [2, -3], [3, 4, 5], [5, -1]]
    ptr, hits = _run(events, offs, rules)
    assert ptr[-1] > 0 and np.any(np.diff(offs) == 0) == (nseg > 1)


# ---- 4. the cursor -------------------------------------------------------------------
def test_cursor_above_cap_and_below_the_list():
    rng = np.random.default_rng(23)
    events = pack(rng.integers(0, 500, size=1500), rng.integers(1, 9, size=1500))
    rules = random_rules(rng, 60, np.arange(1, 10))
    a, _ = _run(events, [0, 100, 250, 500], rules, cap=1500, cursor=1500 + 100000)
    # the slots past the cursor hold poison: as events they lie inside the last stream here
    b, _ = _run(events, [0, 100, 250, 1 << 40], rules, cap=2000, cursor=700, set_rules=False)
    assert a[-1] > 0 and b[-1] > 0
    c, _ = _run(np.empty(0, np.uint64), [0, 100, 250, 1 << 40], rules, cap=2000, cursor=0, set_rules=False)
    assert c.tolist() == [0, 0, 0, 0]


# ---- 5. hits_cap ---------------------------------------------------------------------
@pytest.mark.parametrize("short", ["one", "all"])
def test_hits_cap_short(short):
    torch = _torch()
    m = own_matcher()
    rng = np.random.default_rng(24)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 40, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    rules = random_rules(rng, 600, np.arange(1, 42))
    m.set_rules(rules)
    exp_ptr, exp_hits = pm.rules_by_stream_host(events, offs, rules)
    total = int(exp_ptr[-1])
    assert total > len(events)  # more hits than events: the count is not bounded by cap
    hits_cap = total - 1 if short == "one" else 0
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, hits_cap)
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()  # (the guard behind hits_cap is checked there)
    assert np.array_equal(ptr, exp_ptr)
    # every stored slot holds a hit of its stream's expected range, none more often than expected
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = set(zip(seg.tolist(), exp_hits.tolist()))
    got = list(zip(seg[:hits_cap].tolist(), hits.tolist()))
    assert len(set(got)) == len(got) == hits_cap and set(got) <= want


# ---- 6. return codes -------------------------------------------------------------------
def test_before_set_rules_is_minus_10_and_nothing_is_touched():
    torch = _torch()
    m = fresh_matcher("et", "rt")
    try:
        assert m.rule_count() == 0 and m.rules_min_len() == 0
        events = pack([1, 2, 3, 3], [1, 1, 2, 2])
        offs = np.array([0, 2, 4], dtype=np.int64)
        ev = _list_dev(torch, events, 4, 4)
        o = Out(torch, m, 4, 2, 4)
        args = [ev.buf.data_ptr(), 4, ev.nev.data_ptr(), _dev(torch, offs).data_ptr(), 2, o.hits.data_ptr(), 4,
                o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes, _stream(torch)]
        assert m.lib.pm_hip_rules_by_stream_device(m.obj, *args) == -10
        assert b"pm_hip_set_rules" in m.lib.pm_hip_last_error()
        hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
        host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, hits.ctypes.data_as(u64p), 4,
                ptr.ctypes.data_as(i64p)]
        assert m.lib.pm_hip_rules_by_stream(m.obj, *host) == -10
        torch.cuda.synchronize()
        assert o.untouched() and np.all(hits == POISON64) and np.all(ptr == PTR_POISON)
        # bad arguments come first, as the return codes are ordered
        args[4] = -1
        assert m.lib.pm_hip_rules_by_stream_device(m.obj, *args) == -2
    finally:
        m.free()
    raw = pm.HipMatcher("rt")
    raw.add_pattern(b"abc")
    tptr, terms = csr([[1]])
    assert raw.lib.pm_hip_set_rules(raw.obj, tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), 1) == -1
    assert raw.lib.pm_hip_rules_by_stream_device(raw.obj, *args) == -1
    raw.free()


def test_bad_arguments_are_minus_2_and_nothing_is_touched():
    torch = _torch()
    m = own_matcher()
    lib = m.lib
    m.set_rules([[1, 2], [2]])
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
           dict(sb=o.bytes - 1), dict(sb=0)]
    for b in bad:
        assert lib.pm_hip_rules_by_stream_device(m.obj, *[{**good, **b}[k] for k in order]) == -2, b
        assert b"bad arguments" in lib.pm_hip_last_error(), b
    torch.cuda.synchronize()
    assert o.untouched()
    # nseg == 0: nothing launched or written, whatever the other pointers are
    assert lib.pm_hip_rules_by_stream_device(m.obj, *[{**good, "nseg": 0, "o": None, "s": None, "sb": 0}[k]
                                                      for k in order]) == 0
    torch.cuda.synchronize()
    assert o.untouched()
    # cap == 0 with streams: an all-zero rule_ptr, nothing else
    assert lib.pm_hip_rules_by_stream_device(m.obj, *[{**good, "cap": 0, "e": None}[k] for k in order]) == 0
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
        assert lib.pm_hip_rules_by_stream(m.obj, *a) == -2, k
        assert b"bad arguments" in lib.pm_hip_last_error(), k
    assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON)
    assert lib.pm_hip_rules_scratch_bytes(1, -1) == ctypes.c_size_t(-1).value


def test_every_bad_rule_set_is_minus_2_and_the_rules_stay():
    from test_rules_cpu import bad_rule_sets
    m = own_matcher()
    lib = m.lib
    rules = [[1, 2], [2, -3]]
    events = pack([1, 2, 5, 6, 7], [1, 2, 2, 3, 2])
    offs = [0, 4, 6, 9]
    want = _run(events, offs, rules)
    before = m.table_bytes
    npat = next(g for g in range(NG, 1 << 24) if m.pattern_len(g) == 0) - 1
    cases = bad_rule_sets() + [("a gid above the last pattern", *csr([[1, npat + 1]]), None),
                               ("gid 0", *csr([[1, 0]]), None), ("the largest gid", *csr([[1, (1 << 24) - 1]]), None)]
    for name, tptr, terms, nrules in cases:
        n = (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules
        rc = lib.pm_hip_set_rules(m.obj, None if tptr is None else tptr.ctypes.data_as(u32p),
                                  None if terms is None else terms.ctypes.data_as(u32p), n)
        assert rc == -2, name
        msg = lib.pm_hip_last_error()
        for word in (b"2^24", b"64", b"positive", b"twice", b"PM_RULE_FAST", b"negated", b"pattern"):
            assert word in msg, (name, word)
        assert m.rule_count() == 2 and m.table_bytes == before, name
    got = _run(events, offs, rules, set_rules=False)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_set_rules_again_replaces_the_rules():
    m = own_matcher()
    rng = np.random.default_rng(25)
    events = pack(rng.integers(0, 300, size=2000), rng.integers(1, 30, size=2000))
    offs = np.arange(0, 301, 30)
    first = random_rules(rng, 300, np.arange(1, 31))
    second = random_rules(rng, 40, np.arange(1, 31), max_pos=2)
    a, ha = _run(events, offs, first)
    base = m.table_bytes
    assert m.rules_min_len() == min(m.pattern_len(abs(g)) for r in first for g in r)
    b, hb = _run(events, offs, second)
    assert m.rule_count() == 40 and m.table_bytes < base  # the first tables were freed and are no longer counted
    assert not np.array_equal(a, b)
    c, hc = _run(events, offs, first)
    assert np.array_equal(a, c) and np.array_equal(ha, hc) and m.table_bytes == base


# ---- 7. fuzz ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(seed):
    rng = np.random.default_rng(200 + seed)
    nseg = int(rng.integers(1, 3001))
    offs = random_offsets(rng, nseg)
    n = int(rng.integers(1, 20000))
    ngid = int(rng.integers(2, 30))
    events = pack(rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n), rng.integers(1, ngid + 1, size=n))
    rules = random_rules(rng, int(rng.integers(1, 400)), np.arange(1, ngid + 4))
    fast = [None if rng.random() < 0.5 else int(rng.choice([g for g in r if g > 0])) for r in rules]
    cap = n + int(rng.integers(0, 3)) * 100
    ptr, hits = _run(events, offs, rules, fast=fast, cap=cap)
    exp_ptr, exp_hits = reference_rules(events, offs, rules)
    assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)


# ---- 8. behind real scans ----------------------------------------------------------------
_real = {}


def _real_inputs():
    """et's input T text over fuzz_inputs' stream offsets; the oracle's
    all-matches list of it as (position, gid) events; rules drawn from the
    gids a stream's set holds (they fire there) with negated gids that are
    present, absent from the stream or absent from the list, and rules over
    gids the list does not hold.  Every term's pattern has at least 3 bytes."""
    if not _real:
        m = own_matcher()
        text = input_t("et")[0]
        offs = fuzz_offsets(len(text))
        exp = oracle_per_stream("et", text, offs)
        codes = np.asarray(m._codes, dtype=np.uint32)
        assert len(np.unique(codes[1:])) == len(codes) - 1  # a code names one gid
        order = np.argsort(codes)
        pos, pcodes = expected_matches("et", exp, 3)
        gids = order[np.searchsorted(codes[order], pcodes)]
        assert np.array_equal(codes[gids], pcodes)
        events = pack(pos, gids)
        rng = np.random.default_rng(26)
        held = np.unique(gids)
        in_list = set(held.tolist())
        absent = [g for g in range(1, len(codes)) if g not in in_list and m.pattern_len(g) >= 3][:50]
        assert len(absent) == 50
        cut = np.searchsorted(pos, offs)
        rules = []
        for j in rng.permutation(len(offs) - 1)[:150].tolist():
            mine = np.unique(gids[cut[j]:cut[j + 1]])
            if len(mine) < 2:
                continue
            pick = rng.permutation(mine)[:int(rng.integers(2, 5))].tolist()
            k = len(rules) % 4
            if k == 1:
                pick[-1] = -pick[-1]  # killed in this stream; may fire elsewhere
            elif k == 2:
                pick.append(-int(absent[len(rules) % 50]))
            elif k == 3:
                pick.append(-int(rng.choice(held)))
            if abs(pick[-1]) in pick[:-1]:
                continue  # no gid twice in a rule
            rules.append([int(g) for g in pick])
        rules += [[int(absent[k]), int(held[k])] for k in range(10)] + [[int(absent[k])] for k in range(10, 15)]
        _real["in"] = (text, offs, exp, events, rules)
    return _real["in"]


def _behind(m, torch, scan, n, offs, events, rules, what):
    """scan(ev, d_offs) enqueues an all-matches list scan; the rules call
    follows with no synchronize between; the hits against the reference on the
    oracle's list."""
    nseg = len(offs) - 1
    exp_ptr, exp_hits = reference_rules(events, offs, rules)
    assert exp_ptr[-1] > 50 and len(set((exp_hits & np.uint64(0xFFFFFF)).tolist())) < len(rules)
    d_offs = _dev(torch, offs)
    ev = Ev(torch, len(events) + 100)
    o = Out(torch, m, ev.cap, nseg, len(exp_hits))
    scan(ev, d_offs)
    _call(m, torch, ev, d_offs, nseg, o)
    torch.cuda.synchronize()
    assert ev.total() == len(events), what
    ptr, hits = o.result()
    _assert_equal(ptr, hits, exp_ptr, exp_hits, what)


def test_behind_the_batched_and_the_flow_scan():
    torch = _torch()
    m = own_matcher()
    text, offs, exp, events, rules = _real_inputs()
    m.set_rules(rules)
    min_len = m.rules_min_len()
    assert min_len >= 3
    events = events if min_len == 3 else pack(*_gid_list(m, exp, min_len))
    d_text = _text_dev(torch, text)
    nseg, n = len(offs) - 1, len(text)

    def batch(ev, d_offs):
        m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, min_len, ev.buf.data_ptr(), ev.cap,
                                    ev.nev.data_ptr(), _stream(torch))

    def flow(ev, d_offs):
        m.scan_flows_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, None, None, min_len,
                                    ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
    _behind(m, torch, batch, n, offs, events, rules, "batch")
    assert m.kernel_last == pm.KIND_RT
    _behind(m, torch, flow, n, offs, events, rules, "flow")
    assert m.kernel_last == pm.KIND_AC


def _gid_list(m, exp, min_len):
    codes = np.asarray(m._codes, dtype=np.uint32)
    order = np.argsort(codes)
    pos, pcodes = expected_matches("et", exp, min_len)
    return pos, order[np.searchsorted(codes[order], pcodes)]


def test_read_many_rules_and_the_host_form():
    m = own_matcher()
    text, offs, exp, events, rules = _real_inputs()
    m.set_rules(rules)
    min_len = m.rules_min_len()
    pos, gids = _gid_list(m, exp, min_len)
    exp_ptr, exp_hits = reference_rules(pack(pos, gids), offs, rules)
    # first, while the staging is small: its hits array is grown where the hits outnumber it (a rule per gid,
    # five times over)
    few = pack(pos[:2000], gids[:2000])
    many = [[int(g)] for g in np.unique(gids[:2000])] * 5
    m.set_rules(many)
    p2, h2 = m.rules_by_stream(few, offs)
    e2 = pm.rules_by_stream_host(few, offs, many)
    assert np.array_equal(p2, e2[0]) and np.array_equal(h2, e2[1]) and len(h2) > 2000
    # the host form on the whole list
    m.set_rules(rules)
    ptr, hits = m.rules_by_stream(pack(pos, gids), offs)
    assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)
    assert m.scratch_bytes >= 8 * len(pos) + 8 * len(hits) + m.rules_scratch_bytes(len(pos), len(offs) - 1)
    m.set_rules(many)
    # hits_cap short on the host form: rule_ptr complete, the first hits_cap of the sorted ranges
    out, rp = np.full(10 + 8, POISON64, np.uint64), np.zeros(len(offs), np.int64)
    assert m.lib.pm_hip_rules_by_stream(m.obj, few.ctypes.data_as(u64p), len(few), offs.ctypes.data_as(i64p),
                                        len(offs) - 1, out.ctypes.data_as(u64p), 10, rp.ctypes.data_as(i64p)) == 0
    assert np.array_equal(rp, e2[0]) and np.array_equal(out[:10], e2[1][:10]) and np.all(out[10:] == POISON64)
    p0, h0 = m.rules_by_stream(np.empty(0, np.uint64), offs)
    assert not p0.any() and len(p0) == len(offs) and len(h0) == 0
    # read_many_rules on a dozen small buffers
    m.set_rules(rules)
    js = [int(j) for j in np.argsort(-np.diff(exp_ptr))[:10]] + [0, 1]
    buffers = [bytes(text[offs[j]:offs[j + 1]]) for j in js]
    got = m.read_many_rules(buffers)
    assert len(got) == len(buffers)
    fired = 0
    for j, (gpos, grule) in zip(js, got):
        hp, hr = pm.unpack_events(exp_hits[exp_ptr[j]:exp_ptr[j + 1]])
        assert gpos.tolist() == (hp - offs[j]).tolist() and grule.tolist() == hr.tolist(), j
        fired += len(hr)
    assert fired >= 10


# ---- 9. captured behind a scan, and between served read_block calls ---------------------
def test_captured_behind_a_scan_and_replayed():
    """scan_batch_matches_device and the rules call captured as one chain on a
    side stream and replayed three times, the reversed text copied over the text
    in place before the second: every replay answers for that replay's list;
    the scratch and rule_ptr are not reset between replays, so what one leaves
    behind (the counts, the table) would show in the next."""
    torch = _torch()
    text, offs, exp, events, rules = _real_inputs()
    other = np.ascontiguousarray(text[::-1])
    n, nseg = len(text), len(offs) - 1
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        # rules over the most frequent gids of both texts too (the oracle's), so that both fire some
        gid = np.concatenate([pm.unpack_events(events)[1], _gid_list(own_matcher(), oracle_per_stream("et", other, offs), 3)[1]])
        top = np.argsort(-np.bincount(gid.astype(np.int64)))[:12]
        rules = rules + random_rules(np.random.default_rng(27), 200, top, max_pos=3)
        m.set_rules(rules)
        min_len = m.rules_min_len()
        d_text, d_offs = _text_dev(torch, text), _dev(torch, offs)
        ev = Ev(torch, 4 * n)
        o = Out(torch, m, ev.cap, nseg, 4 * n)
        m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, min_len, ev.buf.data_ptr(), ev.cap,
                                    ev.nev.data_ptr(), _stream(torch))
        torch.cuda.synchronize()
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, min_len, ev.buf.data_ptr(),
                                        ev.cap, ev.nev.data_ptr(), st.cuda_stream)
            _call(m, torch, ev, d_offs, nseg, o, stream=st.cuda_stream)
        torch.cuda.synchronize()
        seen = []
        for replay in range(3):
            if replay == 1:
                d_text[:n].copy_(torch.from_numpy(other))
            ev.nev.zero_()
            o.hits[:o.hits_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            total = ev.total()
            assert 0 < total <= ev.cap
            lst = ev.slots()[:total]
            ptr, hits = o.result()
            exp_ptr, exp_hits = pm.rules_by_stream_host(lst, offs, rules)
            assert 0 < exp_ptr[-1] <= o.hits_cap, replay
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, f"replay {replay}")
            assert np.all(hits[ptr[-1]:] == POISON64)
            seen.append((ptr.copy(), exp_hits))
        assert not np.array_equal(seen[0][0], seen[1][0])  # another text, other hits
        assert np.array_equal(seen[1][0], seen[2][0]) and np.array_equal(seen[1][1], seen[2][1])
    finally:
        m.free()


def test_call_between_served_read_blocks():
    """Small read_block calls of an rt object go to its resident server grid;
    a rules call after every third asks the grid to leave the device first,
    like every device launch, and the next small call launches it again: the
    gids equal one large call's, every rules result the twin's."""
    m = fresh_matcher("snort", "rt")
    try:
        assert all(m.pattern_len(g) > 0 for g in range(1, 8))
        sizes = [100 << 10] * 9
        text = np.tile(SHIP, 1 + sum(sizes) // len(SHIP))[:sum(sizes)]
        cuts = np.cumsum([0] + sizes)
        m.reset()
        whole = m.read_block_gids(text)  # > 256 Ki positions: the pipeline, not the server
        m.reset()
        s0 = m.serve_stats()
        rng = np.random.default_rng(28)
        offs = np.concatenate([[3], 3 + np.cumsum(rng.integers(0, 30, size=300))]).astype(np.int64)
        rules = random_rules(rng, 50, np.arange(1, 7))
        m.set_rules(rules)
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(m.read_block_gids(text[a:b]))
            if k % 3 == 2:
                events = pack(rng.integers(0, offs[-1] + 10, size=3000), rng.integers(1, 6, size=3000))
                ptr, _ = _run(events, offs, rules, m=m, set_rules=False)
                assert ptr[-1] > 0
        assert np.array_equal(np.concatenate(parts), whole)
        s1 = m.serve_stats()
        assert s1["calls"] - s0["calls"] == len(sizes)
        assert s1["launches"] - s0["launches"] >= 3  # the first call, and the call after each stop
    finally:
        m.free()
