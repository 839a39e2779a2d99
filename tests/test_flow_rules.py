"""Flow rules on the device (pm_hip_set_flow_rules, pm_hip_flow_rules_device,
pm_hip_flow_rules; include/pm_hip.h "flow rules"; csrc/pm_flowrules.hip): the
rules whose conjunction becomes true in a call, over a set per flow carried on
the device.  Hand-made lists are compared with the host twin
(pm_flat_flow_rules), which test_flow_rules_cpu.py pins to the dict-and-set
reference, down to the set words; behind real scans the expected hits come
from the oracle's lists through that reference.  The device's ranges are
compared after sorting each.  The sets, the hits, rule_ptr and the scratch
carry poisoned guard slots past their end, which must stay untouched; the hits
array has exactly the expected number of slots unless a test says otherwise."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import first_difference, first_range_difference, mixed_offsets, pack, scan_like
from flow_rule_inputs import reference_flow_rules, rule_bits, sets_array, words_of
from fuzz_inputs import case as fuzz_case
from match_inputs import expected_matches
from nocase_inputs import brute, call_events, flag_of, fuzz_dictionary, fuzz_text, stream_offsets
from oracle_lib import dict_paths
from rule_inputs import csr, random_offsets, random_rules
from test_batch import _dev, _stream
from test_by_stream import PTR_POISON, SCRATCH_GUARD, _i64, _list_dev, _sorted_ranges
from test_events import GUARD, POISON64, Ev, _text_dev
from test_flows import STATE_POISON, _states
from test_gpu_parity import SHIP, _torch, fresh_matcher
from test_nocase import _u64, build, gids_of

pytestmark = pytest.mark.gpu

B = 1024  # the scan block's width (csrc/pm_bystream.h PM_BS_SCAN_BLOCK)
NG = 4200  # the hand-made lists use gids 1..NG, all of them patterns of et and of snort
KEEP = pm.FLOW_RULES_KEEP
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))

_own = {}


def own_matcher():
    """An auto object over et of this module's own: set_flow_rules changes the
    object, and the host forms grow its staging."""
    if "m" not in _own:
        m = pm.HipMatcher("auto")
        m.add_dictionary(pm.Dictionary(dict_paths("et")))
        m.compile()
        assert all(m.pattern_len(g) > 0 for g in range(1, NG + 1))
        _own["m"] = m
    return _own["m"]


class Sets:
    """nrows x W set words on the device in front of a guard."""

    def __init__(self, torch, sets):
        self.shape = sets.shape
        self.n = sets.size
        self.t = _i64(torch, self.n + GUARD, POISON64 - (1 << 64))
        if self.n:
            self.t[:self.n] = torch.from_numpy(np.ascontiguousarray(sets).ravel().view(np.int64).copy()).cuda()

    def get(self):
        a = self.t.cpu().numpy().view(np.uint64)
        assert np.all(a[self.n:] == POISON64), "sets guard"
        return a[:self.n].reshape(self.shape)


class Out:
    """The outputs and scratch of one device call, each in front of a guard;
    the scratch has the stated pm_hip_flow_rules_scratch_bytes."""

    def __init__(self, torch, m, cap, nseg, hits_cap):
        self.hits_cap, self.nseg = hits_cap, nseg
        self.hits = _i64(torch, hits_cap + GUARD, POISON64 - (1 << 64))
        self.ptr = _i64(torch, nseg + 1 + GUARD, PTR_POISON)
        self.bytes = m.lib.pm_hip_flow_rules_scratch_bytes(cap, nseg)
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


def _call(m, torch, ev, d_offs, nseg, d_sets, nrows, d_rows, flags, o, stream=None):
    m.flow_rules_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg, d_sets.t.data_ptr(), nrows,
                        None if d_rows is None else d_rows.data_ptr(), flags, o.hits.data_ptr(), o.hits_cap,
                        o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes, _stream(torch) if stream is None else stream)


def _assert_equal(ptr, hits, exp_ptr, exp_hits, what):
    diff = first_difference(ptr, exp_ptr)
    assert not diff, f"{what}: rule_ptr: {diff}"
    assert ptr[0] == 0 and ptr[-1] == exp_ptr[-1] == len(exp_hits), what
    diff = first_range_difference(ptr, _sorted_ranges(ptr, hits), exp_hits)
    assert not diff, f"{what}: {diff}"


class Flows:
    """The sets of some flows on the device (behind a guard) and their twin's
    on the host; call() runs one device call against the twin's."""

    def __init__(self, rules, nrows, fast=None, m=None, set_rules=True, init=None):
        self.torch = _torch()
        self.m = own_matcher() if m is None else m
        self.rules = rules
        if set_rules:
            self.m.set_flow_rules(rules, fast)
        W = words_of(rules)
        assert self.m.flow_rule_count() == len(rules) and self.m.flow_rule_words == W
        self.host = np.zeros((nrows, W), dtype=np.uint64) if init is None else init.copy()
        self.dev = Sets(self.torch, self.host)
        self.nrows = nrows

    def call(self, events, offs, rows=None, keep=False, cap=None, cursor=None, what=""):
        """The device call on a hand-made list against the twin on the events
        it has to use, with room for exactly the expected hits.  Returns
        (rule_ptr, expected hits)."""
        torch, m = self.torch, self.m
        events = np.ascontiguousarray(events, dtype=np.uint64)
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        nseg = len(offs) - 1
        cap = len(events) if cap is None else cap
        cursor = len(events) if cursor is None else cursor
        exp_ptr, exp_hits = pm.flow_rules_host(events[:min(cursor, cap)], offs, self.rules, self.host, rows, keep)
        ev = _list_dev(torch, events, cap, cursor)
        o = Out(torch, m, cap, nseg, len(exp_hits))
        d_rows = None if rows is None else _dev(torch, np.asarray(rows, dtype=np.int64))
        _call(m, torch, ev, _dev(torch, offs), nseg, self.dev, self.nrows, d_rows, KEEP if keep else 0, o)
        torch.cuda.synchronize()
        ptr, hits = o.result()
        ev.assert_guard(cap)
        assert ev.total() == cursor
        _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
        assert np.array_equal(self.dev.get(), self.host), f"{what}: the sets differ from the twin's"
        return ptr, exp_hits


def _rules_of(hits):
    return (np.asarray(hits, dtype=np.uint64) & np.uint64(0xFFFFFF)).tolist()


# ---- 1. two and three calls --------------------------------------------------------------------
def test_terms_in_three_calls():
    """Rule 0 has a term in each of three calls; rule 1 is completed in call 2
    by one carried and one new term; rule 2 has one term and fires at its
    first occurrence only; rule 3's terms all recur in call 2 after it fired
    in call 1."""
    rules = [[1, 2, 3], [4, 5], [6], [7, 8]]
    f = Flows(rules, 2)
    offs = [10, 50, 90]
    _, h1 = f.call(pack([12, 13, 20, 30, 31, 60], [1, 4, 6, 7, 8, 6]), offs, what="call 1")
    assert h1.tolist() == [(20 << 24) | 2, (31 << 24) | 3, (60 << 24) | 2]
    _, h2 = f.call(pack([11, 15, 16, 17, 18, 19, 70], [6, 2, 5, 7, 8, 4, 6]), offs, what="call 2")
    assert h2.tolist() == [(16 << 24) | 1]
    _, h3 = f.call(pack([14, 15, 40], [6, 3, 3]), offs, what="call 3")
    assert h3.tolist() == [(15 << 24) | 0]
    _, h4 = f.call(pack([14, 15, 40, 41, 42], [1, 2, 3, 4, 5]), offs, what="call 4")
    assert h4.tolist() == []  # everything is carried in flow 0
    bit = rule_bits(rules)
    assert f.host[0, 0] == sum(1 << bit[g] for g in range(1, 9)) and f.host[1, 0] == sum(1 << bit[g] for g in (6,))


def test_negation_carried_later_in_the_call_and_in_the_next_call():
    rules = [[1, 2, -3], [4, -5], [6, 7, -8]]
    f = Flows(rules, 3)
    offs = [0, 100, 200, 300]
    # flow 0: 3 is carried into the call that completes [1, 2, -3]; flow 1: 5 appears behind the completing 4 in
    # the same call; flow 2: [6, 7, -8] hits in call 2 and 8 appears in call 3
    _, h1 = f.call(pack([5, 6, 210], [1, 3, 6]), offs, what="call 1")
    assert h1.tolist() == []
    _, h2 = f.call(pack([7, 110, 150, 220], [2, 4, 5, 7]), offs, what="call 2")
    assert h2.tolist() == [(220 << 24) | 2]
    _, h3 = f.call(pack([9, 120, 230, 231], [1, 4, 8, 6]), offs, what="call 3")
    assert h3.tolist() == []


@pytest.mark.parametrize("order", ["small gid first", "large gid first"])
def test_terms_at_equal_first_positions_give_one_hit_at_the_larger_gids_slot(order):
    """A pattern and its proper suffix first end at the same byte: terms 40
    and 41 at position 77, the rule written in either order, in a list in
    either order.  Exactly one hit, at 77."""
    rules = [[40, 41], [41, 40, 42]] if order == "small gid first" else [[41, 40], [42, 40, 41]]
    f = Flows(rules, 1)
    ev = pack([77, 77, 77, 80], [40, 41, 42, 40])
    _, h = f.call(ev if order == "small gid first" else ev[::-1], [0, 100], what=order)
    assert h.tolist() == [(77 << 24) | 0, (77 << 24) | 1]


# ---- 2. the per-lane turns ------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 200, 1000])
def test_one_slot_indexing_n_rules(n):
    """gid 7 is a positive term of n rules [7, g] / [7, -g]: one table slot per
    stream holds it, and its wave verifies them a rule per lane in turns of
    64.  Flow 0 gets the other terms in call 1 and 7 in call 2 (every rule is
    verified against carried terms), flow 1 gets 7 first, flow 2 all at once."""
    rules = [[7, 100 + k] if k % 3 else [7, -(100 + k)] for k in range(n)]
    rng = np.random.default_rng(n)
    offs = [5, 400, 400, 900, 1400]
    f = Flows(rules, 4)
    others = lambda lo, hi, size: pack(rng.integers(lo, hi, size=size), rng.integers(100, 100 + n + 5, size=size))  # noqa: E731
    p1, _ = f.call(np.concatenate([others(5, 400, 300), pack([450, 460], [7, 7]), others(900, 1400, 200),
                                   pack([1000], [7])]), offs, what=f"{n} rules, call 1")
    p2, _ = f.call(np.concatenate([pack([300, 10], [7, 7]), others(400, 900, 300)]), offs, what=f"{n} rules, call 2")
    assert p1[-1] > 0 and (n == 1 or (p2[1] > 0 and p2[-1] > p2[1]))


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


def test_a_wave_in_which_every_slot_indexes_and_one_in_which_only_lane_63_does():
    """cap 1,024, so a table of 2,048 slots.  64 keys whose home slots are the
    64 slots of wave 3 and are distinct (nothing probes), every gid among them
    a term of two rules; one key at slot 64 * 9 + 63, the completing term of a
    rule whose other term's key lies in another wave, at a smaller position."""
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
    events = pack([offs[j] + (g % 10) for j, g in full] + [offs[last[0]] + 5, offs[other[0]] + 1], [g for _, g in keys])
    assert len({_home(j, g, table) for j, g in keys}) == len(keys)  # every key sits at home
    rules = []
    for g in sorted({g for _, g in full}):
        rules += [[g], [g, -4000]]
    rules.append([last[1], other[1]])
    f = Flows(rules, nseg)
    ptr, hits = f.call(events, offs, cap=1024)
    assert ptr[-1] == 2 * 64 + 1
    assert ((int(offs[last[0]]) + 5) << 24) | (len(rules) - 1) in hits[ptr[last[0]]:ptr[last[0] + 1]].tolist()
    assert pm.load().pm_hip_flow_rules_scratch_bytes(1024, nseg) >= 16 * table


def test_terms_in_a_long_probe_run():
    """4,096 distinct new terms of one flow in a list of cap 4,096: the
    table's 8,192 slots are exactly half full, so the probe runs are as long
    as they get, and every one of the 4,096 commits lands in one row of 64
    words.  Then the same list again: nothing is new."""
    n = 4096
    assert pm.load().pm_hip_flow_rules_scratch_bytes(n, 1) == 16 * 2 * n + 16 + 16
    rng = np.random.default_rng(21)
    events = pack(100 + rng.integers(0, 50000, size=n), rng.permutation(np.arange(1, n + 1)))
    rules = random_rules(rng, 500, np.arange(1, n + 1), max_pos=6, negated=0.0)
    rules += [r + [-(1 + (r[0] + 7 * k) % n)] for k, r in enumerate(rules[:50]) if 1 + (r[0] + 7 * k) % n not in r]
    named = {abs(t) for r in rules for t in r}
    rules += [[g] for g in range(1, n + 1) if g not in named]  # every gid a term: K = n
    f = Flows(rules, 1)
    assert f.m.flow_rule_words == 64
    ptr, hits = f.call(events, [100, 60000], cap=n)
    assert ptr[-1] >= 500 and np.all(f.host == np.uint64((1 << 64) - 1))
    ptr, hits = f.call(events, [100, 60000], cap=n)
    assert ptr[-1] == 0


# ---- 3. the word edges -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [64, 128, 129])
def test_word_edges(k):
    """K = 64, 128 and 129 term gids (W = 1, 2 and 3): rules over the bits 62
    to 65 and 126 to 128 with their terms in different calls, two streams'
    commits landing in adjacent rows, garbage above K surviving."""
    gids = [10 * (b + 1) for b in range(k)]
    rules = [[gids[b], gids[b + 1]] for b in range(k - 1)] + [[gids[-1], -gids[0]], [gids[-1]]]
    W = (k + 63) // 64
    garbage = np.zeros(W, dtype=np.uint64)
    for b in range(k, 64 * W):
        garbage[b >> 6] |= np.uint64(1 << (b & 63))
    nrows = 4
    f = Flows(rules, nrows, init=np.tile(garbage, (nrows, 1)))
    assert f.m.flow_rule_words == W and f.m.flow_rule_bit(gids[-1]) == k - 1 and f.m.flow_rule_bit(11) == -1
    rng = np.random.default_rng(k)
    offs = np.array([100, 200, 300, 400, 500], dtype=np.int64)
    fired = set()
    for call in range(3):
        edge = [g for b, g in enumerate(gids) if (b & 63) in ((62, 63) if call == 0 else (0, 1) if call == 1 else (2,))]
        events = np.concatenate([pack(rng.integers(100, 300, size=2 * k), rng.choice(gids, size=2 * k)),
                                 pack(350 + np.arange(len(edge)), edge), pack(450 + np.arange(len(edge)), edge[::-1])])
        ptr, hits = f.call(events, offs, what=f"K {k}, call {call}")
        fired |= set(_rules_of(hits))
        assert np.all(f.host & garbage == garbage)
    assert 62 in fired and (k == 64 or {63, 126} <= fired) and (k < 129 or 127 in fired)


def test_many_new_terms_of_one_stream_land_in_one_word():
    """64 terms new at once in each of 33 flows: 64 atomic ORs into one word,
    the flows' rows adjacent."""
    rules = [[g] for g in range(1, 65)] + [[1, 64], [64, 1, -2]]
    nseg = 33
    offs = np.arange(nseg + 1, dtype=np.int64) * 100
    rng = np.random.default_rng(5)
    pos = np.concatenate([offs[j] + rng.permutation(100)[:64] for j in range(nseg)])
    f = Flows(rules, nseg)
    ptr, hits = f.call(pack(pos, np.tile(np.arange(1, 65), nseg)), offs)
    assert ptr[-1] == nseg * 65 and np.all(f.host == np.uint64((1 << 64) - 1))


# ---- 4. rows ---------------------------------------------------------------------------------------
def test_rows_identity_permutation_out_of_range_and_spare_rows():
    rng = np.random.default_rng(31)
    rules = random_rules(rng, 200, np.arange(1, 20), max_pos=3)
    nseg, nrows = 40, 50
    f = Flows(rules, nrows)
    total = 0
    for call in range(4):
        offs = random_offsets(rng, nseg, max_len=30)
        events = pack(rng.integers(max(int(offs[0]) - 5, 0), offs[-1] + 5, size=400), rng.integers(1, 21, size=400))
        if call == 0:
            rows = None  # identity: rows 0..39
        else:
            rows = rng.permutation(nrows)[:nseg].astype(np.int64)
            rows[rng.permutation(nseg)[:6]] = [-1, -7, nrows, nrows + 3, 1 << 40, -(1 << 62)]  # inert streams
        before = f.host.copy()
        ptr, _ = f.call(events, offs, rows=rows, what=f"call {call}")
        total += int(ptr[-1])
        named = set(range(nseg)) if rows is None else {int(r) for r in rows if 0 <= r < nrows}
        spare = sorted(set(range(nrows)) - named)
        assert spare and np.array_equal(f.host[spare], before[spare])
        if rows is not None:
            inert = np.nonzero((rows < 0) | (rows >= nrows))[0]
            assert len(inert) == 6 and not np.diff(ptr)[inert].any()
    assert total > 100


# ---- 5. size and cursor edges ------------------------------------------------------------------------
def test_more_slots_than_one_grid():
    """600,000 events: a table of 2^21 slots, more than one grid of lanes, so
    the grid-stride loops of the evaluations and the commit turn again; two
    calls; rules fire in the first and in the last stream."""
    torch = _torch()
    lanes = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 600000
    assert pm.load().pm_hip_flow_rules_scratch_bytes(n, 1) >= 16 * (1 << 21) and lanes < (1 << 21)
    rng = np.random.default_rng(22)
    offs = mixed_offsets(rng)
    full = np.nonzero(np.diff(offs) > 0)[0]
    first, last = int(full[0]), int(full[-1])
    rules = random_rules(rng, 200, np.arange(1, 11)) + [[20, 21], [21, 20, -1], [21, 20, -22]]
    f = Flows(rules, len(offs) - 1)
    events = np.concatenate([scan_like(n - 2, offs, np.arange(1, 9), rng), pack([offs[first], offs[last + 1] - 1], [20, 20])])
    f.call(events, offs, what="call 1")
    events = np.concatenate([scan_like(n - 2, offs, np.arange(1, 11), rng), pack([offs[first], offs[last + 1] - 1], [21, 21])])
    ptr, hits = f.call(events, offs, what="call 2")
    assert 200 in _rules_of(hits[ptr[first]:ptr[first + 1]]) and 200 in _rules_of(hits[ptr[last]:ptr[last + 1]])


@pytest.mark.parametrize("nseg", [1, B - 1, B, B + 1, 3000])
def test_scan_sizes(nseg):
    rng = np.random.default_rng(nseg)
    rules = [[1], [1, 2], [2, -3], [3, 4, 5], [5, -1]]
    f = Flows(rules, nseg + 2)
    for call in range(2):
        offs = random_offsets(rng, nseg, max_len=3, base=17)
        if offs[-1] == offs[0]:
            offs[-1] += 2
        pos = np.concatenate([[offs[0], offs[-1] - 1, offs[-1] - 1], rng.integers(offs[0] - 2, offs[-1] + 2, size=2000)])
        events = pack(pos, np.concatenate([[1, 1, 2], rng.integers(1, 6, size=2000)]))
        ptr, _ = f.call(events, offs, what=f"nseg {nseg}, call {call}")
        assert ptr[-1] > 0 or call == 1


def test_cursor_above_cap_and_below_the_list():
    rng = np.random.default_rng(23)
    events = pack(rng.integers(0, 500, size=1500), rng.integers(1, 9, size=1500))
    rules = random_rules(rng, 60, np.arange(1, 10))
    f = Flows(rules, 3)
    few = pack(rng.integers(0, 500, size=300), rng.integers(1, 5, size=300))  # gids 1..4: the next call has new ones
    a, _ = f.call(few, [0, 100, 250, 500], cap=300, cursor=300 + 100000)
    # the slots past the cursor hold poison: as events they lie inside the last stream here
    b, _ = f.call(events, [0, 100, 250, 1 << 40], cap=2000, cursor=700)
    assert a[-1] > 0 and b[-1] > 0
    before = f.host.copy()
    c, _ = f.call(np.empty(0, np.uint64), [0, 100, 250, 1 << 40], cap=2000, cursor=0)
    assert c.tolist() == [0, 0, 0, 0] and np.array_equal(f.host, before)


@pytest.mark.parametrize("short", ["one", "all"])
def test_hits_cap_short_keeps_rule_ptr_exact_and_commits(short):
    torch = _torch()
    m = own_matcher()
    rng = np.random.default_rng(24)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 40, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    rules = random_rules(rng, 600, np.arange(1, 42))
    m.set_flow_rules(rules)
    host = np.zeros((nseg, 1), dtype=np.uint64)
    exp_ptr, exp_hits = pm.flow_rules_host(events, offs, rules, host)
    total = int(exp_ptr[-1])
    assert total > 500 and host.any()
    hits_cap = total - 1 if short == "one" else 0
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, hits_cap)
    d_sets = Sets(torch, np.zeros_like(host))
    _call(m, torch, ev, _dev(torch, offs), nseg, d_sets, nseg, None, 0, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()  # (the guard behind hits_cap is checked there)
    assert np.array_equal(ptr, exp_ptr) and np.array_equal(d_sets.get(), host)
    # every stored slot holds a hit of its stream's expected range, none more often than expected
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = set(zip(seg.tolist(), exp_hits.tolist()))
    got = list(zip(seg[:hits_cap].tolist(), hits.tolist()))
    assert len(set(got)) == len(got) == hits_cap and set(got) <= want


def test_keep_then_the_committing_call_then_nothing():
    rng = np.random.default_rng(25)
    rules = random_rules(rng, 300, np.arange(1, 30))
    f = Flows(rules, 10)
    offs = np.arange(0, 301, 30)
    for call in range(2):
        events = pack(rng.integers(0, 300, size=150), rng.integers(1, 30, size=150))
        before = f.host.copy()
        kp, kh = f.call(events, offs, keep=True, what="keep")
        assert np.array_equal(f.host, before)
        cp, ch = f.call(events, offs, what="commit")
        assert np.array_equal(kp, cp) and np.array_equal(kh, ch) and cp[-1] > 0
        ap, _ = f.call(events, offs, what="again")
        assert ap[-1] == 0


# ---- 6. return codes -------------------------------------------------------------------------------------
def _good_args(torch, m, nseg=2, nrows=2):
    events = pack([1, 2, 3, 3], [1, 1, 2, 2])
    offs = np.array([0, 2, 4], dtype=np.int64)
    ev = _list_dev(torch, events, 4, 4)
    o = Out(torch, m, 4, nseg, 4)
    d_sets = Sets(torch, np.zeros((nrows, max(m.flow_rule_words, 1)), dtype=np.uint64))
    d_offs, d_rows = _dev(torch, offs), _dev(torch, np.array([1, 0], dtype=np.int64))
    good = dict(e=ev.buf.data_ptr(), cap=4, c=ev.nev.data_ptr(), o=d_offs.data_ptr(), nseg=nseg, sets=d_sets.t.data_ptr(),
                nrows=nrows, rows=d_rows.data_ptr(), flags=0, h=o.hits.data_ptr(), hits_cap=4, p=o.ptr.data_ptr(),
                s=o.scratch.data_ptr(), sb=o.bytes, st=_stream(torch))
    return good, (ev, o, d_sets, d_offs, d_rows), events, offs


ORDER = ("e", "cap", "c", "o", "nseg", "sets", "nrows", "rows", "flags", "h", "hits_cap", "p", "s", "sb", "st")


def test_before_set_flow_rules_is_minus_11_and_nothing_is_touched():
    torch = _torch()
    m = fresh_matcher("et", "rt")
    try:
        for with_rules in (False, True):
            if with_rules:
                m.set_rules([[1, 2], [2]])  # the other rule set changes nothing here
            assert m.flow_rule_count() == 0 and m.flow_rules_min_len() == 0 and m.flow_rule_words == 0
            assert m.flow_rule_bit(1) == -1
            good, keep_alive, events, offs = _good_args(torch, m)
            _, o, d_sets, _, _ = keep_alive
            args = [good[k] for k in ORDER]
            assert m.lib.pm_hip_flow_rules_device(m.obj, *args) == -11
            assert b"pm_hip_set_flow_rules" in m.lib.pm_hip_last_error()
            hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
            sets = np.full((2, 1), 0x77, np.uint64)
            host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, sets.ctypes.data_as(u64p), 2, None, 0,
                    hits.ctypes.data_as(u64p), 4, ptr.ctypes.data_as(i64p)]
            assert m.lib.pm_hip_flow_rules(m.obj, *host) == -11
            torch.cuda.synchronize()
            assert o.untouched() and not d_sets.get().any()
            assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON) and np.all(sets == 0x77)
            # bad arguments come first, as the return codes are ordered
            args[4] = -1
            assert m.lib.pm_hip_flow_rules_device(m.obj, *args) == -2
    finally:
        m.free()
    raw = pm.HipMatcher("rt")
    raw.add_pattern(b"abc")
    tptr, terms = csr([[1]])
    assert raw.lib.pm_hip_set_flow_rules(raw.obj, tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), 1) == -1
    assert raw.lib.pm_hip_flow_rules_device(raw.obj, *args) == -1
    raw.free()


def test_bad_arguments_are_minus_2_and_nothing_is_touched():
    torch = _torch()
    m = own_matcher()
    lib = m.lib
    m.set_flow_rules([[1, 2], [2]])
    good, keep_alive, events, offs = _good_args(torch, m)
    _, o, d_sets, _, _ = keep_alive
    bad = [dict(e=None), dict(c=None), dict(o=None), dict(h=None), dict(p=None), dict(s=None), dict(sets=None),
           dict(e=good["e"] + 4), dict(c=good["c"] + 4), dict(o=good["o"] + 4), dict(h=good["h"] + 4),
           dict(p=good["p"] + 4), dict(s=good["s"] + 8), dict(sets=good["sets"] + 4), dict(rows=good["rows"] + 4),
           dict(nseg=-1), dict(nseg=1 << 31), dict(cap=(1 << 40) + 1), dict(h=good["e"]), dict(sb=o.bytes - 1), dict(sb=0),
           dict(nrows=-1), dict(nrows=(1 << 40) + 1), dict(rows=None, nrows=1), dict(flags=2), dict(flags=KEEP | 4),
           dict(flags=1 << 31)]
    for b in bad:
        assert lib.pm_hip_flow_rules_device(m.obj, *[{**good, **b}[k] for k in ORDER]) == -2, b
        assert b"bad arguments" in lib.pm_hip_last_error(), b
    torch.cuda.synchronize()
    assert o.untouched() and not d_sets.get().any()
    # nseg == 0: nothing launched or written, whatever the other pointers are
    assert lib.pm_hip_flow_rules_device(m.obj, *[{**good, "nseg": 0, "o": None, "s": None, "sb": 0, "rows": None}[k]
                                                 for k in ORDER]) == 0
    torch.cuda.synchronize()
    assert o.untouched() and not d_sets.get().any()
    # cap == 0 with streams: an all-zero rule_ptr, untouched sets, nothing else
    assert lib.pm_hip_flow_rules_device(m.obj, *[{**good, "cap": 0, "e": None}[k] for k in ORDER]) == 0
    torch.cuda.synchronize()
    ptr, hits = o.result()
    assert ptr.tolist() == [0, 0, 0] and np.all(hits == POISON64) and not d_sets.get().any()
    # the host form's -2 cases
    hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
    sets, rows = np.full((2, 1), 0x77, np.uint64), np.array([1, 0], np.int64)
    host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, sets.ctypes.data_as(u64p), 2,
            rows.ctypes.data_as(i64p), 0, hits.ctypes.data_as(u64p), 4, ptr.ctypes.data_as(i64p)]
    for k, v in ((0, None), (2, None), (10, None), (8, None), (4, None), (3, 1 << 31), (1, (1 << 40) + 1),
                 (8, events.ctypes.data_as(u64p)), (7, 2), (5, (1 << 40) + 1)):
        a = list(host)
        a[k] = v
        assert lib.pm_hip_flow_rules(m.obj, *a) == -2, k
        assert b"bad arguments" in lib.pm_hip_last_error(), k
    a = list(host)
    a[5], a[6] = 1, None  # no rows and fewer rows than streams
    assert lib.pm_hip_flow_rules(m.obj, *a) == -2
    assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON) and np.all(sets == 0x77)
    assert lib.pm_hip_flow_rules_scratch_bytes(1, -1) == ctypes.c_size_t(-1).value


def test_every_bad_rule_set_is_minus_2_and_the_rules_stay():
    from test_rules_cpu import bad_rule_sets
    m = own_matcher()
    lib = m.lib
    rules = [[1, 2], [2, -3]]
    f = Flows(rules, 3)
    before = m.table_bytes
    npat = next(g for g in range(NG, 1 << 24) if m.pattern_len(g) == 0) - 1
    cases = bad_rule_sets() + [("a gid above the last pattern", *csr([[1, npat + 1]]), None),
                               ("gid 0", *csr([[1, 0]]), None), ("the largest gid", *csr([[1, (1 << 24) - 1]]), None)]
    for name, tptr, terms, nrules in cases:
        n = (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules
        rc = lib.pm_hip_set_flow_rules(m.obj, None if tptr is None else tptr.ctypes.data_as(u32p),
                                       None if terms is None else terms.ctypes.data_as(u32p), n)
        assert rc == -2, name
        msg = lib.pm_hip_last_error()
        for word in (b"2^24", b"64", b"positive", b"twice", b"PM_RULE_FAST", b"negated", b"pattern"):
            assert word in msg, (name, word)
        assert m.flow_rule_count() == 2 and m.table_bytes == before, name
    ptr, hits = f.call(pack([1, 2, 5, 6, 7], [1, 2, 2, 3, 2]), [0, 4, 6, 9])
    assert hits.tolist() == [(2 << 24) | 0, (2 << 24) | 1, (5 << 24) | 1]  # the last stream holds 3


def test_set_flow_rules_again_replaces_the_tables_and_set_rules_is_independent():
    m = own_matcher()
    rng = np.random.default_rng(26)
    events = pack(rng.integers(0, 300, size=2000), rng.integers(1, 30, size=2000))
    offs = np.arange(0, 301, 30)
    first = random_rules(rng, 300, np.arange(1, 31))
    second = random_rules(rng, 40, np.arange(1, 31), max_pos=2)
    m.set_rules([[1, 2]])
    a, ha = Flows(first, 10).call(events, offs)
    base = m.table_bytes
    assert m.flow_rules_min_len() == min(m.pattern_len(abs(g)) for r in first for g in r)
    assert m.rule_count() == 1  # pm_hip_set_rules' set is its own
    b, hb = Flows(second, 10).call(events, offs)
    assert m.flow_rule_count() == 40 and m.table_bytes < base  # the first tables were freed and are no longer counted
    assert not np.array_equal(a, b)
    m.set_rules([[3, 4], [5], [6, 7, 8]])  # larger tables of the other kind
    c, hc = Flows(first, 10).call(events, offs)
    assert np.array_equal(a, c) and np.array_equal(ha, hc) and m.table_bytes > base
    m.set_rules([[1, 2]])
    assert m.table_bytes == base and m.rule_count() == 1 and m.flow_rule_count() == 300


# ---- 7. fuzz ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(seed):
    rng = np.random.default_rng(200 + seed)
    nseg = int(rng.integers(1, 1000))
    ngid = int(rng.integers(2, 30)) if seed % 2 else int(rng.integers(70, 200))
    rules = random_rules(rng, int(rng.integers(1, 200)), np.arange(1, ngid + 4))
    fast = [None if rng.random() < 0.5 else int(rng.choice([g for g in r if g > 0])) for r in rules]
    nrows = nseg + 5
    f = Flows(rules, nrows, fast=fast)
    carried = {}
    for call in range(3):
        offs = random_offsets(rng, nseg)
        n = int(rng.integers(1, 8000))
        events = pack(rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n), rng.integers(1, ngid + 1, size=n))
        rows = None if call == 0 else rng.permutation(nrows)[:nseg].astype(np.int64)
        ptr, hits = f.call(events, offs, rows=rows, cap=n + int(rng.integers(0, 3)) * 100, what=f"seed {seed}, call {call}")
        exp_ptr, exp_hits = reference_flow_rules(events, offs, rules, carried, nrows, rows)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)
    assert np.array_equal(f.host, sets_array(carried, rules, nrows))


# ---- 8. behind real scans ----------------------------------------------------------------------------------
def _rules_from_lists(rng, ev_a, ev_b, offs, plen, want_straddler=True):
    """Rules over the gids of two calls' lists: per picked stream a term from
    call 1 with a term from call 2 (and both orders of negation), and, where
    there is one, a rule that pairs a pattern ending in A with a straddler: an
    event of call 2 whose pattern is longer than the bytes the stream has had
    in call 2.  Returns (rules, the index of the first straddler rule, its
    stream)."""
    nseg = len(offs) - 1
    pa, ga = pm.unpack_events(ev_a)
    pb, gb = pm.unpack_events(ev_b)
    ja, jb = np.searchsorted(offs, pa, side="right") - 1, np.searchsorted(offs, pb, side="right") - 1
    rules, straddle = [], None
    for j in rng.permutation(nseg).tolist():
        a = np.unique(ga[ja == j])
        b_all = gb[jb == j]
        b = np.setdiff1d(np.unique(b_all), a)
        if len(a) == 0 or len(b) == 0:
            continue
        if straddle is None and want_straddler:
            inside = jb == j
            begins_before = plen[gb[inside]] > pb[inside] - offs[j] + 1
            cross = np.setdiff1d(np.unique(gb[inside][begins_before]), a)
            if len(cross):
                straddle = (len(rules), j)
                rules.append([int(a[0]), int(cross[0])])
        if len(rules) < 120:
            x, y = int(rng.choice(a)), int(rng.choice(b))
            rules += [[x, y], [y, -x], [x, -y]][:1 + len(rules) % 3]
            if len(a) > 1:
                rules.append([int(g) for g in a[:2]] + [y])
    return rules, straddle


def _two_calls_behind(m, torch, scans, offs, ev_a, ev_b, rules, straddle, what):
    """scans[c](ev) enqueues call c's list scan; the flow-rules call follows
    with no synchronize between, twice, then one synchronize: the hits against
    the reference over the oracle's lists."""
    nseg = len(offs) - 1
    carried = {}
    exp = [reference_flow_rules(e, offs, rules, carried, nseg) for e in (ev_a, ev_b)]
    assert exp[0][0][-1] > 0 and exp[1][0][-1] > 0
    if straddle is not None:
        r, j = straddle
        assert r in _rules_of(exp[1][1][exp[1][0][j]:exp[1][0][j + 1]]), "the straddler rule fires in call 2"
    d_offs = _dev(torch, offs)
    d_sets = Sets(torch, np.zeros((nseg, m.flow_rule_words), dtype=np.uint64))
    evs = [Ev(torch, len(e) + 100) for e in (ev_a, ev_b)]
    outs = [Out(torch, m, ev.cap, nseg, len(x[1])) for ev, x in zip(evs, exp)]
    for c in range(2):
        scans[c](evs[c], d_offs)
        _call(m, torch, evs[c], d_offs, nseg, d_sets, nseg, None, 0, outs[c])
    torch.cuda.synchronize()
    for c, e in enumerate((ev_a, ev_b)):
        assert evs[c].total() == len(e), f"{what}, call {c + 1}"
        ptr, hits = outs[c].result()
        _assert_equal(ptr, hits, exp[c][0], exp[c][1], f"{what}, call {c + 1}")
    assert np.array_equal(d_sets.get(), sets_array(carried, rules, nseg)), what


@pytest.mark.parametrize("name", ["unary", "many", "no_short", "seed0", "seed5"])
def test_behind_the_flow_scan_in_two_calls(name):
    torch = _torch()
    c = fuzz_case(name)
    offs, nseg, n = c.offs, c.nseg, len(c.A)
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        codes = np.asarray(m._codes, dtype=np.uint32)
        assert len(np.unique(codes[1:])) == len(codes) - 1  # a code names one gid
        order = np.argsort(codes)
        plen = np.array([m.pattern_len(g) for g in range(len(codes))], dtype=np.int64)

        def lists(min_len):
            out = []
            for exp in (c.ea, c.eb):
                pos, pcodes = expected_matches(name, exp, min_len)
                out.append(pack(pos, order[np.searchsorted(codes[order], pcodes)]))
            return out
        ev_a, ev_b = lists(1)
        rules, straddle = _rules_from_lists(np.random.default_rng(len(name)), ev_a, ev_b, offs, plen)
        assert straddle is not None and len(rules) > 20
        m.set_flow_rules(rules)
        min_len = m.flow_rules_min_len()
        assert min_len == min(plen[abs(t)] for r in rules for t in r)
        ev_a, ev_b = lists(min_len)
        d_a, d_b = _text_dev(torch, c.A), _text_dev(torch, c.B)
        st = _states(torch, np.full(nseg, STATE_POISON, np.uint32))

        def scan_a(ev, d_offs):
            m.scan_flows_matches_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, n, None, st.data_ptr(), min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))

        def scan_b(ev, d_offs):
            m.scan_flows_matches_device(d_b.data_ptr(), d_offs.data_ptr(), nseg, n, st.data_ptr(), None, min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
        _two_calls_behind(m, torch, (scan_a, scan_b), offs, ev_a, ev_b, rules, straddle, name)
    finally:
        m.free()


def test_behind_the_nocase_flow_scan():
    """The call does not care which scan made the list: the nocase flow scan
    over A, then over B continuing A, the expected lists the brute force's."""
    torch = _torch()
    pats = fuzz_dictionary(0)
    flags_nc = [flag_of(p) for p in pats]
    m = build(pats, "auto", flags_nc)
    try:
        gid = gids_of(m, len(pats))
        A, B = fuzz_text(pats, 0, 49152), fuzz_text(pats, 50, 49152)
        offs = stream_offsets(len(A), 0)
        nseg, n, lens = len(offs) - 1, len(A), np.diff(offs)
        whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
        plen = np.array([m.pattern_len(g) for g in range(len(pats) + 1)], dtype=np.int64)

        def lists(min_len):
            rows, _ = brute(pats, flags_nc, whole, gid, min_len)
            return call_events(rows, offs, np.zeros(nseg, np.int64))[0], call_events(rows, offs, lens)[0]
        ev_a, ev_b = lists(1)
        rules, _ = _rules_from_lists(np.random.default_rng(9), ev_a, ev_b, offs, plen, want_straddler=False)
        m.set_flow_rules(rules)
        min_len = m.flow_rules_min_len()
        ev_a, ev_b = lists(min_len)
        W = m.case_words
        d_a, d_b = _text_dev(torch, A), _text_dev(torch, B)
        st = _states(torch, np.full(nseg, STATE_POISON, np.uint32))
        pos = _u64(torch, np.zeros(nseg, np.uint64))
        hist = _u64(torch, np.zeros(max(nseg * W, 1), np.uint64))
        st2, pos2, hist2 = (_states(torch, np.zeros(nseg, np.uint32)), _u64(torch, np.zeros(nseg, np.uint64)),
                            _u64(torch, np.zeros(max(nseg * W, 1), np.uint64)))

        def scan_a(ev, d_offs):
            m.scan_flows_nocase_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, n, None, st.data_ptr(), None, min_len, True,
                                       ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch), None, pos.data_ptr(),
                                       None, hist.data_ptr())

        def scan_b(ev, d_offs):
            m.scan_flows_nocase_device(d_b.data_ptr(), d_offs.data_ptr(), nseg, n, st.data_ptr(), st2.data_ptr(), None,
                                       min_len, True, ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch),
                                       pos.data_ptr(), pos2.data_ptr(), hist.data_ptr() if W else None, hist2.data_ptr())
        _two_calls_behind(m, torch, (scan_a, scan_b), offs, ev_a, ev_b, rules, None, "nocase")
    finally:
        m.free()


# ---- 9. the Python surface ---------------------------------------------------------------------------------
PATS = [b"alpha", b"beta", b"gamma", b"ta", b"delta", b"mma"]


def _brute_packets(pats_by_gid, whole, before):
    """The (position inside the packet, gid) events of the last len(whole) -
    before bytes of a flow: every occurrence that ends there."""
    out = []
    for g, p in pats_by_gid.items():
        at = whole.find(p)
        while at >= 0:
            end = at + len(p) - 1
            if end >= before:
                out.append((end - before, g))
            at = whole.find(p, at + 1)
    return out


def test_flow_table_scan_rules_over_three_rounds():
    m = build(PATS, "auto")
    try:
        gid = gids_of(m, len(PATS))
        g = {p: int(gid[k]) for k, p in enumerate(PATS)}
        by_gid = {v: k for k, v in g.items()}
        rules = [[g[b"alpha"], g[b"beta"]], [g[b"gamma"], -g[b"delta"]], [g[b"ta"]], [g[b"mma"], g[b"gamma"], g[b"alpha"]],
                 [g[b"beta"], g[b"delta"], -g[b"alpha"]]]
        m.set_flow_rules(rules)
        assert m.flow_rules_min_len() == 2
        flows = pm.FlowTable(m)
        rounds = [
            [("a", b"..alp"), ("b", b"beta gam"), ("c", b"delta")],
            [("a", b"ha be"), ("c", b" gamma beta"), ("d", b"gamma delta")],  # b pauses; alpha straddles in a
            [("b", b"ma alpha"), ("a", b"ta gamma"), ("c", b"alpha"), ("d", b"")],
        ]
        text, carried, fired = {}, {}, 0
        key_row = {}

        def check(packets):
            nonlocal fired
            got = flows.scan_rules(packets)
            assert len(got) == len(packets)
            for (k, data), (pos, rule) in zip(packets, got):
                before = len(text.get(k, b""))
                text[k] = text.get(k, b"") + data
                ev = _brute_packets(by_gid, text[k], before)
                row = key_row.setdefault(k, len(key_row))
                _, hits = reference_flow_rules(pack([p for p, _ in ev], [q for _, q in ev]), [0, len(data)], rules, carried,
                                               row + 1, rows=[row])
                hp, hr = pm.unpack_events(hits)
                assert pos.tolist() == hp.tolist() and rule.tolist() == hr.tolist(), (k, data)
                assert flows.bytes[k] == flows.rule_bytes[k] == len(text[k])
                fired += len(hr)
        for packets in rounds:
            check(packets)
        assert fired >= 6 and len(flows) == 4
        # a key reused after end() is a fresh flow: rule [ta] fires again, [alpha, beta] needs both again
        flows.end("a")
        assert "a" not in flows.rule_sets and "a" not in flows.rule_bytes
        text.pop("a")
        carried.pop(key_row.pop("a"))
        key_row["a"] = 10
        check([("a", b"beta")])
        assert flows.scan_rules([]) == []
        # a flow that another scan method fed since (no dictionary file here: a gid is its own code)
        m._codes = np.arange(len(PATS) + 1, dtype=np.uint32)
        flows.scan([("b", b"xyz")])
        with pytest.raises(ValueError, match="scan_rules"):
            flows.scan_rules([("b", b"alpha")])
        # a kept set of another length
        flows.rule_sets["c"] = np.zeros(2, dtype=np.uint64)
        with pytest.raises(ValueError, match="words"):
            flows.scan_rules([("c", b"alpha")])
    finally:
        m.free()


def test_flow_rules_host_form_equals_the_twin():
    m = own_matcher()
    rng = np.random.default_rng(41)
    gids = np.arange(1, 90)
    rules = [[int(g)] for g in gids] * 6 + random_rules(rng, 300, gids)  # more hits than events: the staging is sized first
    m.set_flow_rules(rules)
    W = m.flow_rule_words
    assert W == 2
    nseg, nrows = 200, 230
    dev, host = np.zeros((nrows, W), dtype=np.uint64), np.zeros((nrows, W), dtype=np.uint64)
    for call in range(3):
        offs = random_offsets(rng, nseg)
        events = pack(rng.integers(offs[0], offs[-1] + 1, size=3000), rng.choice(gids, size=3000))
        rows = None if call == 0 else rng.permutation(nrows)[:nseg].astype(np.int64)
        keep = call == 1
        before = dev.copy()
        ptr, hits = m.flow_rules(events, offs, dev, rows, keep=keep)
        exp_ptr, exp_hits = pm.flow_rules_host(events, offs, rules, host, rows, keep=keep)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits) and np.array_equal(dev, host), call
        assert call != 0 or len(hits) > len(events)
        assert not keep or np.array_equal(dev, before)
    # hits_cap short on the host form: rule_ptr complete, the first hits_cap of the sorted ranges, the sets committed
    offs = random_offsets(rng, nseg)
    events = pack(rng.integers(offs[0], offs[-1] + 1, size=500), rng.choice(gids, size=500))
    exp_ptr, exp_hits = pm.flow_rules_host(events, offs, rules, host)
    out, rp = np.full(10 + 8, POISON64, np.uint64), np.zeros(len(offs), np.int64)
    assert m.lib.pm_hip_flow_rules(m.obj, events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p), nseg,
                                   dev.ctypes.data_as(u64p), nrows, None, 0, out.ctypes.data_as(u64p), 10,
                                   rp.ctypes.data_as(i64p)) == 0
    assert len(exp_hits) > 10 and np.array_equal(rp, exp_ptr) and np.array_equal(out[:10], exp_hits[:10])
    assert np.all(out[10:] == POISON64) and np.array_equal(dev, host)
    p0, h0 = m.flow_rules(np.empty(0, np.uint64), offs, dev)
    assert not p0.any() and len(p0) == len(offs) and len(h0) == 0 and np.array_equal(dev, host)
    with pytest.raises(ValueError, match="words"):
        m.flow_rules(events, offs, np.zeros((nrows, W + 1), dtype=np.uint64))
    assert m.scratch_bytes >= 8 * 3000 + 8 * nrows * W + m.flow_rules_scratch_bytes(3000, nseg)


# ---- 10. captured, and between served read_block calls ---------------------------------------------------------
def test_captured_alone_behind_a_fixed_list_buffer_and_replayed():
    """The call captured alone in a graph behind a fixed list buffer and
    replayed over list A, then, with the buffer and its cursor rewritten,
    over list B: hits and sets after each replay equal the twin's two calls."""
    torch = _torch()
    rng = np.random.default_rng(27)
    rules = random_rules(rng, 200, np.arange(1, 25), max_pos=3)
    offs = random_offsets(rng, 300)
    lists = [pack(rng.integers(offs[0], offs[-1], size=n), rng.integers(1, 26, size=n)) for n in (2500, 1800)]
    nseg, cap = len(offs) - 1, 3000
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        m.set_flow_rules(rules)
        host = np.zeros((nseg, words_of(rules)), dtype=np.uint64)
        d_sets = Sets(torch, host)
        d_offs = _dev(torch, offs)
        ev = Ev(torch, cap)
        o = Out(torch, m, cap, nseg, 20000)
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            _call(m, torch, ev, d_offs, nseg, d_sets, nseg, None, 0, o, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert o.untouched() and not d_sets.get().any()  # captured, not run
        totals = []
        for replay, lst in enumerate(lists):
            ev.buf[:len(lst)] = torch.from_numpy(lst.view(np.int64).copy()).cuda()
            ev.nev.fill_(len(lst))
            o.hits[:o.hits_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            exp_ptr, exp_hits = pm.flow_rules_host(lst, offs, rules, host)
            ptr, hits = o.result()
            assert 0 < exp_ptr[-1] <= o.hits_cap, replay
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, f"replay {replay}")
            assert np.all(hits[ptr[-1]:] == POISON64)
            assert np.array_equal(d_sets.get(), host), replay
            totals.append(int(ptr[-1]))
        assert totals[0] != totals[1]
    finally:
        m.free()


def test_call_between_served_read_blocks():
    """Small read_block calls of an rt object go to its resident server grid;
    a flow-rules call after every third asks the grid to leave the device
    first, like every device launch, and the next small call launches it
    again: the gids equal one large call's, every result the twin's."""
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
        f = Flows(rules, 300, m=m)
        parts = []
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(m.read_block_gids(text[a:b]))
            if k % 3 == 2:
                events = pack(rng.integers(0, offs[-1] + 10, size=600), rng.integers(1, 6, size=600))
                ptr, _ = f.call(events, offs, what=f"after block {k}")
                assert ptr[-1] > 0
        assert np.array_equal(np.concatenate(parts), whole)
        s1 = m.serve_stats()
        assert s1["calls"] - s0["calls"] == len(sizes)
        assert s1["launches"] - s0["launches"] >= 3  # the first call, and the call after each stop
    finally:
        m.free()
