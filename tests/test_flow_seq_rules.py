"""The flow ordered rules on the device (pm_hip_set_flow_seq_rules,
pm_hip_flow_seq_rules_device, pm_hip_flow_seq_rules; include/pm_hip.h "flow
ordered rules"): every device call runs in front of poisoned guards around the
rows, the hits, rule_ptr and the scratch and is compared with the host twin
down to the row words; the seeded cases are compared with the keep-everything
reference of flow_seq_rule_inputs.py as well, and cut invariance with the
ordered-rules twin over the uncut flows."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import mixed_offsets, scan_like
from flow_seq_rule_inputs import (KINDS, flow_seq_case, kinds_present, layout_of, reference_flow_seq_rules, rows_array,
                                  run_reference, whole_flows)
from fuzz_inputs import case as fuzz_case
from match_inputs import expected_matches
from nocase_inputs import brute, call_events, flag_of, fuzz_dictionary, fuzz_text, stream_offsets
from oracle_lib import dict_paths
from rule_inputs import random_offsets
from seq_rule_inputs import GID_BITS, GID_MAX, pack, random_seq_rules, seq_csr
from test_batch import _dev, _stream
from test_by_stream import PTR_POISON, SCRATCH_GUARD, _i64, _list_dev
from test_events import GUARD, POISON64, Ev, _text_dev
from test_flow_rules import Sets, _assert_equal, _home, _keys_by_home, _rules_of
from test_flows import STATE_POISON, _states
from test_gpu_parity import SHIP, _torch, fresh_matcher
from test_nocase import _u64, build, gids_of

pytestmark = pytest.mark.gpu

B = 1024  # the scan block's width (csrc/pm_bystream.h PM_BS_SCAN_BLOCK)
NG = 4200  # the hand-made lists use gids 1..NG, all of them patterns of et
KEEP = pm.FLOW_RULES_KEEP
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))

_own = {}


def own_matcher():
    """An auto object over et of this module's own, and its patterns' lengths by gid."""
    if "m" not in _own:
        m = pm.HipMatcher("auto")
        m.add_dictionary(pm.Dictionary(dict_paths("et")))
        m.compile()
        plen = np.array([m.pattern_len(g) for g in range(NG + 1)], dtype=np.uint32)
        assert plen[0] == 0 and np.all(plen[1:] > 0)
        _own["m"], _own["plen"] = m, plen
    return _own["m"], _own["plen"]


def short_gids(plen, n):
    """(gid_map for flow_seq_case: index 0 unused): n gids whose patterns have 2 to 8 bytes, neighbours of
    different lengths (2, 3, ..., 8, 2, ...), so that a link measured with another term's length goes wrong."""
    by_len = {L: np.nonzero(plen == L)[0].tolist() for L in range(2, 9)}
    assert all(len(v) >= 2 for v in by_len.values())
    g = [by_len[2 + k % 7][k // 7] for k in range(n)]
    assert len(set(g)) == n
    return np.array([0] + g, dtype=np.int64)


class Out:
    """The outputs and scratch of one device call, each in front of a guard;
    the scratch has the stated pm_hip_flow_seq_rules_scratch_bytes."""

    def __init__(self, torch, m, cap, nseg, hits_cap):
        self.hits_cap, self.nseg = hits_cap, nseg
        self.hits = _i64(torch, hits_cap + GUARD, POISON64 - (1 << 64))
        self.ptr = _i64(torch, nseg + 1 + GUARD, PTR_POISON)
        self.bytes = m.flow_seq_rules_scratch_bytes(cap, nseg)
        self.scratch = torch.full((self.bytes + SCRATCH_GUARD,), 0xA5, dtype=torch.uint8, device="cuda")

    def untouched(self):
        return (np.all(self.hits.cpu().numpy().view(np.uint64) == POISON64)
                and np.all(self.ptr.cpu().numpy() == PTR_POISON) and np.all(self.scratch.cpu().numpy() == 0xA5))

    def result(self):
        ptr, hits = self.ptr.cpu().numpy(), self.hits.cpu().numpy().view(np.uint64)
        assert np.all(ptr[self.nseg + 1:] == PTR_POISON), "rule_ptr guard"
        assert np.all(hits[self.hits_cap:] == POISON64), "hits guard"
        assert np.all(self.scratch.cpu().numpy()[self.bytes:] == 0xA5), "scratch guard"
        return ptr[:self.nseg + 1], hits[:self.hits_cap]


def _call(m, torch, ev, d_offs, nseg, d_prog, nrows, d_rows, d_pos, flags, o, stream=None):
    m.flow_seq_rules_device(ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), d_offs.data_ptr(), nseg, d_prog.t.data_ptr(),
                            nrows, None if d_rows is None else d_rows.data_ptr(), d_pos.data_ptr(), flags,
                            o.hits.data_ptr(), o.hits_cap, o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes,
                            _stream(torch) if stream is None else stream)


class SeqFlows:
    """The rows of some flows on the device (behind a guard) and their twin's
    on the host; call() runs one device call against the twin's."""

    def __init__(self, rules, nrows, m=None, plen=None, fast=None):
        self.torch = _torch()
        if m is None:
            m, plen = own_matcher()
        self.m, self.plen, self.rules = m, plen, rules
        m.set_flow_seq_rules(rules, fast)
        _, _, C, _, S = layout_of(rules)
        assert m.flow_seq_rule_count() == len(rules) and m.flow_seq_rule_words == S and m.flow_seq_chain_count() == C
        self.host = np.zeros((nrows, S), dtype=np.uint64)
        self.dev = Sets(self.torch, self.host)
        self.nrows = nrows

    def call(self, events, offs, pos_in=None, rows=None, keep=False, cap=None, cursor=None, what=""):
        """The device call on a hand-made list against the twin on the events
        it has to use, with room for exactly the expected hits.  Returns
        (rule_ptr, expected hits)."""
        torch, m = self.torch, self.m
        events = np.ascontiguousarray(events, dtype=np.uint64)
        offs = np.ascontiguousarray(offs, dtype=np.int64)
        nseg = len(offs) - 1
        pos_in = np.zeros(nseg, dtype=np.uint64) if pos_in is None else np.asarray(pos_in, dtype=np.uint64)
        cap = len(events) if cap is None else cap
        cursor = len(events) if cursor is None else cursor
        exp_ptr, exp_hits = pm.flow_seq_rules_host(events[:min(cursor, cap)], offs, self.rules, self.plen, self.host,
                                                   pos_in, rows, keep)
        ev = _list_dev(torch, events, cap, cursor)
        o = Out(torch, m, cap, nseg, len(exp_hits))
        d_rows = None if rows is None else _dev(torch, np.asarray(rows, dtype=np.int64))
        _call(m, torch, ev, _dev(torch, offs), nseg, self.dev, self.nrows, d_rows, _u64(torch, pos_in),
              KEEP if keep else 0, o)
        torch.cuda.synchronize()
        ptr, hits = o.result()
        ev.assert_guard(cap)
        assert ev.total() == cursor
        _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
        assert np.array_equal(self.dev.get(), self.host), f"{what}: the rows differ from the twin's"
        return ptr, exp_hits


def real_case(seed, **kw):
    m, plen = own_matcher()
    return flow_seq_case(seed, real=(short_gids(plen, 10), plen), **kw)


# ---- 1. the planted kinds and random flows, in up to four calls ------------------------------------------
@pytest.mark.parametrize("seed,big,ncalls", [(0, 0, 4), (1, 0, 3), (2, 0, 2), (4, 0, 3), (5, 0, 2),
                                             (3, (1 << 32) - 50, 4), (3, (1 << 32) + 7, 2), (3, (1 << 40) - 120, 3)])
def test_planted_and_random_flows_against_the_reference(seed, big, ncalls):
    """Every planted kind (a head in one call and its follower in the next, a
    chain of three over three calls, A ... A and a straddler across a cut, the
    negations ...), the planted flows cut into two, three and four calls,
    beside random flows, permuted, out-of-range and spare rows
    and a stream with pos_in past 2^57, with flow byte counts from 0, around
    2^32 and near 2^40: the device equals the twin (in call()) and the
    reference, rows included, call after call."""
    case = real_case(seed, nflows=24 if big == 0 else 8, big_base=big, planted_calls=ncalls)
    ref = run_reference(case)
    seen = kinds_present(case, ref)
    assert set(seen) == set(KINDS) and all(seen.values()), seen
    f = SeqFlows(case["rules"], case["nrows"])
    for c, (call, (ptr, hits, rows_after)) in enumerate(zip(case["calls"], ref)):
        got_ptr, got = f.call(call["events"], call["offsets"], call["pos_in"], call["rows"], what=f"call {c}")
        assert np.array_equal(got_ptr, ptr) and np.array_equal(got, hits), c
        assert np.array_equal(f.host, rows_after), c


@pytest.mark.parametrize("seed", range(2))
def test_cut_invariance_on_the_device(seed):
    """The union over the calls of the device's hits, in flow coordinates,
    against pm_flat_seq_rules_by_stream over the uncut flows, for three cuts of
    the same flows: equal for every rule without a negated term; for a rule
    with one the uncut hits are a subset (a later negation retracts nothing)."""
    whole = None
    for cut_seed in range(3):
        case = real_case(seed, cut_seed=cut_seed)
        rules = case["rules"]
        plain = {r for r, rule in enumerate(rules) if all(g > 0 for g, _ in rule)}
        if whole is None:
            events, offs = whole_flows(case)
            ptr, hits = pm.seq_rules_by_stream_host(events, offs, rules, case["plen"])
            whole = {fl: sorted(((h >> GID_BITS) - int(offs[fl]), h & GID_MAX) for h in hits[ptr[fl]:ptr[fl + 1]].tolist())
                     for fl in range(len(offs) - 1)}
            assert sum(1 for v in whole.values() for _, r in v if r in plain) > 20
        f = SeqFlows(rules, case["nrows"])
        got = {}
        for c, call in enumerate(case["calls"]):
            ptr, hits = f.call(call["events"], call["offsets"], call["pos_in"], call["rows"], what=f"cut {cut_seed}")
            for s, fl in enumerate(call["flow"]):
                for h in hits[ptr[s]:ptr[s + 1]].tolist():
                    got.setdefault(fl, []).append(((h >> GID_BITS) - int(call["offsets"][s]) + int(call["pos_in"][s]),
                                                   h & GID_MAX))
        for fl, want in whole.items():
            mine = sorted(got.get(fl, []))
            assert [h for h in mine if h[1] in plain] == [h for h in want if h[1] in plain], (cut_seed, fl)
            assert set(want) <= set(mine), (cut_seed, fl)


def test_a_distance_larger_than_a_packet():
    """Packets of 100 bytes, a distance of 5,000: the follower of packet 2 is
    too close, the one of the packet at flow byte 6,000 completes the chain."""
    m, plen = own_matcher()
    d = 5000 - int(plen[2])  # the follower must end at flow byte 30 + d + L = 5,030 or later
    rules = [[(1, None), (2, d)]]
    f = SeqFlows(rules, 1)
    _, h = f.call(pack([40], [1]), [10, 110], [0])
    assert len(h) == 0 and f.host[0, 0] == ((30 + 1) << 6)
    _, h = f.call(pack([50], [2]), [10, 110], [100])
    assert len(h) == 0
    _, h = f.call(pack([10 + 29, 10 + 30], [2, 2]), [10, 110], [5000])
    assert h.tolist() == [((10 + 30) << 24) | 0] and f.host[0, 0] == ((5030 + 1) << 6) | 1


def test_a_chain_of_64_terms_over_three_calls():
    m, plen = own_matcher()
    gids = list(range(1, 65))
    rules = [[(gids[0], None)] + [(g, 0) for g in gids[1:]]]
    f = SeqFlows(rules, 2)
    step = 300  # longer than any pattern here: every link is satisfied
    assert plen[1:65].max() < step
    at = lambda lo, hi: pack([5 + step * (k - lo) for k in range(lo, hi)], gids[lo:hi])  # noqa: E731
    _, h = f.call(at(0, 20), [5, 5 + step * 20, 5 + step * 20], [0, 0])
    assert len(h) == 0 and int(f.host[0, 0]) & 63 == 19
    # every later term is in this call too, but only the next 43 lie behind the carried level in order
    _, h = f.call(at(20, 63), [5, 5 + step * 43, 5 + step * 43], [step * 20, 0])
    assert len(h) == 0 and int(f.host[0, 0]) & 63 == 62
    _, h = f.call(pack([9, 8], [gids[63], gids[5]]), [5, 400, 400], [step * 63, 0])
    assert h.tolist() == [(9 << 24) | 0]
    assert int(f.host[0, 0]) == ((step * 63 + 4 + 1) << 6) | 63


@pytest.mark.parametrize("present", [1, 2, 64])
def test_the_owner_election_with_1_2_and_64_present_gids(present):
    """Rule 0 has 64 free terms, rule 1 two chains; a stream holds `present`
    of rule 0's gids in call 1 and all of them in call 2 (64: all at once).
    Whichever slots the stream has, the pair is evaluated once: a second
    owner would report the hit twice."""
    gids = list(range(101, 165))
    rules = [[(g, None) for g in gids], [(101, None), (102, 0), (103, None), (164, 0)], [(150, None), (101, 0)]]
    f = SeqFlows(rules, 3)
    offs = [0, 40000, 80000]
    first = gids[-present:]  # the rule's LAST gids: the owner is not the rule's first term
    ev1 = pack([300 * k for k in range(present)] + [40000 + 300 * k for k in range(present)], first + first)
    p1, h1 = f.call(ev1, offs, [0, 0], rows=[2, 0], what="call 1")
    assert (0 in _rules_of(h1)) == (present == 64)
    ev2 = pack([300 * k for k in range(64)], gids)
    p2, h2 = f.call(ev2, offs, [40000, 40000], rows=[2, 0], what="call 2")
    assert _rules_of(h2).count(0) == (0 if present == 64 else 1)
    assert 1 in _rules_of(h1) + _rules_of(h2)


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_one_slot_indexing_n_rules(n):
    """gid 7 heads n rules [7, g at a distance] / [7, -g]: one table slot per
    stream holds it and its wave walks them a rule per lane in turns of 64.
    Flow 0 gets 7 in call 1 and the followers in call 2, flow 1 the other way
    round (nothing may fire: the followers lie before the head), flow 2 all
    at once."""
    rules = [[(7, None), (100 + k, k % 5)] if k % 3 else [(7, None), (-(100 + k), None)] for k in range(n)]
    rng = np.random.default_rng(n)
    offs = [5, 4000, 4000, 9000, 14000]
    f = SeqFlows(rules, 4)
    others = lambda lo, hi, size: pack(rng.integers(lo, hi, size=size), rng.integers(100, 100 + n + 5, size=size))  # noqa: E731
    p1, _ = f.call(np.concatenate([pack([10, 20], [7, 7]), others(4000, 9000, 300), others(9500, 14000, 200),
                                   pack([9100], [7])]), offs, [0, 0, 0, 0], what=f"{n} rules, call 1")
    p2, _ = f.call(np.concatenate([others(400, 4000, 300), pack([4100, 4200], [7, 7])]), offs,
                   [3995, 0, 5000, 5000], what=f"{n} rules, call 2")
    assert p1[-1] > 0 and (n == 1 or p2[1] > 0)


def test_a_wave_in_which_every_lane_has_a_slot_and_one_in_which_only_lane_63_does():
    """cap 1,024, so a table of 2,048 slots.  64 keys whose home slots are the
    64 slots of wave 3 and are distinct (nothing probes), every gid among them
    in two rules; one key at slot 64 * 9 + 63, the owner of a rule whose other
    term's key lies in another wave."""
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
        rules += [[(g, None)], [(g, None), (-4000, None)]]
    rules.append([(last[1], None), (other[1], None)])
    f = SeqFlows(rules, nseg)
    ptr, hits = f.call(events, offs, cap=1024)
    assert ptr[-1] == 2 * 64 + 1
    assert ((int(offs[last[0]]) + 5) << 24) | (len(rules) - 1) in hits[ptr[last[0]]:ptr[last[0] + 1]].tolist()


@pytest.mark.parametrize("shape", ["chains alone", "bits alone", "bits 63 and 64"])
def test_row_shapes(shape):
    """S with K = 0 (W = 0), with C = 0, and with 65 bits behind a chain word."""
    m, _ = own_matcher()
    if shape == "chains alone":
        rules = [[(1, None), (2, 0)], [(3, None), (4, 1), (5, 2)]]
    elif shape == "bits alone":
        rules = [[(1, None), (2, None)], [(3, None), (-4, None)]]
    else:
        rules = [[(g, None)] for g in range(1, 66)] + [[(200, None), (64, 0)], [(65, None), (-64, None)]]
    f = SeqFlows(rules, 3)
    _, _, C, K, S = layout_of(rules)
    assert (C, K, S) == {"chains alone": (2, 0, 2), "bits alone": (0, 4, 1), "bits 63 and 64": (1, 65, 3)}[shape]
    if shape == "bits 63 and 64":
        assert m.flow_seq_rule_bit(64) == 63 and m.flow_seq_rule_bit(65) == 64 and m.flow_seq_rule_bit(200) == -1
        assert m.flow_seq_chain_word(65, 0) == 0 and m.flow_seq_chain_word(65, 1) == -1
        assert m.flow_seq_chain_word(0, 0) == -1 and m.flow_seq_chain_word(99, 0) == -1
    gids = sorted({abs(g) for r in rules for g, _ in r})
    rng = np.random.default_rng(7)
    offs = [0, 3000, 6000, 9000]
    total = 0
    for call in range(2):
        ev = pack(rng.integers(0, 9000, size=60), rng.choice(gids, size=60))
        if shape == "bits 63 and 64":
            ev = np.concatenate([ev, pack([100 + 2500 * call, 3100 + 2500 * call], [64 + call, 65 - call])])
        ptr, _ = f.call(ev, offs, [3000 * call] * 3, what=f"{shape}, call {call}")
        total += int(ptr[-1])
    assert total > 0
    if shape == "bits 63 and 64":
        assert f.host[0, 1] >> np.uint64(63) == 1 and f.host[0, 2] & np.uint64(1) == 1


@pytest.mark.parametrize("n", [16, 17, 4097])
def test_a_range_of_n_occurrences_feeds_the_bisection(n):
    """The follower occurs n times in the call (a range sorted by a lane up to
    16 positions, by a workgroup beyond).  Flow 0 carries the head from a
    packet of 100 bytes at flow byte 10^6 and the distance puts the bound
    exactly on the middle occurrence; flow 1 has its head in this call, three
    bytes in front of the middle occurrence."""
    m, plen = own_matcher()
    L2 = int(plen[2])
    rng = np.random.default_rng(n)
    span = 4 * n + 1000
    where = np.sort(rng.choice(np.arange(600, span), size=n, replace=False))
    mid = int(where[n // 2])
    Q = 1000000
    d = 50 + mid - L2  # Q + 50 + d + L2 == Q + 100 + mid
    rules = [[(1, None), (2, d)], [(3, None), (2, 3)]]
    f = SeqFlows(rules, 2)
    _, h = f.call(pack([7 + 50], [1]), [7, 107, 107], [Q, 0], what="the head")
    assert len(h) == 0
    offs = [7, 7 + span, 7 + 2 * span]
    ev = np.concatenate([pack(7 + where, np.full(n, 2)), pack(7 + span + where, np.full(n, 2)),
                         pack([7 + span + mid - 3 - L2], [3])])
    ptr, hits = f.call(rng.permutation(ev), offs, [Q + 100, 0], what=f"{n} occurrences")
    assert hits.tolist() == [((7 + mid) << 24) | 0, ((7 + span + mid) << 24) | 1]
    assert int(f.host[0, 0]) == ((Q + 100 + mid + 1) << 6) | 1 and int(f.host[1, 1]) == ((mid + 1) << 6) | 1


def test_more_slots_than_one_grid():
    """600,000 events: a table of 2^21 slots, more than one grid of lanes, so
    the grid-stride loops of the index, the evaluations and the commit turn
    again; two calls; a chain completes across them in the first and in the
    last stream."""
    torch = _torch()
    lanes = 8 * 256 * torch.cuda.get_device_properties(0).multi_processor_count
    n = 600000
    assert lanes < (1 << 21)
    rng = np.random.default_rng(22)
    offs = mixed_offsets(rng)
    lens = np.diff(offs)
    full = np.nonzero(lens > 0)[0]
    first, last = int(full[0]), int(full[-1])
    rules = random_seq_rules(rng, 200, range(1, 11)) + [[(20, None), (21, 0)], [(21, None), (20, 0), (-1, None)]]
    f = SeqFlows(rules, len(offs) - 1)
    events = np.concatenate([scan_like(n - 2, offs, np.arange(1, 9), rng), pack([offs[first], offs[last + 1] - 1], [20, 20])])
    f.call(events, offs, np.zeros(len(lens)), what="call 1")
    events = np.concatenate([scan_like(n - 2, offs, np.arange(1, 11), rng), pack([offs[first], offs[last + 1] - 1], [21, 21])])
    ptr, hits = f.call(events, offs, lens, what="call 2")
    assert 200 in _rules_of(hits[ptr[last]:ptr[last + 1]])


@pytest.mark.parametrize("nseg", [1, B - 1, B, B + 1, 3000])
def test_scan_sizes(nseg):
    rng = np.random.default_rng(nseg)
    rules = [[(1, None)], [(1, None), (2, 0)], [(2, None), (-3, None)], [(3, None), (4, 0), (5, 0)], [(5, None), (-1, None)]]
    f = SeqFlows(rules, nseg + 2)
    had = np.zeros(nseg, dtype=np.uint64)
    for call in range(2):
        offs = random_offsets(rng, nseg, max_len=3, base=17)
        if offs[-1] == offs[0]:
            offs[-1] += 2
        pos = np.concatenate([[offs[0], offs[-1] - 1, offs[-1] - 1], rng.integers(offs[0] - 2, offs[-1] + 2, size=2000)])
        events = pack(pos, np.concatenate([[1, 1, 2], rng.integers(1, 6, size=2000)]))
        ptr, _ = f.call(events, offs, had, what=f"nseg {nseg}, call {call}")
        had += np.diff(offs).astype(np.uint64)
        assert ptr[-1] > 0 or call == 1


def test_cursor_above_cap_and_below_the_list():
    rng = np.random.default_rng(23)
    events = pack(rng.integers(0, 500, size=1500), rng.integers(1, 9, size=1500))
    rules = random_seq_rules(rng, 60, range(1, 10))
    f = SeqFlows(rules, 3)
    few = pack(rng.integers(0, 500, size=300), rng.integers(1, 5, size=300))
    a, _ = f.call(few, [0, 100, 250, 500], [0, 0, 0], cap=300, cursor=300 + 100000)
    # the slots past the cursor hold poison: as events they lie inside the last stream here
    b, _ = f.call(events, [0, 100, 250, 1 << 40], [100, 150, 250], cap=2000, cursor=700)
    assert a[-1] > 0 and b[-1] > 0
    before = f.host.copy()
    c, _ = f.call(np.empty(0, np.uint64), [0, 100, 250, 1 << 40], [200, 300, 500], cap=2000, cursor=0)
    assert c.tolist() == [0, 0, 0, 0] and np.array_equal(f.host, before)


# ---- 2. the protocol ------------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["one", "all"])
def test_hits_cap_short_keeps_rule_ptr_exact_and_commits(short):
    torch = _torch()
    m, plen = own_matcher()
    rng = np.random.default_rng(24)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 40, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    rules = random_seq_rules(rng, 600, range(1, 42), max_gap=20)
    m.set_flow_seq_rules(rules)
    S = m.flow_seq_rule_words
    host = np.zeros((nseg, S), dtype=np.uint64)
    pos_in = np.zeros(nseg, dtype=np.uint64)
    exp_ptr, exp_hits = pm.flow_seq_rules_host(events, offs, rules, plen, host, pos_in)
    total = int(exp_ptr[-1])
    assert total > 300 and host.any()
    hits_cap = total - 1 if short == "one" else 0
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, hits_cap)
    d_prog = Sets(torch, np.zeros_like(host))
    _call(m, torch, ev, _dev(torch, offs), nseg, d_prog, nseg, None, _u64(torch, pos_in), 0, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()  # (the guard behind hits_cap is checked there)
    assert np.array_equal(ptr, exp_ptr) and np.array_equal(d_prog.get(), host)
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = set(zip(seg.tolist(), exp_hits.tolist()))
    got = list(zip(seg[:hits_cap].tolist(), hits.tolist()))
    assert len(set(got)) == len(got) == hits_cap and set(got) <= want


def test_keep_then_the_committing_call_then_nothing():
    rng = np.random.default_rng(25)
    rules = random_seq_rules(rng, 300, range(1, 30), max_gap=20)
    f = SeqFlows(rules, 10)
    offs = np.arange(0, 301, 30)
    for call in range(2):
        events = pack(rng.integers(0, 300, size=150), rng.integers(1, 30, size=150))
        pos_in = np.full(10, 30 * call)
        before = f.host.copy()
        kp, kh = f.call(events, offs, pos_in, keep=True, what="keep")
        assert np.array_equal(f.host, before)
        cp, ch = f.call(events, offs, pos_in, what="commit")
        assert np.array_equal(kp, cp) and np.array_equal(kh, ch) and cp[-1] > 0
        ap, _ = f.call(events, offs, pos_in, what="again")
        assert ap[-1] == 0


def _good_args(torch, m, nseg=2, nrows=2):
    events = pack([1, 2, 3, 3], [1, 1, 2, 2])
    offs = np.array([0, 2, 4], dtype=np.int64)
    ev = _list_dev(torch, events, 4, 4)
    o = Out(torch, m, 4, nseg, 4)
    d_prog = Sets(torch, np.zeros((nrows, max(m.flow_seq_rule_words, 1)), dtype=np.uint64))
    d_offs, d_rows = _dev(torch, offs), _dev(torch, np.array([1, 0], dtype=np.int64))
    d_pos = _u64(torch, np.zeros(nseg + 1, np.uint64))
    good = dict(e=ev.buf.data_ptr(), cap=4, c=ev.nev.data_ptr(), o=d_offs.data_ptr(), nseg=nseg, prog=d_prog.t.data_ptr(),
                nrows=nrows, rows=d_rows.data_ptr(), pos=d_pos.data_ptr(), flags=0, h=o.hits.data_ptr(), hits_cap=4,
                p=o.ptr.data_ptr(), s=o.scratch.data_ptr(), sb=o.bytes, st=_stream(torch))
    return good, (ev, o, d_prog, d_offs, d_rows, d_pos), events, offs


ORDER = ("e", "cap", "c", "o", "nseg", "prog", "nrows", "rows", "pos", "flags", "h", "hits_cap", "p", "s", "sb", "st")


def test_before_set_flow_seq_rules_is_minus_12_and_nothing_is_touched():
    torch = _torch()
    m = fresh_matcher("et", "rt")
    try:
        for with_others in (False, True):
            if with_others:  # the other three rule sets change nothing here
                m.set_rules([[1, 2], [2]])
                m.set_flow_rules([[1, 2]])
                m.set_seq_rules([[(1, None), (2, 0)]])
            assert m.flow_seq_rule_count() == 0 and m.flow_seq_rules_min_len() == 0 and m.flow_seq_rule_words == 0
            assert m.flow_seq_rule_bit(1) == -1 and m.flow_seq_chain_word(0, 0) == -1 and m.flow_seq_chain_count() == 0
            good, keep_alive, events, offs = _good_args(torch, m)
            _, o, d_prog, _, _, _ = keep_alive
            args = [good[k] for k in ORDER]
            assert m.lib.pm_hip_flow_seq_rules_device(m.obj, *args) == -12
            assert b"pm_hip_set_flow_seq_rules" in m.lib.pm_hip_last_error()
            hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
            prog, pos = np.full((2, 1), 0x77, np.uint64), np.zeros(2, np.uint64)
            host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, prog.ctypes.data_as(u64p), 2, None,
                    pos.ctypes.data_as(u64p), 0, hits.ctypes.data_as(u64p), 4, ptr.ctypes.data_as(i64p)]
            assert m.lib.pm_hip_flow_seq_rules(m.obj, *host) == -12
            torch.cuda.synchronize()
            assert o.untouched() and not d_prog.get().any()
            assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON) and np.all(prog == 0x77)
            args[4] = -1  # bad arguments come first, as the return codes are ordered
            assert m.lib.pm_hip_flow_seq_rules_device(m.obj, *args) == -2
    finally:
        m.free()
    raw = pm.HipMatcher("rt")
    raw.add_pattern(b"abc")
    tptr, terms, gaps = seq_csr([[(1, None)]])
    assert raw.lib.pm_hip_set_flow_seq_rules(raw.obj, tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                             gaps.ctypes.data_as(u32p), 1) == -1
    assert raw.lib.pm_hip_flow_seq_rules_device(raw.obj, *args) == -1
    raw.free()


def test_bad_arguments_are_minus_2_and_nothing_is_touched():
    torch = _torch()
    m, _ = own_matcher()
    lib = m.lib
    m.set_flow_seq_rules([[(1, None), (2, 0)], [(2, None)]])
    good, keep_alive, events, offs = _good_args(torch, m)
    _, o, d_prog, _, _, _ = keep_alive
    bad = [dict(e=None), dict(c=None), dict(o=None), dict(h=None), dict(p=None), dict(s=None), dict(prog=None),
           dict(pos=None), dict(pos=good["pos"] + 4),
           dict(e=good["e"] + 4), dict(c=good["c"] + 4), dict(o=good["o"] + 4), dict(h=good["h"] + 4),
           dict(p=good["p"] + 4), dict(s=good["s"] + 8), dict(prog=good["prog"] + 4), dict(rows=good["rows"] + 4),
           dict(nseg=-1), dict(nseg=1 << 31), dict(cap=(1 << 40) + 1), dict(h=good["e"]), dict(sb=o.bytes - 1), dict(sb=0),
           dict(nrows=-1), dict(nrows=(1 << 40) + 1), dict(rows=None, nrows=1), dict(flags=2), dict(flags=KEEP | 4),
           dict(flags=1 << 31)]
    for b in bad:
        assert lib.pm_hip_flow_seq_rules_device(m.obj, *[{**good, **b}[k] for k in ORDER]) == -2, b
        assert b"bad arguments" in lib.pm_hip_last_error(), b
    torch.cuda.synchronize()
    assert o.untouched() and not d_prog.get().any()
    # nseg == 0: nothing launched or written, whatever the other pointers are (pos_in is always required)
    assert lib.pm_hip_flow_seq_rules_device(m.obj, *[{**good, "nseg": 0, "o": None, "s": None, "sb": 0, "rows": None}[k]
                                                     for k in ORDER]) == 0
    torch.cuda.synchronize()
    assert o.untouched() and not d_prog.get().any()
    # cap == 0 with streams: an all-zero rule_ptr, untouched rows, nothing else
    assert lib.pm_hip_flow_seq_rules_device(m.obj, *[{**good, "cap": 0, "e": None}[k] for k in ORDER]) == 0
    torch.cuda.synchronize()
    ptr, hits = o.result()
    assert ptr.tolist() == [0, 0, 0] and np.all(hits == POISON64) and not d_prog.get().any()
    # the host form's -2 cases
    hits, ptr = np.full(4, POISON64, np.uint64), np.full(3, PTR_POISON, np.int64)
    prog, rows, pos = np.full((2, 2), 0x77, np.uint64), np.array([1, 0], np.int64), np.zeros(2, np.uint64)
    host = [events.ctypes.data_as(u64p), 4, offs.ctypes.data_as(i64p), 2, prog.ctypes.data_as(u64p), 2,
            rows.ctypes.data_as(i64p), pos.ctypes.data_as(u64p), 0, hits.ctypes.data_as(u64p), 4, ptr.ctypes.data_as(i64p)]
    for k, v in ((0, None), (2, None), (11, None), (9, None), (4, None), (7, None), (3, 1 << 31), (1, (1 << 40) + 1),
                 (9, events.ctypes.data_as(u64p)), (8, 2), (5, (1 << 40) + 1)):
        a = list(host)
        a[k] = v
        assert lib.pm_hip_flow_seq_rules(m.obj, *a) == -2, k
        assert b"bad arguments" in lib.pm_hip_last_error(), k
    a = list(host)
    a[5], a[6] = 1, None  # no rows and fewer rows than streams
    assert lib.pm_hip_flow_seq_rules(m.obj, *a) == -2
    assert np.all(hits == POISON64) and np.all(ptr == PTR_POISON) and np.all(prog == 0x77)
    with pytest.raises(ValueError, match="within"):
        m.set_flow_seq_rules([[(1, None), (2, 0, 50)]])
    assert m.flow_seq_rule_count() == 2


def test_every_bad_rule_set_is_minus_2_and_the_rules_stay():
    m, _ = own_matcher()
    lib = m.lib
    rules = [[(1, None), (2, 0)], [(2, None), (-3, None)]]
    f = SeqFlows(rules, 3)
    before = m.table_bytes
    F = 0xFFFFFFFF
    u32 = lambda v: np.array(v, dtype=np.uint32)  # noqa: E731
    cases = [("no term_ptr", None, u32([1]), u32([F]), 1), ("no terms", u32([0, 1]), None, u32([F]), 1),
             ("no gaps", u32([0, 1]), u32([1]), None, 1), ("no rules", u32([0]), u32([1]), u32([F]), 0),
             ("term_ptr not from 0", u32([1, 2]), u32([1, 2]), u32([F, F]), 1),
             ("an empty rule", u32([0, 0]), u32([1]), u32([F]), 1),
             ("65 terms", u32([0, 65]), u32(range(1, 66)), u32([F] + [0] * 64), 1),
             ("only negated", u32([0, 1]), u32([1 | 1 << 31]), u32([F]), 1),
             ("unknown bit", u32([0, 1]), u32([1 | 1 << 29]), u32([F]), 1),
             ("two fast", u32([0, 2]), u32([1 | 1 << 30, 2 | 1 << 30]), u32([F, 0]), 1),
             ("fast on a negated term", u32([0, 2]), u32([1, 2 | 3 << 30]), u32([F, F]), 1),
             ("gid 0", u32([0, 2]), u32([1, 0]), u32([F, 0]), 1),
             ("a gap on the first positive term", u32([0, 2]), u32([1, 2]), u32([0, 0]), 1),
             ("a gap on a negated term", u32([0, 2]), u32([1, 2 | 1 << 31]), u32([F, 3]), 1),
             ("a gap above 2^31", u32([0, 2]), u32([1, 2]), u32([F, 0x80000000]), 1),
             ("a gid twice free", u32([0, 2]), u32([1, 1]), u32([F, F]), 1),
             ("a gid positive and negated", u32([0, 2]), u32([1, 1 | 1 << 31]), u32([F, F]), 1)]
    ptr_of = lambda a: None if a is None else a.ctypes.data_as(u32p)  # noqa: E731
    for name, tptr, terms, gaps, n in cases:
        assert lib.pm_hip_set_flow_seq_rules(m.obj, ptr_of(tptr), ptr_of(terms), ptr_of(gaps), n) == -2, name
        msg = lib.pm_hip_last_error()
        for word in (b"2^24", b"64", b"positive", b"twice", b"PM_RULE_FAST", b"negated", b"pattern", b"gap", b"within"):
            assert word in msg, (name, word)
        assert m.flow_seq_rule_count() == 2 and m.table_bytes == before, name
    ptr, hits = f.call(pack([1, 400, 405, 406, 900], [1, 2, 2, 3, 2]), [0, 404, 406, 909], [0, 0, 0])
    assert _rules_of(hits) == [0, 1, 1]  # the middle stream holds 2 and 3


def test_a_reload_replaces_the_tables_and_the_other_three_sets_are_independent():
    m, _ = own_matcher()
    rng = np.random.default_rng(26)
    events = pack(rng.integers(0, 300, size=2000), rng.integers(1, 30, size=2000))
    offs = np.arange(0, 301, 30)
    first = random_seq_rules(rng, 300, range(1, 31), max_gap=15)
    second = random_seq_rules(rng, 40, range(1, 31), max_pos=2)
    m.set_rules([[1, 2]])
    m.set_flow_rules([[1, 2]])
    m.set_seq_rules([[(1, None), (2, 0)]])
    a, ha = SeqFlows(first, 10).call(events, offs)
    base = m.table_bytes
    assert m.flow_seq_rules_min_len() == min(m.pattern_len(abs(g)) for r in first for g, _ in r)
    assert m.rule_count() == 1 and m.flow_rule_count() == 1 and m.seq_rule_count() == 1
    b, hb = SeqFlows(second, 10).call(events, offs)
    assert m.flow_seq_rule_count() == 40 and m.table_bytes < base  # the first tables were freed and are no longer counted
    assert not np.array_equal(a, b)
    m.set_seq_rules([[(3, None), (4, 0)], [(5, None)], [(6, None), (7, 1), (8, 2)]])  # larger tables of another kind
    m.set_flow_rules([[3, 4], [5], [6, 7, 8]])
    c, hc = SeqFlows(first, 10).call(events, offs)
    assert np.array_equal(a, c) and np.array_equal(ha, hc) and m.table_bytes > base
    assert m.rule_count() == 1 and m.flow_rule_count() == 3 and m.seq_rule_count() == 3 and m.flow_seq_rule_count() == 300
    # PM_RULE_FAST is accepted and changes no result
    fast = [next(g for g, _ in r if g > 0) if k % 2 else None for k, r in enumerate(first)]
    d, hd = SeqFlows(first, 10, fast=fast).call(events, offs)
    assert np.array_equal(a, d) and np.array_equal(ha, hd)


# ---- 3. behind real scans --------------------------------------------------------------------------------
def _seq_rules_from_lists(rng, ev_a, ev_b, offs, plen):
    """Ordered rules over the gids of two calls' lists: per picked stream a
    term of call 1 followed, at a distance, by a term of call 2, the reverse
    order (which cannot fire), negations, and, where there is one, a straddler
    rule: a pattern of call 1 followed at distance 0 by an event of call 2
    whose pattern begins in call 1's bytes, behind the first pattern's end.
    Returns (rules, (the straddler rule, its stream) or None)."""
    nseg = len(offs) - 1
    lens = np.diff(offs)
    pa, ga = pm.unpack_events(ev_a)
    pb, gb = pm.unpack_events(ev_b)
    ja, jb = np.searchsorted(offs, pa, side="right") - 1, np.searchsorted(offs, pb, side="right") - 1
    rules, straddle = [], None
    for j in rng.permutation(nseg).tolist():
        a = np.unique(ga[ja == j])
        b = np.setdiff1d(np.unique(gb[jb == j]), a)
        if len(a) == 0 or len(b) == 0:
            continue
        if straddle is None:
            inside = jb == j
            for q, g in zip(pb[inside].tolist(), gb[inside].tolist()):
                start = int(lens[j]) + q - int(offs[j]) - int(plen[g]) + 1  # in flow bytes
                if start >= int(lens[j]) or g in a:
                    continue
                heads = [(int(p), int(x)) for p, x in zip(pa[ja == j].tolist(), ga[ja == j].tolist())]
                ok = [x for x in set(x for _, x in heads) if min(p for p, y in heads if y == x) - int(offs[j]) < start]
                if ok:
                    straddle = (len(rules), j)
                    rules.append([(ok[0], None), (g, 0)])
                    break
        if len(rules) < 120:
            x, y = int(rng.choice(a)), int(rng.choice(b))
            rules += [[(x, None), (y, int(rng.integers(0, 4)))], [(y, None), (x, 0)], [(x, None), (-y, None)],
                      [(y, None), (-x, None)]][:1 + len(rules) % 4]
            if len(a) > 1:
                rules.append([(int(a[0]), None), (int(a[1]), None), (y, 0)])
    return rules, straddle


def _two_calls_behind(m, torch, scans, offs, ev_a, ev_b, rules, plen, straddle, what):
    """scans[c](ev, d_offs) enqueues call c's list scan; the flow ordered-rules
    call follows with no synchronize between, twice, then one synchronize: the
    hits and the rows against the reference over the oracle's lists."""
    nseg = len(offs) - 1
    lens = np.diff(offs).astype(np.uint64)
    pos = [np.zeros(nseg, dtype=np.uint64), lens]
    state = {}
    exp = [reference_flow_seq_rules(state, e, offs, p, rules, plen, nseg) for e, p in zip((ev_a, ev_b), pos)]
    assert exp[0][0][-1] > 0 and exp[1][0][-1] > 0
    if straddle is not None:
        r, j = straddle
        assert r in _rules_of(exp[1][1][exp[1][0][j]:exp[1][0][j + 1]]), "the straddler rule fires in call 2"
    d_offs = _dev(torch, offs)
    d_prog = Sets(torch, np.zeros((nseg, m.flow_seq_rule_words), dtype=np.uint64))
    d_pos = [_u64(torch, p) for p in pos]
    evs = [Ev(torch, len(e) + 100) for e in (ev_a, ev_b)]
    outs = [Out(torch, m, ev.cap, nseg, len(x[1])) for ev, x in zip(evs, exp)]
    for c in range(2):
        scans[c](evs[c], d_offs)
        _call(m, torch, evs[c], d_offs, nseg, d_prog, nseg, None, d_pos[c], 0, outs[c])
    torch.cuda.synchronize()
    for c, e in enumerate((ev_a, ev_b)):
        assert evs[c].total() == len(e), f"{what}, call {c + 1}"
        ptr, hits = outs[c].result()
        _assert_equal(ptr, hits, exp[c][0], exp[c][1], f"{what}, call {c + 1}")
    assert np.array_equal(d_prog.get(), rows_array(state, rules, plen, nseg)), what


@pytest.mark.parametrize("name", ["unary", "many", "seed0", "seed5"])
def test_behind_the_flow_scan_in_two_calls(name):
    torch = _torch()
    c = fuzz_case(name)
    offs, nseg, n = c.offs, c.nseg, len(c.A)
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary(dict_paths(name)))
    m.compile()
    try:
        codes = np.asarray(m._codes, dtype=np.uint32)
        order = np.argsort(codes)
        plen = np.array([m.pattern_len(g) for g in range(len(codes))], dtype=np.int64)

        def lists(min_len):
            out = []
            for exp in (c.ea, c.eb):
                pos, pcodes = expected_matches(name, exp, min_len)
                out.append(pack(pos, order[np.searchsorted(codes[order], pcodes)]))
            return out
        ev_a, ev_b = lists(1)
        rules, straddle = _seq_rules_from_lists(np.random.default_rng(len(name)), ev_a, ev_b, offs, plen)
        assert straddle is not None and len(rules) > 20
        m.set_flow_seq_rules(rules)
        min_len = m.flow_seq_rules_min_len()
        assert min_len == min(plen[abs(g)] for r in rules for g, _ in r)
        ev_a, ev_b = lists(min_len)
        d_a, d_b = _text_dev(torch, c.A), _text_dev(torch, c.B)
        st = _states(torch, np.full(nseg, STATE_POISON, np.uint32))

        def scan_a(ev, d_offs):
            m.scan_flows_matches_device(d_a.data_ptr(), d_offs.data_ptr(), nseg, n, None, st.data_ptr(), min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))

        def scan_b(ev, d_offs):
            m.scan_flows_matches_device(d_b.data_ptr(), d_offs.data_ptr(), nseg, n, st.data_ptr(), None, min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
        _two_calls_behind(m, torch, (scan_a, scan_b), offs, ev_a, ev_b, rules, plen, straddle, name)
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
        A, B2 = fuzz_text(pats, 0, 49152), fuzz_text(pats, 50, 49152)
        offs = stream_offsets(len(A), 0)
        nseg, n, lens = len(offs) - 1, len(A), np.diff(offs)
        whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B2[offs[j]:offs[j + 1]]) for j in range(nseg)]
        plen = np.array([m.pattern_len(g) for g in range(len(pats) + 1)], dtype=np.int64)

        def lists(min_len):
            rows, _ = brute(pats, flags_nc, whole, gid, min_len)
            return call_events(rows, offs, np.zeros(nseg, np.int64))[0], call_events(rows, offs, lens)[0]
        ev_a, ev_b = lists(1)
        rules, _ = _seq_rules_from_lists(np.random.default_rng(9), ev_a, ev_b, offs, plen)
        m.set_flow_seq_rules(rules)
        min_len = m.flow_seq_rules_min_len()
        ev_a, ev_b = lists(min_len)
        W = m.case_words
        d_a, d_b = _text_dev(torch, A), _text_dev(torch, B2)
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
        _two_calls_behind(m, torch, (scan_a, scan_b), offs, ev_a, ev_b, rules, plen, None, "nocase")
    finally:
        m.free()


PATS = [b"alpha", b"beta", b"gamma", b"ta", b"delta", b"mma"]


def test_behind_the_window_flow_scan_sharing_its_byte_counts():
    """The window flow scan writes each flow's byte count; the same array is
    this call's pos_in in the next round.  "ta" may begin at flow byte 12 or
    later only, so the "ta" inside "beta" at the flow's start does not count."""
    m = build(PATS, "auto")
    try:
        gid = gids_of(m, len(PATS))
        g = {p: int(gid[k]) for k, p in enumerate(PATS)}
        lo = np.zeros(len(PATS), dtype=np.uint32)
        lo[PATS.index(b"ta")] = 12
        m.set_windows(lo, np.full(len(PATS), 0xFFFFFFFF, dtype=np.uint32))
        rules = [[(g[b"alpha"], None), (g[b"ta"], 0)], [(g[b"ta"], None), (g[b"gamma"], 1)], [(g[b"beta"], None), (g[b"ta"], 0)]]
        m.set_flow_seq_rules(rules)
        S = m.flow_seq_rule_words
        packets = [[b"beta alp", b"gamma beta "], [b"ha  ta", b"alpha ta ga"], [b" gamma", b"mma"]]
        prog = np.zeros((2, S), dtype=np.uint64)
        st, pos = np.zeros(2, np.uint32), np.zeros(2, np.uint64)
        got = []
        for rnd in packets:
            data = np.frombuffer(b"".join(rnd), dtype=np.uint8)
            offs = np.concatenate([[0], np.cumsum([len(p) for p in rnd])]).astype(np.int64)
            ev, st, pos_out, _ = m._read_list("windows", data, offs, m.flow_seq_rules_min_len(), True, None, st, pos)
            ptr, hits = m.flow_seq_rules(ev, offs, prog, pos)
            got.append([[(int(h >> np.uint64(24)) - int(offs[j]), int(h) & GID_MAX) for h in hits[ptr[j]:ptr[j + 1]]]
                        for j in range(2)])
            pos = pos_out
        # flow 0 = "beta alpha  ta gamma": alpha ends at 9, ta at 13 (round 2, byte 5), gamma at 19 (round 3, byte 5);
        # the ta of beta (bytes 2-3) lies before the window, so rule 2 fires on the ta at 13 as well
        assert got[0] == [[], []]
        assert got[1][0] == [(5, 0), (5, 2)] and got[2][0] == [(5, 1)]
        # flow 1 = "gamma beta alpha ta gamma": ta of beta begins at byte 8 < 12: dropped; alpha..ta in round 2
        assert got[1][1] == [(7, 0), (7, 2)] and got[2][1] == [(2, 1)]
    finally:
        m.free()


def test_flow_table_scan_seq_rules_over_three_rounds_against_the_whole_flows():
    m = build(PATS, "auto")
    try:
        gid = gids_of(m, len(PATS))
        g = {p: int(gid[k]) for k, p in enumerate(PATS)}
        rules = [[(g[b"alpha"], None), (g[b"beta"], 0)], [(g[b"gamma"], None), (g[b"delta"], 3)], [(g[b"ta"], None)],
                 [(g[b"mma"], None), (g[b"alpha"], 0), (g[b"ta"], 2)], [(g[b"beta"], None), (g[b"beta"], 0)],
                 [(g[b"alpha"], None), (g[b"gamma"], None), (g[b"delta"], 0)]]
        m.set_flow_seq_rules(rules)
        m.set_seq_rules(rules)
        assert m.flow_seq_rules_min_len() == 2
        flows = pm.FlowTable(m)
        rounds = [
            [("a", b"..alp"), ("b", b"beta gam"), ("c", b"delta")],
            [("a", b"ha be"), ("c", b" gamma beta"), ("d", b"gamma delta")],  # b pauses; alpha straddles in a
            [("b", b"ma alpha beta"), ("a", b"ta gamma  delta"), ("c", b"alpha   delta beta"), ("d", b"")],
        ]
        text, got = {}, {}
        for packets in rounds:
            out = flows.scan_seq_rules(packets)
            assert len(out) == len(packets)
            for (k, data), (pos, rule) in zip(packets, out):
                before = len(text.get(k, b""))
                text[k] = text.get(k, b"") + data
                got.setdefault(k, []).extend(zip((pos + before).tolist(), rule.tolist()))
                assert flows.bytes[k] == flows.seq_rule_bytes[k] == len(text[k])
        keys = sorted(text)
        whole = m.read_many_seq_rules([text[k] for k in keys])
        fired = 0
        for k, (pos, rule) in zip(keys, whole):
            assert sorted(got[k]) == sorted(zip(pos.tolist(), rule.tolist())), k
            fired += len(pos)
        assert fired >= 8 and len(flows) == 4
        assert flows.scan_seq_rules([]) == []
        flows.end("a")
        assert "a" not in flows.seq_rule_rows and "a" not in flows.seq_rule_bytes
        out = flows.scan_seq_rules([("a", b"ta")])
        assert out[0][1].tolist() == [2]  # a fresh flow: [ta] fires again
        # a flow that another scan method fed since (no dictionary file here: a gid is its own code)
        m._codes = np.arange(len(PATS) + 1, dtype=np.uint32)
        flows.scan([("b", b"xyz")])
        with pytest.raises(ValueError, match="scan_seq_rules"):
            flows.scan_seq_rules([("b", b"alpha")])
        flows.seq_rule_rows["c"] = np.zeros(m.flow_seq_rule_words + 1, dtype=np.uint64)
        with pytest.raises(ValueError, match="words"):
            flows.scan_seq_rules([("c", b"alpha")])
    finally:
        m.free()


def test_host_form_equals_the_twin():
    m, plen = own_matcher()
    rng = np.random.default_rng(41)
    gids = np.arange(1, 90)
    rules = [[(int(g), None)] for g in gids] * 6 + random_seq_rules(rng, 300, gids.tolist(), max_gap=30)
    m.set_flow_seq_rules(rules)
    S = m.flow_seq_rule_words
    nseg, nrows = 200, 230
    dev, host = np.zeros((nrows, S), dtype=np.uint64), np.zeros((nrows, S), dtype=np.uint64)
    had = np.zeros(nrows, dtype=np.uint64)
    for call in range(3):
        offs = random_offsets(rng, nseg)
        events = pack(rng.integers(offs[0], offs[-1] + 1, size=3000), rng.choice(gids, size=3000))
        rows = np.arange(nseg) if call == 0 else rng.permutation(nrows)[:nseg].astype(np.int64)
        keep = call == 1
        before = dev.copy()
        pos_in = had[rows]
        ptr, hits = m.flow_seq_rules(events, offs, dev, pos_in, None if call == 0 else rows, keep=keep)
        exp_ptr, exp_hits = pm.flow_seq_rules_host(events, offs, rules, plen, host, pos_in, None if call == 0 else rows,
                                                   keep=keep)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits) and np.array_equal(dev, host), call
        assert call != 0 or len(hits) > len(events)
        assert not keep or np.array_equal(dev, before)
        if not keep:
            had[rows] += np.diff(offs).astype(np.uint64)
    # hits_cap short on the host form: rule_ptr complete, the first hits_cap of the sorted ranges, the rows committed
    offs = random_offsets(rng, nseg)
    events = pack(rng.integers(offs[0], offs[-1] + 1, size=500), rng.choice(gids, size=500))
    pos_in = had[:nseg].copy()
    fresh_dev, fresh_host = np.zeros_like(dev), np.zeros_like(host)
    exp_ptr, exp_hits = pm.flow_seq_rules_host(events, offs, rules, plen, fresh_host, pos_in)
    out, rp = np.full(10 + 8, POISON64, np.uint64), np.zeros(len(offs), np.int64)
    assert m.lib.pm_hip_flow_seq_rules(m.obj, events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p), nseg,
                                       fresh_dev.ctypes.data_as(u64p), nrows, None, pos_in.ctypes.data_as(u64p), 0,
                                       out.ctypes.data_as(u64p), 10, rp.ctypes.data_as(i64p)) == 0
    assert len(exp_hits) > 10 and np.array_equal(rp, exp_ptr) and np.array_equal(out[:10], exp_hits[:10])
    assert np.all(out[10:] == POISON64) and np.array_equal(fresh_dev, fresh_host)
    p0, h0 = m.flow_seq_rules(np.empty(0, np.uint64), offs, dev, pos_in)
    assert not p0.any() and len(p0) == len(offs) and len(h0) == 0 and np.array_equal(dev, host)
    with pytest.raises(ValueError, match="words"):
        m.flow_seq_rules(events, offs, np.zeros((nrows, S + 1), dtype=np.uint64), pos_in)


def test_captured_alone_behind_a_fixed_list_buffer_and_replayed():
    """The call captured alone in a graph behind a fixed list buffer and
    replayed over list A, then, with the buffer, its cursor and the byte
    counts rewritten, over list B: hits and rows after each replay equal the
    twin's two calls."""
    torch = _torch()
    rng = np.random.default_rng(27)
    rules = random_seq_rules(rng, 200, range(1, 25), max_pos=3, max_gap=20)
    offs = random_offsets(rng, 300)
    lists = [pack(rng.integers(offs[0], offs[-1], size=n), rng.integers(1, 26, size=n)) for n in (2500, 1800)]
    nseg, cap = len(offs) - 1, 3000
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        plen = np.array([m.pattern_len(g) for g in range(30)], dtype=np.uint32)
        m.set_flow_seq_rules(rules)
        host = np.zeros((nseg, m.flow_seq_rule_words), dtype=np.uint64)
        d_prog = Sets(torch, host)
        d_offs = _dev(torch, offs)
        d_pos = _u64(torch, np.zeros(nseg, np.uint64))
        ev = Ev(torch, cap)
        o = Out(torch, m, cap, nseg, 20000)
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            _call(m, torch, ev, d_offs, nseg, d_prog, nseg, None, d_pos, 0, o, stream=st.cuda_stream)
        torch.cuda.synchronize()
        assert o.untouched() and not d_prog.get().any()  # captured, not run
        totals = []
        pos_in = np.zeros(nseg, dtype=np.uint64)
        for replay, lst in enumerate(lists):
            ev.buf[:len(lst)] = torch.from_numpy(lst.view(np.int64).copy()).cuda()
            ev.nev.fill_(len(lst))
            d_pos.copy_(torch.from_numpy(pos_in.view(np.int64).copy()).cuda().view(d_pos.dtype))
            o.hits[:o.hits_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            exp_ptr, exp_hits = pm.flow_seq_rules_host(lst, offs, rules, plen, host, pos_in)
            ptr, hits = o.result()
            assert 0 < exp_ptr[-1] <= o.hits_cap, replay
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, f"replay {replay}")
            assert np.all(hits[ptr[-1]:] == POISON64)
            assert np.array_equal(d_prog.get(), host), replay
            totals.append(int(ptr[-1]))
            pos_in = pos_in + np.diff(offs).astype(np.uint64)
        assert totals[0] != totals[1]
    finally:
        m.free()


def test_call_between_served_read_blocks():
    """Small read_block calls of an rt object go to its resident server grid;
    a flow ordered-rules call after every third asks the grid to leave the
    device first, like every device launch, and the next small call launches
    it again: the gids equal one large call's, every result the twin's."""
    m = fresh_matcher("snort", "rt")
    try:
        plen = np.array([m.pattern_len(g) for g in range(10)], dtype=np.uint32)
        assert np.all(plen[1:8] > 0)
        sizes = [100 << 10] * 9
        text = np.tile(SHIP, 1 + sum(sizes) // len(SHIP))[:sum(sizes)]
        cuts = np.cumsum([0] + sizes)
        m.reset()
        whole = m.read_block_gids(text)  # > 256 Ki positions: the pipeline, not the server
        m.reset()
        s0 = m.serve_stats()
        rng = np.random.default_rng(28)
        offs = np.concatenate([[3], 3 + np.cumsum(rng.integers(0, 30, size=300))]).astype(np.int64)
        rules = random_seq_rules(rng, 50, range(1, 7))
        f = SeqFlows(rules, 300, m=m, plen=plen)
        parts, had = [], np.zeros(300, dtype=np.uint64)
        for k, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
            parts.append(m.read_block_gids(text[a:b]))
            if k % 3 == 2:
                events = pack(rng.integers(0, offs[-1] + 10, size=600), rng.integers(1, 6, size=600))
                ptr, _ = f.call(events, offs, had, what=f"after block {k}")
                had += np.diff(offs).astype(np.uint64)
                assert ptr[-1] > 0 or k > 2
        assert np.array_equal(np.concatenate(parts), whole)
        s1 = m.serve_stats()
        assert s1["calls"] - s0["calls"] == len(sizes)
        assert s1["launches"] - s0["launches"] >= 3  # the first call, and the call after each stop
    finally:
        m.free()
