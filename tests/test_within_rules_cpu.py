"""Within (an upper bound on an ordered rule's link) without a device
(include/pm_hip.h "ordered rules", within): the host twin
pm_flat_seq_rules_by_stream_within and pm_flat_seq_rule_tables_within against
the all-pairs reference and the exhaustive search of within_rule_inputs.py,
the rejected rule sets, and the packers."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from rule_inputs import random_offsets
from seq_rule_inputs import FREE, NEGATED, pack, random_seq_rules, seq_csr, stream_occurrences
from within_rule_inputs import (KINDS, exhaustive, fuzz_case, fuzz_counts, kinds_shown, planted_case,
                                reference_within_rules, with_bounds, within_csr)

POISON64 = 0xA5A5A5A5A5A5A5A5
PTR_POISON = -0x5A5A5A5A5A5A5A5B
P32 = 0xA5A5A5A5
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))
FUZZ_SEEDS = range(6)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def twin_raw(events, offs, raw, plen, hits_cap, guard=8):
    """pm_flat_seq_rules_by_stream_within on poisoned outputs: (rc, rule_ptr with guard, hits with guard)."""
    tptr, terms, gaps, withins = raw
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    plen = np.ascontiguousarray(plen, dtype=np.uint32)
    hits = np.full(hits_cap + guard, POISON64, np.uint64)
    ptr = np.full(len(offs) + guard, PTR_POISON, np.int64)
    rc = pm.load().pm_flat_seq_rules_by_stream_within(_p(events, u64p), len(events), _p(offs, i64p), len(offs) - 1,
                                                      _p(tptr, u32p), _p(terms, u32p), _p(gaps, u32p),
                                                      _p(withins, u32p), len(tptr) - 1, _p(plen, u32p), len(plen) - 1,
                                                      _p(hits, u64p), hits_cap, _p(ptr, i64p))
    return rc, ptr, hits


def tables(raw, plen):
    """pm_flat_seq_rule_tables_within on poisoned outputs: (rc, anchor_ptr, anchor_rules, anchor_term)."""
    tptr, terms, gaps, withins = raw
    plen = np.ascontiguousarray(plen, dtype=np.uint32)
    n = len(tptr) - 1
    aptr = np.full(len(plen) + 1, P32, np.uint32)
    arules = np.full(max(n, 1), P32, np.uint32)
    aterm = np.full(max(n, 1), P32, np.uint32)
    rc = pm.load().pm_flat_seq_rule_tables_within(_p(tptr, u32p), _p(terms, u32p), _p(gaps, u32p), _p(withins, u32p),
                                                  n, _p(plen, u32p), len(plen) - 1, _p(aptr, u32p), _p(arules, u32p),
                                                  _p(aterm, u32p))
    return rc, aptr, arules, aterm


def check(events, offs, rules, plen):
    """The twin == the reference; returns them."""
    exp_ptr, exp_hits = reference_within_rules(events, offs, rules, plen)
    ptr, hits = pm.seq_rules_by_stream_host(events, offs, rules, plen)
    assert np.array_equal(ptr, exp_ptr), (ptr, exp_ptr)
    assert np.array_equal(hits, exp_hits)
    return ptr, hits


@pytest.mark.parametrize("seed", range(8))
def test_planted_kinds_are_in_every_case_and_the_twin_is_the_reference(seed):
    events, offs, rules, plen, plan = planted_case(seed)
    assert set(plan) == set(KINDS)
    seen = kinds_shown(events, offs, rules, plen, plan)  # on the references alone
    assert all(seen.values()), seen
    ptr, hits = check(events, offs, rules, plen)
    # the packed form, and the order of the list and further duplicates change nothing
    again = pm.seq_rules_by_stream_host(np.sort(np.concatenate([events, events[::2]])), offs, within_csr(rules), plen)
    assert np.array_equal(again[0], ptr) and np.array_equal(again[1], hits)


_fuzz = {}


def fuzz(seed):
    """The fuzz case of a seed and its reference, computed once."""
    if seed not in _fuzz:
        case = fuzz_case(seed, scale=0.2)
        _fuzz[seed] = (case, reference_within_rules(*case))
    return _fuzz[seed]


def test_the_fuzz_inputs_meet_the_condition():
    """On the reference alone, summed over the seeds: at least 500 (stream,
    rule) pairs where the reference fires and greedy_with_check does not, 200
    where it fires later than the distance-only reference, 100 that the bound
    kills."""
    total = np.zeros(3, dtype=np.int64)
    for seed in FUZZ_SEEDS:
        total += np.array(fuzz_counts(*fuzz(seed)[0]))
    print("rescued, later, killed:", total.tolist())
    assert total[0] >= 500 and total[1] >= 200 and total[2] >= 100, total.tolist()


@pytest.mark.parametrize("seed", FUZZ_SEEDS)
def test_fuzz_the_twin_is_the_reference(seed):
    (events, offs, rules, plen), (exp_ptr, exp_hits) = fuzz(seed)
    ptr, hits = pm.seq_rules_by_stream_host(events, offs, rules, plen)
    assert exp_ptr[-1] > 0 and np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)


@pytest.mark.parametrize("seed", range(4))
def test_the_twin_is_the_exhaustive_search_on_tiny_streams(seed):
    rng = np.random.default_rng(900 + seed)
    nseg = 120
    offs = random_offsets(rng, nseg, max_len=60)
    ngid = 4
    plen = np.concatenate([[0], rng.integers(1, 5, size=ngid)]).astype(np.uint32)
    n = 700
    events = pack(rng.integers(int(offs[0]), int(offs[-1]), size=n), rng.integers(1, ngid + 1, size=n))
    rules = with_bounds(rng, random_seq_rules(rng, 60, range(1, ngid + 1), max_pos=4, follow=0.85, max_gap=6), plen,
                        share=0.8, slack=12)
    ptr, hits = pm.seq_rules_by_stream_host(events, offs, rules, plen)
    got = {}
    for s in range(nseg):
        for h in hits[ptr[s]:ptr[s + 1]].tolist():
            got[(s, h & 0xFFFFFF)] = h >> 24
    occ = stream_occurrences(events, offs)
    tried = fired = 0
    for s in sorted(occ):
        for r, rule in enumerate(rules):
            want = exhaustive(occ[s], rule, plen)
            if want == "skip":
                continue
            tried += 1
            fired += want is not None
            assert got.get((s, r)) == want, (s, r, rule)
    assert tried > 2000 and fired > 200


@pytest.mark.parametrize("seed", range(3))
def test_every_within_free_is_the_existing_twin(seed):
    rng = np.random.default_rng(950 + seed)
    offs = random_offsets(rng, 200, max_len=150)
    events = pack(rng.integers(max(int(offs[0]) - 9, 0), offs[-1] + 9, size=4000), rng.integers(1, 7, size=4000))
    plen = np.concatenate([[0], rng.integers(1, 7, size=8)]).astype(np.uint32)
    rules = random_seq_rules(rng, 150, np.arange(1, 9), max_gap=12)
    old = pm.seq_rules_by_stream_host(events, offs, seq_csr(rules), plen)
    tptr, terms, gaps = seq_csr(rules)
    new = pm.seq_rules_by_stream_host(events, offs, (tptr, terms, gaps, np.full(len(terms), FREE, np.uint32)), plen)
    assert old[0][-1] > 0 and np.array_equal(old[0], new[0]) and np.array_equal(old[1], new[1])
    rc, ptr, hits = twin_raw(events, offs, (tptr, terms, gaps, None), plen, len(old[1]))  # NULL withins: all free
    assert rc == 0 and np.array_equal(ptr[:len(offs)], old[0]) and np.array_equal(hits[:len(old[1])], old[1])
    a, b = tables((tptr, terms, gaps, None), plen), pm.load().pm_flat_seq_rule_tables
    aptr, arules, aterm = (np.zeros_like(x) for x in a[1:])
    assert a[0] == 0 and b(_p(tptr, u32p), _p(terms, u32p), _p(gaps, u32p), len(tptr) - 1, _p(plen, u32p),
                           len(plen) - 1, _p(aptr, u32p), _p(arules, u32p), _p(aterm, u32p)) == 0
    assert np.array_equal(a[1], aptr) and np.array_equal(a[2], arules) and np.array_equal(a[3], aterm)


def bad_within_rule_sets(L=3):
    """(name, (term_ptr, terms, gaps, withins)) of every -2 case of
    pm_hip_set_seq_rules_within that the bounds add, where pattern 2 has L bytes."""
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    good = within_csr([[(1, None), (2, 0, L)]])
    return [
        ("a within on a free term", (u32(0, 2), u32(1, 2), u32(FREE, FREE), u32(FREE, 5))),
        ("a within on the first positive term", (u32(0, 2), u32(1, 2), u32(FREE, 0), u32(9, 9))),
        ("a within on a negated term", (u32(0, 3), u32(1, 2, 3 | NEGATED), u32(FREE, 0, FREE), u32(FREE, 9, 9))),
        ("a within below d + L", (u32(0, 2), u32(1, 2), u32(FREE, 4), u32(FREE, 4 + L - 1))),
        ("a within of 0 on a follower", (u32(0, 2), u32(1, 2), u32(FREE, 0), u32(FREE, 0))),
        ("a within of 0x80000000", (u32(0, 2), u32(1, 2), u32(FREE, 0), u32(FREE, 0x80000000))),
        ("a within of 0xFFFFFFFE", (u32(0, 2), u32(1, 2), u32(FREE, 0), u32(FREE, 0xFFFFFFFE))),
        ("a distance that leaves no room below 0x7FFFFFFF", (u32(0, 2), u32(1, 2), u32(FREE, 0x7FFFFFFF),
                                                              u32(FREE, 0x7FFFFFFF))),
        ("NULL gaps beside withins", (good[0], good[1], None, good[3])),
    ]


def test_every_bad_rule_set_is_minus_2_with_nothing_written():
    events = pack([1, 2, 3], [1, 2, 3])
    plen = np.concatenate([[0], np.full(70, 3)]).astype(np.uint32)
    for name, raw in bad_within_rule_sets():
        rc, ptr, hits = twin_raw(events, [0, 10], raw, plen, 4)
        assert rc == -2 and np.all(ptr == PTR_POISON) and np.all(hits == POISON64), name
        rc, aptr, arules, aterm = tables(raw, plen)
        assert rc == -2, name
        assert np.all(aptr == P32) and np.all(arules == P32) and np.all(aterm == P32), name
    # the ordered rules' own bad sets stay bad beside free bounds
    from test_seq_rules_cpu import bad_seq_rule_sets
    for name, (tptr, terms, gaps), nrules in bad_seq_rule_sets():
        if nrules is not None or tptr is None or terms is None:
            continue
        raw = (tptr, terms, gaps, np.full(max(len(terms), 1), FREE, np.uint32))
        assert twin_raw(events, [0, 10], raw, plen, 4)[0] == -2 and tables(raw, plen)[0] == -2, name
    # what is accepted: w == d + L, the largest bound, a bound behind a negated term, A ... A within
    ok = within_csr([[(1, None), (2, 4, 7), (-3, None), (4, 0, 0x7FFFFFFF), (1, 0, 3), (5, None), (6, None, 3)]])
    assert tables(ok, plen)[0] == 0 and twin_raw(events, [0, 10], ok, plen, 4)[0] == 0


def test_hand_case():
    """L = 3 for every pattern.  A ends at 12 and 30, B at 15, 20 and 40.
    within 3 (== L) takes the B at 15 only; distance 2 within 8 the B at 20 (12
    + 5 <= 20 <= 12 + 8); distance 5 within 9 none from 12 (needs 20 <= p <=
    21: 20) -- it is 20; within 6 from 30 needs 33..36: none, from 12 15..18:
    15; A ... A within 18 takes 30, within 17 nothing."""
    plen = [0, 3, 3, 3]
    events = pack([12, 30, 15, 20, 40], [1, 1, 2, 2, 2])
    rules = [[(1, None), (2, 0, 3)], [(1, None), (2, 2, 8)], [(1, None), (2, 5, 9)], [(1, None), (2, None, 6)],
             [(1, None), (1, 0, 18)], [(1, None), (1, 0, 17)], [(1, None), (2, 7, 10)], [(1, None), (2, 6, 10)]]
    ptr, hits = check(events, [10, 50], rules, plen)
    pos, rule = pm.unpack_events(hits)
    # rule 6: 12 + 10 <= p <= 22: none; 30 + 10 = 40 <= p <= 40: the B at 40.  rule 7: 21..22 none; 39..40: 40
    assert sorted(zip(rule.tolist(), pos.tolist())) == [(0, 15), (1, 20), (2, 20), (3, 15), (4, 30), (6, 40), (7, 40)]


def test_packers():
    rules = [[(1, None), (-3, None), (2, 0, 9)], [(4, None), (4, 9), (5, None, 7)]]
    ptr, terms, gaps, withins = pm.pack_seq_rules_within(rules, fast=[2, 4])
    assert ptr.tolist() == [0, 3, 6] and gaps.tolist() == [FREE, FREE, 0, FREE, 9, 0]  # a bare within: gap 0
    assert withins.tolist() == [FREE, FREE, 9, FREE, FREE, 7]
    assert terms.tolist() == [1, 3 | NEGATED, 2 | (1 << 30), 4 | (1 << 30), 4, 5]
    assert all(a.dtype == np.uint32 for a in (ptr, terms, gaps, withins))
    for a, b in zip(pm.pack_seq_rules_within(rules), within_csr(rules)):
        assert np.array_equal(a, b)
    with pytest.raises(ValueError):
        pm.pack_seq_rules(rules)  # a term carries a within
    plain = [[(1, None), (2, 3)]]
    assert [a.tolist() for a in pm.pack_seq_rules_within(plain)[:3]] == [a.tolist() for a in pm.pack_seq_rules(plain)]
    assert pm.pack_seq_rules_within(plain)[3].tolist() == [FREE, FREE]
    for bad in ([[(1, None), (2, 0, -1)]], [[(1, None), (2, 0, 0x80000000)]], [[(1, None, 3, 4)]]):
        with pytest.raises(ValueError):
            pm.pack_seq_rules_within(bad)
    # a tuple of three or four rules is a sequence of rules, not the packed form
    three = ([(1, None), (2, 0, 9)], [(2, None)], [(1, None), (2, 3)])
    ev = pack([12, 20, 40], [1, 2, 2])
    a = pm.seq_rules_by_stream_host(ev, [10, 50], three, [0, 3, 3])
    b = pm.seq_rules_by_stream_host(ev, [10, 50], list(three), [0, 3, 3])
    assert a[0][-1] == 3 and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    with pytest.raises(ValueError):  # the library's check: below d + L
        pm.seq_rules_by_stream_host(pack([1], [1]), [0, 10], [[(1, None), (2, 4, 6)]], [0, 3, 3])
