"""Rules without a device (include/pm_hip.h "rules"): the host twin
pm_flat_rules_by_stream and the inverted index pm_flat_rule_tables against
the dict-and-set reference of rule_inputs.py, and the scratch formula."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import pack
from rule_inputs import FAST, GID_MAX, NEGATED, csr, random_offsets, random_rules, reference_rules, walk_tables

POISON64 = 0xA5A5A5A5A5A5A5A5
PTR_POISON = -0x5A5A5A5A5A5A5A5B
u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))


def twin_raw(events, offs, tptr, terms, hits_cap, nrules=None, guard=8):
    """pm_flat_rules_by_stream on poisoned outputs: (rc, rule_ptr with guard, hits with guard)."""
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    hits = np.full(hits_cap + guard, POISON64, np.uint64)
    ptr = np.full(len(offs) + guard, PTR_POISON, np.int64)
    rc = pm.load().pm_flat_rules_by_stream(
        events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p), len(offs) - 1,
        None if tptr is None else tptr.ctypes.data_as(u32p), None if terms is None else terms.ctypes.data_as(u32p),
        (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules, hits.ctypes.data_as(u64p), hits_cap,
        ptr.ctypes.data_as(i64p))
    return rc, ptr, hits


def tables(rules, plen, fast=None, raw=None, nrules=None):
    """pm_flat_rule_tables on poisoned outputs: (rc, anchor_ptr, anchor_rules, anchor_term)."""
    tptr, terms = csr(rules, fast) if raw is None else raw
    plen = np.ascontiguousarray(plen, dtype=np.uint32)
    n = (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules
    aptr = np.full(len(plen) + 1, 0xA5A5A5A5, np.uint32)
    arules = np.full(max(min(n, 4096), 1), 0xA5A5A5A5, np.uint32)  # (a call that is given more rules is rejected)
    aterm = np.full(len(arules), 0xA5A5A5A5, np.uint32)
    rc = pm.load().pm_flat_rule_tables(None if tptr is None else tptr.ctypes.data_as(u32p),
                                       None if terms is None else terms.ctypes.data_as(u32p), n,
                                       plen.ctypes.data_as(u32p), len(plen) - 1, aptr.ctypes.data_as(u32p),
                                       arules.ctypes.data_as(u32p), aterm.ctypes.data_as(u32p))
    return rc, aptr, arules, aterm


def check(events, offs, rules):
    """The twin == the reference; returns them."""
    exp_ptr, exp_hits = reference_rules(events, offs, rules)
    ptr, hits = pm.rules_by_stream_host(events, offs, rules)
    assert np.array_equal(ptr, exp_ptr), (ptr, exp_ptr)
    assert np.array_equal(hits, exp_hits)
    return ptr, hits


def test_hand_case():
    """Three streams, the middle one empty.  Rule 0 fires in stream 0 at the
    first position of its later term; rule 1 misses gid 4 everywhere; rule 2 is
    killed in stream 0 by its negation and fires in stream 2, where the negated
    gid 3 is absent (it lies in stream 0 only), beside rule 0; rule 3 is one
    term."""
    offs = [10, 50, 50, 90]
    events = pack([12, 30, 20, 40, 45, 60, 70, 65], [1, 1, 2, 3, 2, 1, 2, 1])
    rules = [[1, 2], [1, 4], [2, 1, -3], [3]]
    ptr, hits = check(events, offs, rules)
    assert ptr.tolist() == [0, 2, 2, 4]
    pos, rule = pm.unpack_events(hits)
    assert list(zip(pos.tolist(), rule.tolist())) == [(20, 0), (40, 3), (70, 0), (70, 2)]


def test_anchor_independence():
    """Each positive term in turn as PM_RULE_FAST: another index, the same
    hits from a walk driven by that index, and the twin's."""
    rng = np.random.default_rng(1)
    plen = np.concatenate([[0], rng.integers(1, 9, size=30)]).astype(np.uint32)
    rules = [[1, 2, 3, -4], [2, 3], [5, 1, 2, -6, -7], [3, 2, 1]]
    offs = random_offsets(rng, 40)
    events = pack(rng.integers(offs[0], offs[-1], size=600), rng.integers(1, 8, size=600))
    exp = check(events, offs, rules)
    assert exp[0][-1] > 0
    seen = set()
    for turn in range(3):
        fast = [[g for g in rule if g > 0][turn % sum(g > 0 for g in rule)] for rule in rules]
        rc, aptr, arules, aterm = tables(rules, plen, fast)
        assert rc == 0 and aptr[0] == 0 and aptr[-1] == len(rules)
        tptr, terms = csr(rules, fast)
        assert [int(terms[k]) & GID_MAX for k in aterm] == fast
        seen.add(tuple(aptr.tolist() + arules.tolist()))
        got = walk_tables(events, offs, rules, aptr, arules)
        assert np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
        # the twin ignores PM_RULE_FAST
        ptr, hits = pm.rules_by_stream_host(events, offs, (tptr, terms))
        assert np.array_equal(ptr, exp[0]) and np.array_equal(hits, exp[1])
    assert len(seen) == 3


def test_default_anchor_is_the_longest_positive_term_ties_to_the_smaller_gid():
    plen = np.array([0, 3, 9, 9, 5, 20, 9], dtype=np.uint32)
    rules = [[1, 3, 2, -5], [4, 1], [6, 3], [1], [2, 6, 5]]
    rc, aptr, arules, aterm = tables(rules, plen)
    assert rc == 0
    tptr, terms = csr(rules)
    assert [int(terms[k]) & GID_MAX for k in aterm] == [2, 4, 3, 1, 5]  # gid 5 is negated in rule 0: never the anchor
    assert aptr.tolist() == [0, 0, 1, 2, 3, 4, 5, 5]
    assert arules.tolist() == [3, 0, 2, 1, 4]
    # PM_RULE_FAST overrides the length
    rc, aptr, arules, aterm = tables(rules, plen, [1, None, None, None, 6])
    assert rc == 0 and [int(terms[k]) & GID_MAX for k in aterm] == [1, 4, 3, 1, 6]
    assert arules[aptr[1]:aptr[2]].tolist() == [0, 3]  # ascending inside a gid's range


def test_one_gid_in_3000_rules():
    rng = np.random.default_rng(2)
    rules = [[7, int(g)] if k % 3 else [7, -int(g)] for k, g in enumerate(rng.integers(8, 40, size=3000))]
    offs = random_offsets(rng, 30, max_len=100)
    events = pack(rng.integers(offs[0], offs[-1], size=900), rng.integers(5, 40, size=900))
    ptr, _ = check(events, offs, rules)
    assert ptr[-1] > 3000
    rc, aptr, arules, _ = tables(rules, np.concatenate([[0], np.full(40, 4)]), [7] * 3000)
    assert rc == 0 and aptr[8] - aptr[7] == 3000
    got = walk_tables(events, offs, rules, aptr, arules)
    assert np.array_equal(got[0], ptr)


def test_64_terms_pass_and_65_are_rejected():
    rule64 = list(range(1, 41)) + [-g for g in range(41, 65)]
    offs = [0, 100, 200]
    events = pack(np.arange(40), np.arange(1, 41))  # all 40 positive terms in stream 0
    ptr, hits = check(events, offs, [rule64])
    assert ptr.tolist() == [0, 1, 1] and hits.tolist() == [39 << 24]
    check(np.append(events, pack([50], [64])), offs, [rule64])  # a negated one too: no hit
    plen = np.concatenate([[0], np.full(70, 3)])
    assert tables([rule64], plen)[0] == 0
    rule65 = rule64 + [-65]
    tptr, terms = csr([rule65])
    assert twin_raw(events, offs, tptr, terms, 4)[0] == -2
    assert tables([rule65], plen)[0] == -2


def test_duplicates_outside_events_and_order_change_nothing():
    rng = np.random.default_rng(3)
    offs = random_offsets(rng, 200)
    events = pack(rng.integers(offs[0], offs[-1], size=3000), rng.integers(1, 12, size=3000))
    rules = random_rules(rng, 300, np.arange(1, 14))
    ptr, hits = check(events, offs, rules)
    assert ptr[-1] > 0
    outside = pack(np.concatenate([rng.integers(0, offs[0], size=50), rng.integers(offs[-1], offs[-1] + 99, size=50)]),
                   rng.integers(1, 14, size=100))
    more = np.concatenate([events, events[::3], outside])
    rng.shuffle(more)
    ptr2, hits2 = check(more, offs, rules)
    assert np.array_equal(ptr, ptr2) and np.array_equal(hits, hits2)
    ptr3, hits3 = pm.rules_by_stream_host(np.sort(more), offs, rules)
    assert np.array_equal(ptr, ptr3) and np.array_equal(hits, hits3)


def test_positions_near_2_40_and_the_largest_gid():
    top = 1 << 40
    offs = top - np.array([9000, 5000, 5000, 1000, 0], dtype=np.int64)
    rng = np.random.default_rng(4)
    pos = np.append(top - rng.integers(1, 9100, size=2000), top - 1)
    gid = np.append(rng.choice([1, 2, GID_MAX], size=2000), GID_MAX - 1)
    rules = [[GID_MAX, 1], [GID_MAX - 1], [2, -GID_MAX], [GID_MAX - 1, GID_MAX, 1, 2]]
    ptr, hits = check(pack(pos, gid), offs, rules)
    hpos, hrule = pm.unpack_events(hits)
    assert int(hpos.max()) == top - 1 and set(hrule.tolist()) >= {0, 1, 3}


@pytest.mark.parametrize("short", ["one", "all"])
def test_hits_cap_short_keeps_rule_ptr_complete(short):
    rng = np.random.default_rng(5)
    offs = random_offsets(rng, 100)
    events = pack(rng.integers(offs[0], offs[-1], size=2000), rng.integers(1, 10, size=2000))
    rules = random_rules(rng, 100, np.arange(1, 11))
    exp_ptr, exp_hits = reference_rules(events, offs, rules)
    total = int(exp_ptr[-1])
    assert total > 10
    cap = total - 1 if short == "one" else 0
    tptr, terms = csr(rules)
    rc, ptr, hits = twin_raw(events, offs, tptr, terms, cap)
    assert rc == 0 and np.array_equal(ptr[:len(offs)], exp_ptr) and np.all(ptr[len(offs):] == PTR_POISON)
    assert np.array_equal(hits[:cap], exp_hits[:cap]) and np.all(hits[cap:] == POISON64)


def bad_rule_sets():
    """(name, term_ptr, terms, nrules or None) of every -2 case of pm_hip_set_rules
    that needs no dictionary."""
    good_ptr, good_terms = csr([[1, 2], [3, -4]])
    u32 = lambda *v: np.array(v, dtype=np.uint32)  # noqa: E731
    return [
        ("NULL term_ptr", None, good_terms, 2),
        ("NULL terms", good_ptr, None, 2),
        ("no rules", good_ptr, good_terms, 0),
        ("too many rules", good_ptr, good_terms, (1 << 24) + 1),
        ("term_ptr not from 0", u32(1, 2, 4), good_terms, None),
        ("an empty rule", u32(0, 2, 2, 4), good_terms, None),
        ("term_ptr decreasing", u32(0, 3, 2), good_terms, None),
        ("65 terms", *csr([list(range(1, 66))]), None),
        ("no positive term", *csr([[1, 2], [-3, -4]]), None),
        ("a gid twice", *csr([[1, 2, 1]]), None),
        ("a gid twice, once negated", *csr([[1, 2, -1]]), None),
        ("unknown bits", u32(0, 2), u32(1, 2 | (1 << 29)), None),
        ("unknown bits", u32(0, 2), u32(1, 2 | (1 << 24)), None),
        ("two fast terms", u32(0, 2), u32(1 | FAST, 2 | FAST), None),
        ("fast on a negated term", u32(0, 2), u32(1, 2 | FAST | NEGATED), None),
    ]


def test_every_bad_rule_set_is_minus_2_with_nothing_written():
    events = pack([1, 2, 3], [1, 2, 3])
    plen = np.concatenate([[0], np.full(70, 3)]).astype(np.uint32)
    for name, tptr, terms, nrules in bad_rule_sets():
        rc, ptr, hits = twin_raw(events, [0, 10], tptr, terms, 4, nrules)
        assert rc == -2 and np.all(ptr == PTR_POISON) and np.all(hits == POISON64), name
        rc, aptr, arules, aterm = tables(None, plen, raw=(tptr, terms), nrules=nrules)
        assert rc == -2, name
        assert np.all(aptr == 0xA5A5A5A5) and np.all(arules == 0xA5A5A5A5) and np.all(aterm == 0xA5A5A5A5), name
    # a gid that names no pattern: above npat, or of length 0 (the tables know the dictionary; the twin does not)
    for rules, lens in (([[1, 71]], plen), ([[1, 2]], np.array([0, 3, 0, 3], np.uint32)), ([[0, 1]], plen)):
        rc, aptr, arules, aterm = tables(rules, lens)
        assert rc == -2 and np.all(aptr == 0xA5A5A5A5) and np.all(arules == 0xA5A5A5A5)
    # the twin's own arguments
    tptr, terms = csr([[1, 2]])
    offs = np.array([0, 10], np.int64)
    lib = pm.load()
    args = [events.ctypes.data_as(u64p), 3, offs.ctypes.data_as(i64p), 1, tptr.ctypes.data_as(u32p),
            terms.ctypes.data_as(u32p), 1, events.ctypes.data_as(u64p), 3, offs.ctypes.data_as(i64p)]
    assert lib.pm_flat_rules_by_stream(*args) == -2  # hits == events
    for k in (0, 2, 9):
        a = list(args)
        a[7] = None
        a[8] = 0
        a[k] = None
        assert lib.pm_flat_rules_by_stream(*a) == -2, k


def test_scratch_bytes_is_the_documented_formula():
    lib = pm.load()

    def r16(b):
        return (b + 15) // 16 * 16
    for cap in (0, 1, 31, 32, 33, 1023, 1024, 1025, 1 << 20, (1 << 20) + 1, 1 << 40):
        for nseg in (0, 1, 1023, 1024, 1025, 1024 * 1024 + 1, (1 << 31) - 1):
            table = 64
            while table < 2 * cap:
                table *= 2
            assert lib.pm_hip_rules_scratch_bytes(cap, nseg) == 16 * table + r16(8 * nseg) + r16(8 * ((nseg + 1023) // 1024))
            assert lib.pm_hip_rules_scratch_bytes(cap, nseg) == lib.pm_hip_by_stream_scratch_bytes(cap, nseg, 1) - 4 * table
    none = ctypes.c_size_t(-1).value
    assert lib.pm_hip_rules_scratch_bytes((1 << 40) + 1, 1) == none
    assert lib.pm_hip_rules_scratch_bytes(1, -1) == none
    assert lib.pm_hip_rules_scratch_bytes(1, 1 << 31) == none


@pytest.mark.parametrize("seed", range(12))
def test_fuzz(seed):
    """nseg in 1..3000, stream lengths 0..40 with runs of empty streams, random
    rules over a few gids (so that rules fire) and a few that never appear."""
    rng = np.random.default_rng(100 + seed)
    nseg = int(rng.integers(1, 3001))
    offs = random_offsets(rng, nseg)
    n = int(rng.integers(0, 20000))
    ngid = int(rng.integers(2, 30))
    events = pack(rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n), rng.integers(1, ngid + 1, size=n))
    rules = random_rules(rng, int(rng.integers(1, 400)), np.arange(1, ngid + 4))
    ptr, hits = check(events, offs, rules)
    plen = np.concatenate([[0], rng.integers(1, 6, size=ngid + 3)]).astype(np.uint32)
    rc, aptr, arules, _ = tables(rules, plen)
    assert rc == 0
    got = walk_tables(events, offs, rules, aptr, arules)
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], hits)
