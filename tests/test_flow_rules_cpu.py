"""The flow rules' host side (pm_flat_flow_rules, pm_flat_flow_rule_bits,
pm_hip_flow_rules_scratch_bytes; include/pm_hip.h "flow rules") without a
device: the twin against the dict-and-set reference of flow_rule_inputs.py over
seeded flows cut into calls, the bit numbering, the word edges, cut
invariance, PM_FLOW_RULES_KEEP and every -2 case.  The twin's outputs carry
poisoned guard slots past their end."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from flow_rule_inputs import (NO_BIT, flow_case, kinds_of_case, pack, reference_flow_rules, rule_bits, sets_array,
                              words_of)
from rule_inputs import GID_BITS, csr, random_rules
from test_rules_cpu import bad_rule_sets

u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))
POISON64 = np.uint64(0xDEADBEEFCAFEF00D)
PTR_POISON = np.int64(-0x5A5A5A5A5A5A5A5B)
GUARD = 8
SEEDS = range(8)


def twin_raw(events, offs, tptr, terms, sets, rows, flags, hits_cap, nrules=None, words=None, nrows=None):
    """pm_flat_flow_rules with hits_cap slots in front of guards: (rc,
    rule_ptr with its guard, hits with theirs).  sets is updated in place."""
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    ptr = np.full(nseg + 1 + GUARD, PTR_POISON, dtype=np.int64)
    hits = np.full(hits_cap + GUARD, POISON64, dtype=np.uint64)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    rc = pm.load().pm_flat_flow_rules(
        events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p), nseg,
        None if tptr is None else tptr.ctypes.data_as(u32p), None if terms is None else terms.ctypes.data_as(u32p),
        (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules,
        None if sets is None else sets.ctypes.data_as(u64p), (0 if sets is None else sets.shape[0]) if nrows is None else nrows,
        (1 if sets is None else sets.shape[1]) if words is None else words,
        None if rows is None else rows.ctypes.data_as(i64p), flags, hits.ctypes.data_as(u64p), hits_cap,
        ptr.ctypes.data_as(i64p))
    return rc, ptr, hits


def twin(events, offs, rules, sets, rows=None, keep=False):
    """The twin with room for exactly the reference's hits -- counted by a
    KEEP call, which must leave the sets alone -- and its guards checked."""
    tptr, terms = csr(rules)
    before = sets.copy()
    rc, ptr, _ = twin_raw(events, offs, tptr, terms, sets, rows, pm.FLOW_RULES_KEEP, 0)
    assert rc == 0 and np.array_equal(sets, before)
    nseg = len(offs) - 1
    total = int(ptr[nseg])
    rc, ptr2, hits = twin_raw(events, offs, tptr, terms, sets, rows, pm.FLOW_RULES_KEEP if keep else 0, total)
    assert rc == 0 and np.array_equal(ptr2, ptr)
    assert np.all(ptr2[nseg + 1:] == PTR_POISON) and np.all(hits[total:] == POISON64)
    return ptr2[:nseg + 1], hits[:total]


_cases = {}


def seeded(seed):
    """(case, kinds, the reference's per-call results), computed once."""
    if seed not in _cases:
        case = flow_case(seed)
        _cases[seed] = (case, *kinds_of_case(case))
    return _cases[seed]


# ---- the reference alone: every seeded case holds every kind of hit -----------------------
@pytest.mark.parametrize("kind", ["all_new_later", "carried_positive", "carried_negation", "negation_after", "tie",
                                  "negation_next_call"])
def test_every_seeded_case_holds(kind):
    """(a) all positives new in a call after the first; (b) a positive
    carried; (c) suppressed by a carried negated term while its positives
    complete; (d) suppressed by a negated term behind the completing byte in
    the same call; (e) two new positive terms at one first position; (f) a hit
    whose negated term first appears in a later call."""
    for seed in SEEDS:
        assert seeded(seed)[1][kind] >= 1, (seed, kind)


# ---- twin = reference ------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS)
def test_twin_equals_reference(seed):
    case, _, results = seeded(seed)
    rules, nrows = case["rules"], case["nrows"]
    sets = np.zeros((nrows, words_of(rules)), dtype=np.uint64)
    assert len(case["calls"]) == 5 and len(case["calls"][2]["events"]) == 0
    assert any(np.any(np.diff(c["offsets"]) == 0) for c in case["calls"])  # empty streams
    untouched = sorted(set(range(nrows)) - set(case["row_of"].tolist()))
    for c, (call, (exp_ptr, exp_hits, exp_sets)) in enumerate(zip(case["calls"], results)):
        ptr, hits = twin(call["events"], call["offsets"], rules, sets, call["rows"])
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits), (seed, c)
        assert np.array_equal(sets, exp_sets), (seed, c)
        # the inert streams (rows -1 and past nrows) hold events and report nothing
        assert ptr[-1] == ptr[-3] or c == 2
    assert len(untouched) == 3 and not sets[untouched].any()
    # through the package's wrapper
    sets2 = np.zeros_like(sets)
    for call, (exp_ptr, exp_hits, exp_sets) in zip(case["calls"], results):
        ptr, hits = pm.flow_rules_host(call["events"], call["offsets"], rules, sets2, call["rows"])
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits) and np.array_equal(sets2, exp_sets)


def test_identity_rows_need_a_row_per_stream():
    rules = [[1, 2], [2, -3], [3]]
    sets = np.zeros((3, 1), dtype=np.uint64)
    carried = {}
    for events, offs in ((pack([5, 12, 25], [1, 3, 2]), [0, 10, 20, 30]), (pack([7, 13, 23], [2, 2, 1]), [0, 10, 20, 30])):
        ptr, hits = twin(events, offs, rules, sets)
        exp = reference_flow_rules(events, offs, rules, carried, 3)
        assert np.array_equal(ptr, exp[0]) and np.array_equal(hits, exp[1])
    # flow 0 carries 1; [2, -3] is suppressed in flow 1, which carries 3; flow 2 carries 2
    assert hits.tolist() == [(7 << 24) | 0, (7 << 24) | 1, (23 << 24) | 0]
    assert np.array_equal(sets, sets_array(carried, rules, 3))
    tptr, terms = csr(rules)
    rc, ptr, hits = twin_raw(events, offs, tptr, terms, sets[:2].copy(), None, 0, 4)
    assert rc == -2 and np.all(ptr == PTR_POISON) and np.all(hits == POISON64)


# ---- the bit numbering ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(4))
def test_flow_rule_bits_are_the_ranks_of_the_sorted_unique_gids(seed):
    rng = np.random.default_rng(300 + seed)
    npat = 5000
    rules = random_rules(rng, int(rng.integers(1, 400)), rng.choice(np.arange(1, npat + 1), size=300, replace=False))
    bits, k = pm.flow_rule_bits_host(rules, npat)
    gids = np.unique(np.abs(np.concatenate([np.array(r) for r in rules])))
    assert k == len(gids) and len(bits) == npat + 1
    assert np.array_equal(np.nonzero(bits != NO_BIT)[0], gids) and np.array_equal(bits[gids], np.arange(len(gids)))
    assert {int(g): int(bits[g]) for g in gids} == rule_bits(rules)


def test_flow_rule_bits_bad_arguments_write_nothing():
    lib = pm.load()
    out, k = np.full(71, 0xA5A5A5A5, np.uint32), ctypes.c_uint32(0xA5A5A5A5)

    def call(tptr, terms, nrules, npat=70, out_p=out.ctypes.data_as(u32p), k_p=ctypes.byref(k)):
        return lib.pm_flat_flow_rule_bits(None if tptr is None else tptr.ctypes.data_as(u32p),
                                          None if terms is None else terms.ctypes.data_as(u32p), nrules, npat, out_p, k_p)
    for name, tptr, terms, nrules in bad_rule_sets():
        n = (len(tptr) - 1 if tptr is not None else 1) if nrules is None else nrules
        assert call(tptr, terms, n) == -2, name
    good = csr([[1, 70]])
    assert call(*csr([[1, 71]]), 1) == -2 and call(*csr([[0, 1]]), 1) == -2  # a gid outside [1, npat]
    assert call(*good, 1, npat=1 << 24) == -2 and call(*good, 1, out_p=None) == -2 and call(*good, 1, k_p=None) == -2
    assert np.all(out == 0xA5A5A5A5) and k.value == 0xA5A5A5A5
    assert call(*good, 1) == 0 and k.value == 2 and out[1] == 0 and out[70] == 1 and np.all(out[2:70] == NO_BIT)


# ---- the word edges ------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 64, 65, 128])
def test_word_edges_and_garbage_above_k(k):
    """K term gids 10, 20, ..: the last bits of the words carry terms (63 and
    64 where they exist), every bit at or above K is set in every row before
    the first call, changes nothing and survives."""
    gids = [10 * (b + 1) for b in range(k)]
    rules = [[gids[0]]] if k == 1 else [[gids[b], gids[b + 1]] for b in range(k - 1)] + [[gids[-1], -gids[0]], [gids[-1]]]
    W = max(1, (k + 63) // 64)
    assert words_of(rules) == W and rule_bits(rules)[gids[-1]] == k - 1
    garbage = np.zeros(W, dtype=np.uint64)
    for b in range(k, 64 * W):
        garbage[b >> 6] |= np.uint64(1 << (b & 63))
    assert garbage.any() or k in (64, 128)
    nrows = 3
    sets = np.tile(garbage, (nrows, 1))
    carried = {}
    rng = np.random.default_rng(k)
    fired = set()
    for call in range(3):
        offs = np.array([100, 200, 300, 400], dtype=np.int64)
        n = 3 * k
        # flow 1 gets the word-edge terms in different calls: bits 62/63 first, 64/65 next
        edge = [g for b, g in enumerate(gids) if (b & 63) in ((62, 63) if call == 0 else (0, 1))]
        events = np.concatenate([pack(rng.integers(100, 400, size=n), rng.choice(gids, size=n)),
                                 pack(250 + np.arange(len(edge)), edge)])
        ptr, hits = twin(events, offs, rules, sets)
        exp_ptr, exp_hits = reference_flow_rules(events, offs, rules, carried, nrows)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits), call
        assert np.array_equal(sets, sets_array(carried, rules, nrows) | garbage), call
        fired |= {int(h) & 0xFFFFFF for h in hits.tolist()}
    if k >= 65:
        assert 63 in fired  # rule [gids[63], gids[64]]: a term at bit 63 and one at bit 64


def test_a_rule_across_bits_63_and_64_fires_with_one_term_carried():
    gids = list(range(1, 66))
    rules = [[g] for g in gids[:63]] + [[64, 65], [65, -64]]
    bit = rule_bits(rules)
    assert bit[64] == 63 and bit[65] == 64
    sets = np.zeros((1, 2), dtype=np.uint64)
    ptr, hits = twin(pack([3], [64]), [0, 10], rules, sets)
    assert len(hits) == 0 and sets.tolist() == [[1 << 63, 0]]
    ptr, hits = twin(pack([4, 5], [65, 64]), [0, 10], rules, sets)
    assert hits.tolist() == [(4 << 24) | 63] and sets.tolist() == [[1 << 63, 1]]  # [65, -64]: 64 is carried


# ---- cut invariance ------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_cut_invariance_without_negated_terms(seed):
    """With no negated term the union over the calls of the hits, in flow
    coordinates, is what pm_flat_rules_by_stream reports over the uncut flows;
    three cuts of the same flows."""
    whole = None
    for cut_seed in range(3):
        case = flow_case(1000 + seed, negated=0.0)
        rng = np.random.default_rng(cut_seed)
        if cut_seed:  # the same flows and events, other cuts: regroup the flow events by new random cuts
            case = _recut(case, rng)
        rules, nrows = case["rules"], case["nrows"]
        if whole is None:
            lens = np.array(case["flow_len"], dtype=np.int64)
            offs = np.concatenate([[0], np.cumsum(lens)])
            ev = np.concatenate([pack(offs[f] + p, g) for f, (p, g) in enumerate(case["flow_events"])])
            ptr, hits = pm.rules_by_stream_host(ev, offs, rules)
            whole = sorted((f, int(h >> np.uint64(GID_BITS)) - int(offs[f]), int(h) & 0xFFFFFF)
                           for f in range(len(lens)) for h in hits[ptr[f]:ptr[f + 1]])
            assert len(whole) > 50
        sets = np.zeros((nrows, words_of(rules)), dtype=np.uint64)
        got = []
        for call in case["calls"]:
            ptr, hits = twin(call["events"], call["offsets"], rules, sets, call["rows"])
            for j, f in enumerate(call["flow"]):
                got += [(f, int(h >> np.uint64(GID_BITS)) - int(call["offsets"][j]) + call["base"][j], int(h) & 0xFFFFFF)
                        for h in hits[ptr[j]:ptr[j + 1]]]
        assert sorted(got) == whole, (seed, cut_seed)


def _recut(case, rng):
    """The case's flows and events in three calls at new random cuts, streams
    in flow order, rows as before."""
    nflows = len(case["flow_len"])
    cuts = [np.concatenate([[0], np.sort(rng.integers(0, L + 1, size=2)), [L]]) for L in case["flow_len"]]
    calls = []
    for c in range(3):
        lens = [int(cuts[f][c + 1] - cuts[f][c]) for f in range(nflows)]
        offs = 11 + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        parts = []
        for f, (p, g) in enumerate(case["flow_events"]):
            inside = (p >= cuts[f][c]) & (p < cuts[f][c + 1])
            parts.append(pack(offs[f] + p[inside] - cuts[f][c], g[inside]))
        calls.append(dict(events=np.concatenate(parts), offsets=offs, rows=case["row_of"].astype(np.int64),
                          flow=list(range(nflows)), base=[int(cuts[f][c]) for f in range(nflows)]))
    return dict(case, calls=calls)


# ---- KEEP ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 3])
def test_keep_reports_the_committing_calls_hits_and_a_repeat_reports_none(seed):
    case, _, results = seeded(seed)
    rules, nrows = case["rules"], case["nrows"]
    sets = np.zeros((nrows, words_of(rules)), dtype=np.uint64)
    for call, (exp_ptr, exp_hits, exp_sets) in zip(case["calls"], results):
        before = sets.copy()
        kp, kh = twin(call["events"], call["offsets"], rules, sets, call["rows"], keep=True)
        assert np.array_equal(sets, before)
        assert np.array_equal(kp, exp_ptr) and np.array_equal(kh, exp_hits)
        ptr, hits = twin(call["events"], call["offsets"], rules, sets, call["rows"])
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits) and np.array_equal(sets, exp_sets)
        again_ptr, again = twin(call["events"], call["offsets"], rules, sets, call["rows"])
        assert len(again) == 0 and not again_ptr.any() and np.array_equal(sets, exp_sets)


def test_hits_cap_short_keeps_rule_ptr_exact_and_commits():
    case, _, results = seeded(1)
    rules, nrows, call = case["rules"], case["nrows"], case["calls"][0]
    exp_ptr, exp_hits, exp_sets = results[0]
    tptr, terms = csr(rules)
    nseg = len(call["offsets"]) - 1
    for cap in (len(exp_hits) - 1, 0):
        sets = np.zeros((nrows, words_of(rules)), dtype=np.uint64)
        rc, ptr, hits = twin_raw(call["events"], call["offsets"], tptr, terms, sets, call["rows"], 0, cap)
        assert rc == 0 and np.array_equal(ptr[:nseg + 1], exp_ptr) and np.array_equal(hits[:cap], exp_hits[:cap])
        assert np.all(hits[cap:] == POISON64) and np.array_equal(sets, exp_sets)


# ---- every -2 case -------------------------------------------------------------------------------
def test_every_bad_argument_is_minus_2_with_nothing_written():
    rules = [[1, 2], [3, -4]]
    tptr, terms = csr(rules)
    events = pack([1, 12, 13], [1, 2, 3])
    offs = np.array([0, 10, 20], np.int64)
    rows = np.array([1, 0], np.int64)

    def untouched(rc, ptr, hits, sets, name):
        assert rc == -2, name
        assert np.all(ptr == PTR_POISON) and np.all(hits == POISON64) and np.all(sets == 0x77), name
    for name, bptr, bterms, nrules in bad_rule_sets():
        # (W of the good set: the rule checks come first)
        sets = np.full((2, 1), 0x77, dtype=np.uint64)
        untouched(*twin_raw(events, offs, bptr, bterms, sets, rows, 0, 4, nrules), sets, name)
    sets = np.full((2, 1), 0x77, dtype=np.uint64)
    bad = [("a flag besides KEEP", dict(flags=2)), ("a flag besides KEEP", dict(flags=1 | (1 << 31))),
           ("words not W", dict(words=2)), ("words 0", dict(words=0)), ("NULL rows and nrows < nseg", dict(rows=None, nrows=1)),
           ("nrows x W past 2^40", dict(nrows=(1 << 40) + 1))]
    for name, change in bad:
        a = dict(rows=rows, flags=0, words=None, nrows=None)
        a.update(change)
        untouched(*twin_raw(events, offs, tptr, terms, sets, a["rows"], a["flags"], 4, words=a["words"], nrows=a["nrows"]),
                  sets, name)
    untouched(*twin_raw(events, offs, tptr, terms, None, rows, 0, 4, nrows=2, words=1), sets, "NULL sets with rows")
    lib = pm.load()
    good = [events.ctypes.data_as(u64p), 3, offs.ctypes.data_as(i64p), 2, tptr.ctypes.data_as(u32p),
            terms.ctypes.data_as(u32p), 2, sets.ctypes.data_as(u64p), 2, 1, rows.ctypes.data_as(i64p), 0, None, 0, None]
    ptr, hits = np.full(3, PTR_POISON, np.int64), np.full(4, POISON64, np.uint64)
    good[14] = ptr.ctypes.data_as(i64p)
    for name, k, v in (("NULL events", 0, None), ("NULL offsets", 2, None), ("NULL rule_ptr", 14, None),
                       ("nseg 2^31", 3, 1 << 31), ("nevents past 2^40", 1, (1 << 40) + 1),
                       ("misaligned sets", 7, ctypes.cast(ctypes.c_void_p(sets.ctypes.data + 4), u64p))):
        a = list(good)
        a[k] = v
        assert lib.pm_flat_flow_rules(*a) == -2, name
    a = list(good)
    a[12], a[13] = None, 4  # hits NULL with hits_cap
    assert lib.pm_flat_flow_rules(*a) == -2
    a[12] = events.ctypes.data_as(u64p)  # hits == events
    assert lib.pm_flat_flow_rules(*a) == -2
    assert np.all(ptr == PTR_POISON) and np.all(sets == 0x77) and np.all(hits == POISON64)
    # the good call after all of them; nseg == 0 writes nothing
    sets[:] = 0
    assert lib.pm_flat_flow_rules(*good) == 0 and ptr.tolist() == [0, 0, 1] and sets.tolist() == [[2 | 4], [1]]
    a = list(good)
    a[3], a[14] = 0, None
    assert lib.pm_flat_flow_rules(*a) == 0 and sets.tolist() == [[2 | 4], [1]]


def test_scratch_bytes_is_the_rules_calls_formula():
    lib = pm.load()

    def r16(b):
        return (b + 15) // 16 * 16
    for cap in (0, 1, 32, 33, 1024, 1025, 1 << 20, 1 << 40):
        for nseg in (0, 1, 1023, 1024, 1025, (1 << 31) - 1):
            table = 64
            while table < 2 * cap:
                table *= 2
            assert lib.pm_hip_flow_rules_scratch_bytes(cap, nseg) == 16 * table + r16(8 * nseg) + r16(8 * ((nseg + 1023) // 1024))
    none = ctypes.c_size_t(-1).value
    assert lib.pm_hip_flow_rules_scratch_bytes((1 << 40) + 1, 1) == none
    assert lib.pm_hip_flow_rules_scratch_bytes(1, -1) == none and lib.pm_hip_flow_rules_scratch_bytes(1, 1 << 31) == none
