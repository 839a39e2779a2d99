"""The flow ordered rules' host side (pm_flat_flow_seq_rules,
pm_flat_flow_seq_rule_layout, pm_hip_flow_seq_rules_scratch_bytes;
include/pm_hip.h "flow ordered rules") without a device: the twin against the
keep-everything reference of flow_seq_rule_inputs.py over seeded flows cut into
calls, rows included; cut invariance against the ordered-rules twin over the
uncut flows; the free-gap case against the flow-rules twin; the planted kinds,
asserted on the reference alone; the layout against hand-written ones; KEEP
and every -2 case.  The twin's outputs carry poisoned guard slots."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from flow_rule_inputs import flow_case, rule_bits
from flow_seq_rule_inputs import (KINDS, NO_WORD, flow_seq_case, kinds_present, layout_of, run_reference, whole_flows)
from seq_rule_inputs import GID_BITS, GID_MAX, free_rules, seq_csr

u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))
POISON64 = np.uint64(0xDEADBEEFCAFEF00D)
PTR_POISON = np.int64(-0x5A5A5A5A5A5A5A5B)
GUARD = 8
SEEDS = range(6)


def twin_raw(events, offs, csr, plen, prog, rows, pos_in, flags, hits_cap, words=None):
    """pm_flat_flow_seq_rules with hits_cap slots in front of guards: (rc,
    rule_ptr with its guard, hits with theirs).  prog is updated in place."""
    tptr, terms, gaps = csr
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    plen = np.ascontiguousarray(plen, dtype=np.uint32)
    nseg = len(offs) - 1
    ptr = np.full(nseg + 1 + GUARD, PTR_POISON, dtype=np.int64)
    hits = np.full(hits_cap + GUARD, POISON64, dtype=np.uint64)
    rows = None if rows is None else np.ascontiguousarray(rows, dtype=np.int64)
    pos_in = None if pos_in is None else np.ascontiguousarray(pos_in, dtype=np.uint64)
    rc = pm.load().pm_flat_flow_seq_rules(
        events.ctypes.data_as(u64p), len(events), offs.ctypes.data_as(i64p), nseg, tptr.ctypes.data_as(u32p),
        terms.ctypes.data_as(u32p), None if gaps is None else gaps.ctypes.data_as(u32p), len(tptr) - 1,
        plen.ctypes.data_as(u32p), len(plen) - 1, prog.ctypes.data_as(u64p), prog.shape[0],
        prog.shape[1] if words is None else words, None if rows is None else rows.ctypes.data_as(i64p),
        None if pos_in is None else pos_in.ctypes.data_as(u64p), flags, hits.ctypes.data_as(u64p), hits_cap,
        ptr.ctypes.data_as(i64p))
    return rc, ptr, hits


def twin(events, offs, rules, plen, prog, pos_in, rows=None, keep=False):
    """The twin with room for exactly its hits -- counted by a KEEP call, which
    must leave the rows alone -- and its guards checked."""
    csr = seq_csr(rules)
    before = prog.copy()
    rc, ptr, _ = twin_raw(events, offs, csr, plen, prog, rows, pos_in, pm.FLOW_RULES_KEEP, 0)
    assert rc == 0 and np.array_equal(prog, before)
    nseg = len(offs) - 1
    total = int(ptr[nseg])
    rc, ptr2, hits = twin_raw(events, offs, csr, plen, prog, rows, pos_in, pm.FLOW_RULES_KEEP if keep else 0, total)
    assert rc == 0 and np.array_equal(ptr2, ptr)
    assert np.all(ptr2[nseg + 1:] == PTR_POISON) and np.all(hits[total:] == POISON64)
    return ptr2[:nseg + 1], hits[:total]


_cases = {}


def case_of(seed):
    """The case and the reference's per-call results, computed once."""
    if seed not in _cases:
        case = flow_seq_case(seed)
        _cases[seed] = (case, run_reference(case))
    return _cases[seed]


@pytest.mark.parametrize("seed", SEEDS)
def test_every_seeded_case_holds_every_planted_kind(seed):
    case, ref = case_of(seed)
    seen = kinds_present(case, ref)
    assert set(seen) == set(KINDS)
    assert all(seen.values()), [k for k, v in seen.items() if not v]


@pytest.mark.parametrize("seed", SEEDS)
def test_twin_matches_the_reference_rows_included(seed):
    case, ref = case_of(seed)
    S = layout_of(case["rules"])[4]
    prog = np.zeros((case["nrows"], S), dtype=np.uint64)
    for call, (ptr, hits, rows_after) in zip(case["calls"], ref):
        got_ptr, got = twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"],
                            call["rows"])
        assert np.array_equal(got_ptr, ptr)
        assert np.array_equal(got, hits)
        assert np.array_equal(prog, rows_after)


@pytest.mark.parametrize("ncalls", [2, 3])
def test_planted_kinds_in_two_and_three_calls(ncalls):
    """case_of's planted flows have four calls; here the same kinds with the
    planted flows cut into two and into three."""
    case = flow_seq_case(4, nflows=8, planted_calls=ncalls)
    ref = run_reference(case)
    seen = kinds_present(case, ref)
    assert set(seen) == set(KINDS) and all(seen.values()), seen
    S = layout_of(case["rules"])[4]
    prog = np.zeros((case["nrows"], S), dtype=np.uint64)
    for call, (ptr, hits, rows_after) in zip(case["calls"], ref):
        got_ptr, got = twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"],
                            call["rows"])
        assert np.array_equal(got_ptr, ptr) and np.array_equal(got, hits) and np.array_equal(prog, rows_after)


def test_twin_with_byte_counts_past_2_to_the_32_and_40():
    for big in ((1 << 32) - 50, (1 << 32) + 7, (1 << 40) - 120):
        case = flow_seq_case(3, nflows=6, big_base=big)
        S = layout_of(case["rules"])[4]
        prog = np.zeros((case["nrows"], S), dtype=np.uint64)
        ref = run_reference(case)
        assert all(kinds_present(case, ref).values())
        for call, (ptr, hits, rows_after) in zip(case["calls"], ref):
            got_ptr, got = twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"],
                                call["rows"])
            assert np.array_equal(got_ptr, ptr) and np.array_equal(got, hits) and np.array_equal(prog, rows_after)


def flow_hits(case, per_call):
    """{flow: sorted [(flow position, rule)]} of per-call (rule_ptr, hits)."""
    out = {}
    for call, (ptr, hits) in zip(case["calls"], per_call):
        for s, f in enumerate(call["flow"]):
            for h in hits[ptr[s]:ptr[s + 1]].tolist():
                assert f >= 0, "a hit in an inert stream"
                out.setdefault(f, []).append(((h >> GID_BITS) - int(call["offsets"][s]) + int(call["pos_in"][s]),
                                              h & GID_MAX))
    return {f: sorted(v) for f, v in out.items()}


@pytest.mark.parametrize("seed", SEEDS)
def test_cut_invariance_against_the_ordered_rules_twin_over_the_uncut_flows(seed):
    """The union over the calls of the hits, in flow coordinates, against
    pm_flat_seq_rules_by_stream over the uncut flows, for three cuts of the same
    flows.  For a rule without a negated term the two are equal.  A negated
    term that first appears in a later call retracts nothing (the contract), so
    for a rule with one the uncut hits are a subset of the cut ones, and they
    are equal again where the flow is not cut at all."""
    whole = None
    for cut_seed in range(3):
        case = flow_seq_case(seed, cut_seed=cut_seed)
        rules = case["rules"]
        plain = {r for r, rule in enumerate(rules) if all(g > 0 for g, _ in rule)}
        if whole is None:
            events, offs = whole_flows(case)
            ptr, hits = pm.seq_rules_by_stream_host(events, offs, rules, case["plen"])
            whole = {f: sorted(((h >> GID_BITS) - int(offs[f]), h & GID_MAX) for h in hits[ptr[f]:ptr[f + 1]].tolist())
                     for f in range(len(offs) - 1)}
            assert sum(1 for v in whole.values() for _, r in v if r in plain) > 20
            assert sum(1 for v in whole.values() for _, r in v if r not in plain) > 5
        S = layout_of(rules)[4]
        prog = np.zeros((case["nrows"], S), dtype=np.uint64)
        per_call = [twin(c["events"], c["offsets"], rules, case["plen"], prog, c["pos_in"], c["rows"])
                    for c in case["calls"]]
        got = flow_hits(case, per_call)
        for f, want in whole.items():
            mine = got.get(f, [])
            assert [h for h in mine if h[1] in plain] == [h for h in want if h[1] in plain], (cut_seed, f)
            assert set(want) <= set(mine), (cut_seed, f)
            if len(case["cuts"][f]) == 2:  # one call holds the whole flow
                assert mine == want, (cut_seed, f)


@pytest.mark.parametrize("seed", range(3))
def test_every_gap_free_is_the_flow_rules_twin(seed):
    case = flow_case(seed)
    rules, nrows = case["rules"], case["nrows"]
    ngid = max(abs(t) for r in rules for t in r)
    plen = np.concatenate([[0], np.full(ngid, 3)]).astype(np.uint32)
    seq = free_rules(rules)
    chain_word, bit, C, K, S = layout_of(seq)
    assert C == 0 and bit == rule_bits(rules)
    sets = np.zeros((nrows, S), dtype=np.uint64)
    prog = np.zeros((nrows, S), dtype=np.uint64)
    total = 0
    for call in case["calls"]:
        want_ptr, want = pm.flow_rules_host(call["events"], call["offsets"], rules, sets, call["rows"])
        got_ptr, got = twin(call["events"], call["offsets"], seq, plen, prog, call["base"], call["rows"])
        assert np.array_equal(got_ptr, want_ptr) and np.array_equal(got, want)
        assert np.array_equal(prog, sets)
        total += len(want)
    assert total > 0


def test_keep_reports_and_leaves_the_rows():
    case, ref = case_of(0)
    S = layout_of(case["rules"])[4]
    prog = np.zeros((case["nrows"], S), dtype=np.uint64)
    for call, (ptr, hits, rows_after) in zip(case["calls"], ref):
        before = prog.copy()
        kept = twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"], call["rows"],
                    keep=True)
        assert np.array_equal(prog, before)
        assert np.array_equal(kept[0], ptr) and np.array_equal(kept[1], hits)
        twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"], call["rows"])
        again = twin(call["events"], call["offsets"], case["rules"], case["plen"], prog, call["pos_in"], call["rows"])
        assert again[0][-1] == 0 and np.array_equal(prog, rows_after)  # after the commit: nothing


def test_a_short_hits_cap_keeps_rule_ptr_exact_and_commits():
    case, ref = case_of(1)
    S = layout_of(case["rules"])[4]
    prog = np.zeros((case["nrows"], S), dtype=np.uint64)
    call, (ptr, hits, rows_after) = case["calls"][0], ref[0]
    assert len(hits) > 3
    rc, got_ptr, got = twin_raw(call["events"], call["offsets"], seq_csr(case["rules"]), case["plen"], prog,
                                call["rows"], call["pos_in"], 0, 3)
    assert rc == 0 and np.array_equal(got_ptr[:len(ptr)], ptr) and np.all(got[3:] == POISON64)
    assert np.array_equal(prog, rows_after)


def layout(rules, plen):
    return pm.flow_seq_rule_layout_host(rules, plen)


def test_layout_against_hand_written_layouts():
    plen = np.concatenate([[0], np.full(200, 2)]).astype(np.uint32)
    # two chains in rule 0 (the second one headed behind a negated term), a one-term chain and a negation
    rules = [[(7, None), (3, 0), (-9, None), (3, 5), (4, None), (8, 1)], [(5, None)], [(6, None), (6, 2), (2, None)]]
    chain, bits, C, K, S = layout(rules, plen)
    assert chain.tolist() == [0, NO_WORD, NO_WORD, NO_WORD, 1, NO_WORD, NO_WORD, 2, NO_WORD, NO_WORD]
    assert (C, K, S) == (3, 3, 4)
    assert {g: int(b) for g, b in enumerate(bits) if b != NO_WORD} == {2: 0, 5: 1, 9: 2}
    ref_chain, ref_bit, rC, rK, rS = layout_of(rules)
    assert ref_chain == {(0, 0): 0, (0, 4): 1, (2, 0): 2} and ref_bit == {2: 0, 5: 1, 9: 2} and (rC, rK, rS) == (3, 3, 4)
    # K = 0: chains alone; C = 0 and K = 0 cannot be (a rule has a positive term), C = 0: bits alone, S >= 1
    assert layout([[(1, None), (2, 0)]], plen)[2:] == (1, 0, 1)
    assert layout([[(1, None)]], plen)[2:] == (0, 1, 1)
    # K = 64 and 65 with C = 0 and C = 1: the bits' words lie behind the chain words
    for K, words in ((64, 1), (65, 2)):
        single = [[(g, None)] for g in range(1, K + 1)]
        assert layout(single, plen)[2:] == (0, K, words)
        _, bits, C, k, S = layout(single + [[(150, None), (151, 0)]], plen)
        assert (C, k, S) == (1, K, 1 + words) and int(bits[K]) == K - 1 and int(bits[150]) == NO_WORD


def test_a_within_is_refused():
    plen = np.array([0, 2, 2], dtype=np.uint32)
    with pytest.raises(ValueError):
        pm.flow_seq_rule_layout_host([[(1, None), (2, 0, 9)]], plen)
    with pytest.raises(ValueError):
        pm.flow_seq_rules_host(np.empty(0, np.uint64), [0, 4], [[(1, None), (2, 0, 9)]], plen,
                               np.zeros((1, 1), np.uint64), [0])


def test_bad_arguments_give_minus_2_and_touch_nothing():
    plen = np.array([0, 2, 2, 3], dtype=np.uint32)
    good = seq_csr([[(1, None), (2, 0)], [(3, None), (-1, None)]])
    ev = np.array([(5 << 24) | 1], dtype=np.uint64)
    offs = np.array([0, 10], dtype=np.int64)

    def run(csr=good, prog_shape=(1, 2), rows=None, pos_in=(0,), flags=0, words=None, offs=offs):
        prog = np.full(prog_shape, 0x77, dtype=np.uint64)
        rc, ptr, hits = twin_raw(ev, offs, csr, plen, prog, rows, pos_in, flags, 4, words=words)
        untouched = np.all(prog == 0x77) and np.all(ptr == PTR_POISON) and np.all(hits == POISON64)
        return rc, untouched

    assert run()[0] == 0
    assert run(pos_in=None) == (-2, True)
    assert run(flags=2) == (-2, True)
    assert run(words=1) == (-2, True)  # not the set's S
    assert run(prog_shape=(1, 3)) == (-2, True)
    assert run(prog_shape=(0, 2)) == (-2, True)  # nrows < nseg without rows
    tptr, terms, gaps = good
    assert run(csr=(tptr, terms, None)) == (-2, True)
    bad_gap = gaps.copy()
    bad_gap[0] = 0  # a gap on the first positive term
    assert run(csr=(tptr, terms, bad_gap)) == (-2, True)
    neg_gap = gaps.copy()
    neg_gap[3] = 1  # a gap on a negated term
    assert run(csr=(tptr, terms, neg_gap)) == (-2, True)
    unknown = terms.copy()
    unknown[0] = 9  # no such pattern
    assert run(csr=(tptr, unknown, gaps)) == (-2, True)
    lay = pm.load().pm_flat_flow_seq_rule_layout
    out = np.full(8, 0x55, dtype=np.uint32)
    c = ctypes.c_uint32(0x55)
    rc = lay(tptr.ctypes.data_as(u32p), unknown.ctypes.data_as(u32p), gaps.ctypes.data_as(u32p), 2,
             plen.ctypes.data_as(u32p), 3, out.ctypes.data_as(u32p), out.ctypes.data_as(u32p), ctypes.byref(c),
             ctypes.byref(c), ctypes.byref(c))
    assert rc == -2 and np.all(out == 0x55) and c.value == 0x55


def test_scratch_bytes_is_the_ordered_rules_formula():
    lib = pm.load()
    for cap, nseg in ((0, 0), (1, 1), (1000, 7), (4097, 1025)):
        assert lib.pm_hip_flow_seq_rules_scratch_bytes(cap, nseg) == lib.pm_hip_seq_rules_scratch_bytes(cap, nseg)
    assert lib.pm_hip_flow_seq_rules_scratch_bytes((1 << 40) + 1, 1) == ctypes.c_size_t(-1).value
    assert lib.pm_hip_flow_seq_rules_scratch_bytes(1, -1) == ctypes.c_size_t(-1).value
