"""The expected values of test_text_rules.py without a device: the references
of text_rule_inputs.py (occurrences as byte ranges of the text, no pattern
length in a link) against every choice of one stream (exhaustive_seq), against
the event references of rule_inputs, seq_rule_inputs and flow_rule_inputs and
against the host twins -- three derivations of one answer, as in
test_fuzz_by_stream_cpu.py -- and the conditions on the inputs that keep the
GPU file from being vacuous.  CPU only."""
import numpy as np
import pytest

import patternmatching_amd as pm
from event_inputs import code_lengths
from flow_rule_inputs import reference_flow_rules, sets_array, words_of
from fuzz_inputs import case
from rule_inputs import reference_rules
from seq_rule_inputs import reference_seq_rules
from test_fuzz_by_stream_cpu import CASES, FORMS
from test_tables_cpu import image
from text_rule_inputs import (AA, CALL2, CASE_PAIR, FIRING, NOT_FIRING, events_of, exhaustive_seq, expected, expected_flow,
                              expected_nocase, named_streams, occurrences_by_stream, product_size, seq_positions, shown)

ALL_MATCHES = ("matches", "groups_all", "windows")
PRODUCT_CAP = 10 ** 4
CHOICES_PER_LIST = 150000  # choices spent per list before the random pairs stop
GID_MASK = np.uint64(0xFFFFFF)

# Kinds a list cannot show 32 times (A ... A: 8 times), each with what it shows: asserted, not skipped.  All are in
# seed5's group lists, which hold 295 to 389 events in 273 streams: a stream with two occurrences of one pattern
# that do not overlap is rare there (1 and 0 in call 1, 4 in call 2: the streams counted from the rows), and only
# one stream of one of the four lists holds two occurrences that share exactly one byte.
SHORT = {
    ("seed5", "a", "groups_all", "overlap"): 0, ("seed5", "a", "groups_longest", "overlap"): 0,
    ("seed5", "b", "groups_all", "overlap"): 1, ("seed5", "b", "groups_longest", "overlap"): 0,
    ("seed5", "a", "groups_all", "aa_exact"): 1, ("seed5", "a", "groups_all", "aa_plus1"): 1,
    ("seed5", "a", "groups_longest", "aa_exact"): 0, ("seed5", "a", "groups_longest", "aa_plus1"): 0,
    ("seed5", "b", "groups_all", "aa_exact"): 4, ("seed5", "b", "groups_all", "aa_plus1"): 4,
    ("seed5", "b", "groups_longest", "aa_exact"): 4, ("seed5", "b", "groups_longest", "aa_plus1"): 4,
}


def tables(name):
    """(the case, gid -> code, gid -> pattern length from the oracle's patterns)."""
    c = case(name)
    d, img, tab = image(name, pm.KIND_AC)
    tab = np.asarray(tab, dtype=np.uint32)
    cl, ll = code_lengths(name)
    plen = np.concatenate([[0], ll[np.searchsorted(cl, tab[1:])]]).astype(np.uint32)
    return c, tab, plen


def _lists(name):
    c, tab, plen = tables(name)
    for which in ("a", "b"):
        for form in FORMS:
            yield c, plen, which, form, expected(c, which, form, tab)


@pytest.mark.parametrize("name", CASES)
def test_the_ordered_reference_equals_every_choice(name):
    """seq_rules_from_text == exhaustive_seq on (stream, rule) pairs with 1 to
    10^4 choices: every planned derived rule in its own stream, then pairs in
    a fixed random order until CHOICES_PER_LIST choices are spent (a pair is
    taken as drawn, whatever its size).  All fitting pairs are 385 million
    choices in unary alone, minutes of Python.  Covered of the pairs that fit:
    unary 3,111 of 388,608 (0.8 %), seed0 3,894 of 419,152 (0.9 %), no_short
    12,664 of 384,686 (3.3 %), many 34,037 of 198,105 (17 %), seed5 52,406 of
    124,841 (42 %); 2,536 to 3,462 of them are planned rules.  At least 1,000
    pairs, 500 planned ones and 300 that fire in every case."""
    covered = fired = own = 0
    rng = np.random.default_rng(11)
    for c, plen, which, form, x in _lists(name):
        rules = x["derived"]["seq"]
        got = seq_positions(x["rows"], c.nseg, rules)
        occ = occurrences_by_stream(x["rows"])
        # every planned rule in its own stream first, whatever the budget: the by-construction cases
        planned = [(s, r) for _, s, r, _ in x["derived"]["seq_plan"] if s in occ]
        done = set(planned)
        spent = 0
        pairs = planned + [(s, r) for s in rng.permutation(sorted(occ)).tolist() for r in rng.permutation(len(rules)).tolist()]
        for k, (s, r) in enumerate(pairs):
            if k >= len(planned) and ((s, r) in done or spent >= CHOICES_PER_LIST):
                if spent >= CHOICES_PER_LIST:
                    break  # (in the order drawn: a small product is not preferred once the budget runs low)
                continue
            n = product_size(occ[s], rules[r])
            if 1 <= n <= PRODUCT_CAP:
                want = exhaustive_seq(occ[s], rules[r])
                assert got[r].get(s) == want, (name, which, form, s, rules[r])
                spent += n
                covered += 1
                fired += want is not None
                own += k < len(planned)
    print(f"{name}: {covered} pairs against every choice, {own} of them planned rules in their own streams")
    assert covered >= 1000 and fired >= 300 and own >= 500, (name, covered, fired, own)


@pytest.mark.parametrize("name", CASES)
def test_three_derivations_agree(name):
    """The text references == the event references == the host twins on the
    events made from the rows, in the order a device never gives (shuffled)."""
    rng = np.random.default_rng(9)
    for c, plen, which, form, x in _lists(name):
        what = f"{name}, text {which}, {form}"
        d = x["derived"]
        events = rng.permutation(events_of(x["rows"], c.offs, x["before"]))
        for exp, others in ((x["rules"], (reference_rules(events, c.offs, d["rules"]),
                                          pm.rules_by_stream_host(events, c.offs, d["rules"]))),
                            (x["seq"], (reference_seq_rules(events, c.offs, d["seq"], plen),
                                        pm.seq_rules_by_stream_host(events, c.offs, d["seq"], plen)))):
            assert exp[0][-1] == len(exp[1]) > 0, what
            for ptr, hits in others:
                assert np.array_equal(ptr, exp[0]) and np.array_equal(hits, exp[1]), what


@pytest.mark.parametrize("name", CASES)
def test_three_derivations_of_the_flow_rules_agree(name):
    """flow_rules_from_text (no sets) == reference_flow_rules (a dict of
    carried gids) == pm_flat_flow_rules (the twin's sets), call 1 then call 2
    on the rows of a fixed permutation."""
    c, tab, plen = tables(name)
    lens = np.diff(c.offs)
    rng = np.random.default_rng(10)
    for form in FORMS:
        f = expected_flow(c, form, tab)
        rules, rows = f["rules"], f["d_rows"]
        carried, sets = {}, np.zeros((c.nseg, words_of(rules)), dtype=np.uint64)
        for k, which in enumerate(("a", "b")):
            x = expected(c, which, form, tab)
            events = rng.permutation(events_of(x["rows"], c.offs, x["before"]))
            ref = reference_flow_rules(events, c.offs, rules, carried, c.nseg, rows)
            keep = pm.flow_rules_host(events, c.offs, rules, sets.copy(), rows, keep=True)
            twin = pm.flow_rules_host(events, c.offs, rules, sets, rows)
            for ptr, hits in (ref, keep, twin):
                assert np.array_equal(ptr, f["calls"][k][0]) and np.array_equal(hits, f["calls"][k][1]), (name, form, k)
            assert np.array_equal(sets, sets_array(carried, rules, c.nseg)), (name, form, k)
        held = {int(rows[j]): g for j, g in enumerate(f["held"]) if g}
        assert np.array_equal(sets, sets_array(held, rules, c.nseg)), (name, form)
        assert np.all(lens >= 0)


def _material(rows, nseg, before):
    """(streams with two non-overlapping occurrences of different patterns;
    streams whose earliest-ending occurrence began before the call and is
    followed by a later one), from the rows alone."""
    pairs = straddle = 0
    for s, occ in occurrences_by_stream(rows).items():
        flat = sorted((b, a, g) for g, v in occ.items() for a, b in v)  # by end
        end0, start0, g0 = flat[0]
        pairs += any(g != g0 and a >= end0 for _, a, g in flat)
        if before is not None:
            straddle += start0 < before[s] and any(a >= end0 for _, a, _ in flat[1:])
    return pairs, straddle


@pytest.mark.parametrize("name", CASES)
def test_the_lists_hold_the_material(name):
    """Conditions on the inputs, from the oracle's rows alone."""
    for c, plen, which, form, x in _lists(name):
        pairs, straddle = _material(x["rows"], c.nseg, x["before"])
        if form in ALL_MATCHES:
            assert pairs >= 60, (name, which, form, pairs)
        if which == "b":
            assert straddle >= 10, (name, form, straddle)


@pytest.mark.parametrize("name", CASES)
def test_every_list_shows_every_derived_kind(name):
    """On the text reference's result alone: of every kind at least 32 derived
    rules fire in their stream at the derived byte, or do not fire there where
    they must not (an overlap rule: not from the two occurrences that share a
    byte; it has the hit the stream's other occurrences give, mostly none); of
    the A ... A kinds and the chains whose head straddles the cut at least 8.
    The unordered and the ordered rules of a kind that has both are counted
    apart.  What a list cannot give is named in SHORT and its shortage
    asserted.  The named streams that hold anything all gave a rule."""
    for c, plen, which, form, x in _lists(name):
        d = x["derived"]
        seen = _seen(d, x, c.offs)
        assert all(ok == planned for ok, planned in seen.values()), (name, which, form, seen)
        floor = {**{k: 32 for k in FIRING + NOT_FIRING}, **{k: 8 for k in AA}}
        if which == "b":
            floor.update({k: 8 for k in CALL2})
        for kind, least in floor.items():
            # (a kind that both calls get, as adjacent, has to show in each)
            n = min(v[0] for (sort, k), v in seen.items() if k == kind) if any(k == kind for _, k in seen) else 0
            most = SHORT.get((name, which, form, kind))
            if most is None:
                assert n >= least, (name, which, form, kind, n)
            else:
                assert n == most < least, (name, which, form, kind, n)
        assert len(d["streams"]) >= 48 and max(d["streams"]) - min(d["streams"]) > c.nseg * 3 // 4
        head = [j for j in range(22) if 1 <= c.offs[j + 1] - c.offs[j] <= 17]
        holding = set(x["rows"][:, 0].tolist())
        named = named_streams(np.diff(c.offs))
        empty = np.nonzero(np.diff(c.offs) == 0)[0]
        assert len(head) == 8 and set(head) <= set(named) and len(empty) >= 3
        assert all(k in named for j in empty.tolist() for k in (j - 1, j + 1) if 0 <= k < c.nseg and c.offs[k + 1] > c.offs[k])
        # every head stream and every neighbour of an empty stream that holds an occurrence gave a rule of each sort
        for sort, plan in (("rules", d["plan"]), ("ordered", d["seq_plan"])):
            single = {j for kind, j, _, _ in plan if kind == "single"}
            assert single == {j for j in named if j in holding}, (name, which, form, sort)
        # (seed5's patterns are rare over 256 symbols: streams of 1 to 17 bytes hold none in its group lists)
        assert any(j in holding for j in head) or name == "seed5"


def _seen(d, x, offs):
    """(sort, kind) -> [shown, planned] of the unordered and the ordered plan."""
    return {**{("rules", k): v for k, v in shown(d["plan"], *x["rules"], offs, x["before"]).items()},
            **{("ordered", k): v for k, v in shown(d["seq_plan"], *x["seq"], offs, x["before"]).items()}}


def _rules_in(ptr, hits, j):
    return set((hits[ptr[j]:ptr[j + 1]] & GID_MASK).tolist())


@pytest.mark.parametrize("name", CASES)
def test_the_flow_rules_cross_the_cut(name):
    """Per form, on the text reference's result alone: at least 20 rules
    complete in call 2 with a term carried from call 1, 5 are suppressed by a
    negated pattern only call 1 has, 5 fire in call 1 and are not reported
    again in call 2."""
    c, tab, plen = tables(name)
    for form in FORMS:
        f = expected_flow(c, form, tab)
        (p1, h1), (p2, h2) = f["calls"]
        n = dict(carried=0, neg_call1=0, once=0)
        for kind, j, r in f["plan"]:
            first, second = r in _rules_in(p1, h1, j), r in _rules_in(p2, h2, j)
            n[kind] += {"carried": not first and second, "neg_call1": not first and not second,
                        "once": first and not second}[kind]
        assert n["carried"] >= 20 and n["neg_call1"] >= 5 and n["once"] >= 5, (name, form, n)
        assert p1[-1] > 0 and p2[-1] > 0


def test_the_nocase_lists():
    """The nocase test's lists: the three derivations agree (the twins with
    the patterns' own lengths), every derived kind shows 32 times, and at
    least 8 rules of each sort pair two patterns that are equal up to case and
    differ in their nocase flag -- two gids where a code would be one."""
    from test_nocase_cpu import Twin
    from nocase_inputs import flag_of, fuzz_dictionary
    pats = fuzz_dictionary(0)
    gid = Twin(pats, [flag_of(p) for p in pats], pm.KIND_AC).gid_of_index
    x = expected_nocase(gid)
    plen = np.zeros(len(pats) + 1, np.uint32)
    for k, p in enumerate(pats):
        plen[gid[k]] = len(p)  # (of equal byte strings the later add has the gid)
    offs = x["offs"]
    nseg = len(offs) - 1
    assert len(x["pairs"]) >= 2 and x["began_before"] > 0
    for which in ("a", "b"):
        y = x[which]
        d = y["derived"]
        events = np.random.default_rng(13).permutation(events_of(y["rows"], offs, y["before"]))
        for exp, others in ((y["rules"], (reference_rules(events, offs, d["rules"]),
                                          pm.rules_by_stream_host(events, offs, d["rules"]))),
                            (y["seq"], (reference_seq_rules(events, offs, d["seq"], plen),
                                        pm.seq_rules_by_stream_host(events, offs, d["seq"], plen)))):
            for ptr, hits in others:
                assert np.array_equal(ptr, exp[0]) and np.array_equal(hits, exp[1]), which
        seen = _seen(d, y, offs)
        assert all(ok == planned for ok, planned in seen.values()), seen
        for kind in FIRING + NOT_FIRING + AA + (CALL2 if which == "b" else ()):
            assert min(v[0] for (_, k), v in seen.items() if k == kind) >= 32, (which, kind, seen)
        assert seen[("rules", CASE_PAIR[0])][0] >= 8 and seen[("ordered", CASE_PAIR[1])][0] >= 8, seen
        assert nseg == len(np.diff(offs))
