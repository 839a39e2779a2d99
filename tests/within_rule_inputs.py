"""References and generators of the within tests (test_within_rules.py on the
GPU, test_within_rules_cpu.py without one).  TEST INFRASTRUCTURE; no device,
nothing here calls the library.

A rule is seq_rule_inputs' list of terms, in which a term is (g, gap) or
(g, gap, w): w None or absent for no upper bound, else the occurrence chosen
for the term must end at most w bytes after the one chosen for the positive
term before it has ended (include/pm_hip.h "ordered rules", within).

reference_within_rules() is reference_seq_rules() with the all-pairs test f +
d + L <= o <= f + w per level: no bisection, no cursor.  exhaustive() tries
every choice of one occurrence per positive term.  greedy_with_check() makes
the distance-only greedy choice and then tests the bounds: what a caller would
get who bolted a check onto the greedy call; it only counts cases.
"""
import itertools

import numpy as np

from seq_rule_inputs import (FAST, FREE, GID_BITS, NEGATED, pack, random_seq_rules, reference_seq_rules,
                             stream_occurrences)

SPAN = 400


def split(term):
    """(g, gap, w) of a term in either form."""
    return (term[0], term[1], None) if len(term) == 2 else (term[0], term[1], term[2])


def distance_only(rules):
    """The rules without their upper bounds (a bare within keeps its gap 0)."""
    out = []
    for rule in rules:
        out.append([(g, 0 if gap is None and w is not None else gap) for g, gap, w in map(split, rule)])
    return out


def chains_of(rule):
    """The rule's chains, each a list of (gid, gap, w) with the head's gap
    None, and the gids of its negated terms."""
    chains, negs = [], []
    for g, gap, w in map(split, rule):
        if w is not None and gap is None:
            gap = 0
        if g < 0:
            negs.append(-g)
        elif gap is None:
            chains.append([(g, None, None)])
        else:
            chains[-1].append((g, gap, w))
    return chains, negs


def rule_in_stream(occ, rule, plen):
    """The hit position of the rule over one stream's occurrences (occ: gid ->
    ascending array of positions), or None: every pair of every level."""
    chains, negs = chains_of(rule)
    if any(len(occ.get(g, ())) for g in negs):
        return None
    position = -1
    for chain in chains:
        feasible = np.asarray(occ.get(chain[0][0], ()), dtype=np.int64)
        for g, d, w in chain[1:]:
            if not len(feasible):
                break
            o = np.asarray(occ.get(g, ()), dtype=np.int64)
            if not len(o):
                feasible = o
                break
            ok = feasible[:, None] + d + int(plen[g]) <= o[None, :]
            if w is not None:
                ok &= o[None, :] <= feasible[:, None] + w
            feasible = o[ok.any(axis=0)]
        if not len(feasible):
            return None
        position = max(position, int(feasible.min()))
    return position


def exhaustive(occ, rule, plen, limit=5000):
    """The same by trying every choice of one occurrence per positive term;
    "skip" where there are more than `limit` choices."""
    chains, negs = chains_of(rule)
    if any(len(occ.get(g, ())) for g in negs):
        return None
    terms = [t for chain in chains for t in chain]
    lists = [[int(p) for p in occ.get(g, ())] for g, _, _ in terms]
    total = 1
    for lst in lists:
        total *= len(lst)
    if total > limit:
        return "skip"
    best = None
    for choice in itertools.product(*lists):
        ok = True
        for i, (g, d, w) in enumerate(terms):
            if d is None:
                continue
            if choice[i] < choice[i - 1] + d + int(plen[g]) or (w is not None and choice[i] > choice[i - 1] + w):
                ok = False
                break
        if ok and (best is None or max(choice) < best):
            best = max(choice)
    return best


def greedy_with_check(occ, rule, plen):
    """The distance-only greedy choice (a head at its first position, a
    follower at its first position that satisfies the distance), which fails
    when that choice breaks a bound."""
    chains, negs = chains_of(rule)
    if any(len(occ.get(g, ())) for g in negs):
        return None
    position = -1
    for chain in chains:
        prev = None
        for g, d, w in chain:
            o = np.asarray(occ.get(g, ()), dtype=np.int64)
            if d is not None:
                o = o[o >= prev + d + int(plen[g])]
            if not len(o) or (w is not None and int(o[0]) > prev + w):
                return None
            prev = int(o[0])
        position = max(position, prev)
    return position


def per_pair(events, offsets, rules, plen, fn=rule_in_stream):
    """{(stream, rule): fn's answer} over the streams that hold anything."""
    occ = stream_occurrences(events, offsets)
    return {(s, r): fn(occ[s], rule, plen) for s in sorted(occ) for r, rule in enumerate(rules)}


def reference_within_rules(events, offsets, rules, plen):
    """(rule_ptr int64 of nseg + 1, hits u64 of position << 24 | rule), each
    stream's range ascending."""
    nseg = len(offsets) - 1
    occ = stream_occurrences(events, offsets)
    ptr = np.zeros(nseg + 1, dtype=np.int64)
    hits = []
    for s in range(nseg):
        mine = []
        if s in occ:
            for r, rule in enumerate(rules):
                p = rule_in_stream(occ[s], rule, plen)
                if p is not None:
                    mine.append((p << GID_BITS) | r)
        hits += sorted(mine)
        ptr[s + 1] = len(hits)
    return ptr, np.array(hits, dtype=np.uint64)


def within_csr(rules, fast=None):
    """(term_ptr, terms, gaps, withins) u32 of pm_hip_set_seq_rules_within;
    fast[r] a gid or None (the flag goes on the first positive term of that gid)."""
    ptr = np.zeros(len(rules) + 1, dtype=np.uint32)
    terms, gaps, withins = [], [], []
    for r, rule in enumerate(rules):
        f = None if fast is None else fast[r]
        for g, gap, w in map(split, rule):
            if w is not None and gap is None:
                gap = 0
            if g == f:
                terms.append(g | FAST)
                f = None
            else:
                terms.append((-g | NEGATED) if g < 0 else g)
            gaps.append(FREE if gap is None else gap)
            withins.append(FREE if w is None else w)
        ptr[r + 1] = len(terms)
    u32 = lambda v: np.array(v, dtype=np.uint32)  # noqa: E731
    return ptr, u32(terms), u32(gaps), u32(withins)


def with_bounds(rng, rules, plen, share=0.7, slack=40):
    """The rules with a bound d + L + U[0, slack] on `share` of their following terms."""
    out = []
    for rule in rules:
        new = []
        for g, gap in rule:
            if g > 0 and gap is not None and rng.random() < share:
                new.append((g, gap, gap + int(plen[g]) + int(rng.integers(0, slack + 1))))
            else:
                new.append((g, gap))
        out.append(new)
    return out


def within_run(rules):
    """The longest run of consecutive bounded links in any rule (negated terms
    stand in no chain and break no run)."""
    best = 0
    for rule in rules:
        run = 0
        for g, gap, w in map(split, rule):
            if g < 0:
                continue
            run = run + 1 if w is not None else 0
            best = max(best, run)
    return best


def fuzz_case(seed, scale=1.0, plen=None):
    """(events, offsets, rules, plen): 50-200 streams of up to 400 bytes,
    5,000-30,000 events times scale (the tests pass scale 0.2: 1,000-6,000
    events, which keeps the all-pairs reference quick and still meets the
    counts test_within_rules_cpu.py asserts: 10,977 / 5,679 / 7,695 over its
    six seeds) over 2-6 gids of 1-8 bytes, 200 rules of up to 5 positive
    terms, 80% of the later ones following at a distance of up to 10, 70% of
    those with a bound d + L + U[0, 40].  plen: the lengths of gids 0..6 at
    least, in place of the random ones."""
    rng = np.random.default_rng(7000 + seed)
    nseg = int(rng.integers(50, 201))
    lens = rng.integers(0, SPAN + 1, size=nseg)
    offs = np.concatenate([[int(rng.integers(0, 1000))], lens]).cumsum().astype(np.int64)
    n = int(int(rng.integers(5000, 30001)) * scale)
    ngid = int(rng.integers(2, 7))
    drawn = np.concatenate([[0], rng.integers(1, 9, size=ngid)]).astype(np.uint32)
    plen = drawn if plen is None else np.asarray(plen, dtype=np.uint32)[:ngid + 1]
    events = pack(rng.integers(max(int(offs[0]) - 20, 0), int(offs[-1]) + 20, size=n), rng.integers(1, ngid + 1, size=n))
    rules = with_bounds(rng, random_seq_rules(rng, 200, range(1, ngid + 1), max_pos=5, follow=0.8, max_gap=10), plen)
    return events, offs, rules, plen


def fuzz_counts(events, offs, rules, plen):
    """Over the (stream, rule) pairs, on the reference alone: (the reference
    fires and greedy_with_check does not, the reference fires later than the
    distance-only reference, the bound kills a pair that distance alone fires)."""
    exact = per_pair(events, offs, rules, plen)
    greedy = per_pair(events, offs, rules, plen, greedy_with_check)
    loose = per_pair(events, offs, distance_only(rules), plen)
    rescued = sum(1 for k, v in exact.items() if v is not None and greedy[k] is None)
    later = sum(1 for k, v in exact.items() if v is not None and loose[k] is not None and v > loose[k])
    killed = sum(1 for k, v in exact.items() if v is None and loose[k] is not None)
    return rescued, later, killed


# ---- the planted kinds ----------------------------------------------------------------
# gids 1..5 are A, B, C, D, E; every planted stream is 400 bytes long and holds one kind.
KINDS = ("rescued", "upper_by_zero", "upper_by_one", "two_back", "memo", "later_position", "killed", "exact_gap",
         "aa_within", "mixed", "two_chains", "two_chains_both", "neighbour", "duplicates")


def planted_case(seed, ngid=12, noise=True, plen=None):
    """(events, offsets, rules, plen, plan): a shuffled list with duplicated
    events over one planted stream per kind of KINDS and random streams.  plan
    maps a kind to (stream, rule, expected position or None).  The planted
    rules come first, random bounded ones follow.  plen: the lengths of gids
    0..ngid at least, those of gids 1..5 at most 30 bytes (None: random ones
    of 1 to 8 bytes)."""
    rng = np.random.default_rng(seed)
    drawn = np.concatenate([[0], rng.integers(1, 9, size=ngid)]).astype(np.uint32)
    plen = drawn if plen is None else np.asarray(plen, dtype=np.uint32)
    assert len(plen) > ngid and plen[1:6].max() <= 30 and plen[1:ngid + 1].min() >= 1
    A, B, C, D = 1, 2, 3, 4
    LA, LB, LC, LD = (int(plen[g]) for g in (A, B, C, D))
    base = int(rng.integers(1, 1000))
    p = int(rng.integers(100, 120))
    d = int(rng.integers(1, 9))
    rules, streams, plan = [], [], {}

    def plant(kind, rule, expect, ev, twice=False):
        at = base + SPAN * len(streams)
        assert all(0 <= q < SPAN for q, _ in ev), kind
        if kind:
            rules.append(rule)
            plan[kind] = (len(streams), len(rules) - 1, None if expect is None else at + expect)
        streams.append([(at + q, g) for q, g in ev] * (2 if twice else 1))

    # rescued: the only B ends within reach of the second A alone: the greedy choice (the first A) fails
    rescued = [(A, None), (B, 0, LB + 5)]
    plant("rescued", rescued, p + 100 + LB + 2, [(p, A), (p + 100, A), (p + 100 + LB + 2, B)])
    plant("upper_by_zero", [(A, None), (B, 2, LB + 10)], p + LB + 10, [(p, A), (p + LB + 10, B)])
    plant("upper_by_one", [(A, None), (B, 2, LB + 10)], None, [(p, A), (p + LB + 11, B)])
    # two_back: B1 reachable from A1 only, B2 from A2 only, C from B2 only
    b2 = p + 60 + LB + 1
    plant("two_back", [(A, None), (B, 0, LB + 3), (C, 0, LC + 3)], b2 + LC + 2,
          [(p, A), (p + LB + 1, B), (p + 60, A), (b2, B), (b2 + LC + 2, C)])
    # memo: the first C begins inside B and fails; the second asks B's level for the same answer
    b = p + LB
    plant("memo", [(A, None), (B, 0, LB + 5), (C, 0, LC + 10)], b + LC + 1, [(p, A), (b, B), (b + LC - 1, C), (b + LC + 1, C)])
    later = [(A, None), (B, 0, LB + 4)]
    plant("later_position", later, p + 50 + LB + 1, [(p, A), (p + LB + 20, B), (p + 50, A), (p + 50 + LB + 1, B)])
    plant("killed", [(A, None), (B, 0, LB + 4)], None, [(p, A), (p + LB + 30, B)])
    plant("exact_gap", [(A, None), (B, d, d + LB)], p + 40 + d + LB,
          [(p, A), (p + d + LB - 1, B), (p + d + LB + 1, B), (p + 40, A), (p + 40 + d + LB, B)])
    plant("aa_within", [(A, None), (A, 0, LA + 6)], p + 50 + LA + 3, [(p, A), (p + 50, A), (p + 50 + LA + 3, A)])
    # mixed: bounded, unbounded, bounded; an early C with a D in reach lies before B: the second run's head
    # is constrained by E + d + L
    bb = p + LB + 1
    c = bb + 5 + LC + 2
    plant("mixed", [(A, None), (B, 0, LB + 3), (C, 5), (D, 0, LD + 4)], c + LD + 2,
          [(p, A), (bb, B), (35, C), (35 + LD + 1, D), (c, C), (c + LD + 2, D)])
    chains = [(A, None), (B, 0, LB + 3), (C, None), (D, 0, LD + 3)]
    plant("two_chains", chains, None, [(p, A), (p + LB + 1, B), (p + 100, C), (p + 100 + LD + 4, D)])
    plant("two_chains_both", chains, p + 100 + LD + 3, [(p, A), (p + LB + 1, B), (p + 100, C), (p + 100 + LD + 3, D)])
    # neighbour: B within reach only across the stream boundary
    plant("neighbour", [(A, None), (B, 0, 2 * LB + 10)], None, [(SPAN - 2, A)])
    plant(None, None, None, [(LB, B)])
    plant("duplicates", [(A, None), (B, 0, LB + 5), (C, 1, LC + 4)], p + 100 + LB + 2 + 1 + LC,
          [(p, A), (p + 100, A), (p + 100 + LB + 2, B), (p + 100 + LB + 2 + 1 + LC, C)], twice=True)
    planted = len(streams)
    pos = [q for s in streams for q, _ in s]
    gid = [g for s in streams for _, g in s]
    offs = [base + SPAN * k for k in range(planted + 1)]
    if noise:
        nrand = int(rng.integers(3, 30))
        lens = rng.integers(0, 120, size=nrand)
        lens[rng.random(nrand) < 0.2] = 0
        offs += (offs[-1] + np.cumsum(lens)).tolist()
        n = int(rng.integers(50, 600))
        pos += rng.integers(offs[planted], offs[-1] + 20, size=n).tolist()
        gid += rng.integers(1, ngid + 1, size=n).tolist()
        more = random_seq_rules(rng, int(rng.integers(5, 60)), range(1, ngid + 1), max_pos=5, follow=0.8, max_gap=10)
        rules = rules + with_bounds(rng, more, plen)
    events = pack(pos, gid)
    events = np.concatenate([events, events[rng.integers(0, len(events), size=len(events) // 3)]])  # duplicates
    return rng.permutation(events), np.asarray(offs, dtype=np.int64), rules, plen, plan


def kinds_shown(events, offs, rules, plen, plan):
    """kind -> whether the references show it: seq_rule_inputs.kinds_present
    on reference_within_rules, and for the kinds that are about the difference
    to the greedy or the distance-only answer, that difference."""
    from seq_rule_inputs import kinds_present
    seen = kinds_present(plan, *reference_within_rules(events, offs, rules, plen))
    occ = stream_occurrences(events, offs)
    loose_ptr, loose_hits = reference_seq_rules(events, offs, distance_only(rules), plen)

    def loose(kind):
        s, r, _ = plan[kind]
        mine = loose_hits[loose_ptr[s]:loose_ptr[s + 1]]
        got = [int(h >> np.uint64(GID_BITS)) for h in mine if int(h & np.uint64((1 << GID_BITS) - 1)) == r]
        return got[0] if got else None
    for kind in ("rescued", "two_back", "later_position", "duplicates"):
        s, r, _ = plan[kind]
        seen[kind] = seen[kind] and greedy_with_check(occ[s], rules[r], plen) is None
    seen["later_position"] = seen["later_position"] and loose("later_position") < plan["later_position"][2]
    for kind in ("killed", "upper_by_one", "two_chains"):
        seen[kind] = seen[kind] and loose(kind) is not None
    return seen
