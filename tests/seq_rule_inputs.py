"""Reference and generators of the ordered-rules tests (test_seq_rules.py on
the GPU, test_seq_rules_cpu.py without one).  TEST INFRASTRUCTURE; no device,
nothing here calls the library.

A rule is a list of (g, gap) pairs: g a positive term (gid g), -g a negated
one; gap None for a free term, d >= 0 for a term that begins at least d bytes
after the positive term listed before it has ended (include/pm_hip.h "ordered
rules").  plen[g] is the length of pattern g.

reference_seq_rules() does not use the greedy argument: per stream and rule it
computes, level by level, the set of feasible occurrences of every chain --
occurrence o of term i is feasible iff SOME feasible occurrence of term i - 1
satisfies the link -- takes the minimum over the last level and the maximum
over the chains.
"""
import numpy as np

GID_BITS = 24
GID_MAX = (1 << GID_BITS) - 1
NEGATED = 1 << 31
FAST = 1 << 30
FREE = 0xFFFFFFFF


def pack(pos, gid):
    return (np.asarray(pos, dtype=np.uint64) << np.uint64(GID_BITS)) | np.asarray(gid, dtype=np.uint64)


def chains_of(rule):
    """The rule's chains, each a list of (gid, gap) with the head's gap None,
    and the gids of its negated terms."""
    chains, negs = [], []
    for g, gap in rule:
        if g < 0:
            negs.append(-g)
        elif gap is None:
            chains.append([(g, None)])
        else:
            chains[-1].append((g, gap))
    return chains, negs


def rule_in_stream(occ, rule, plen):
    """The hit position of the rule over one stream's occurrences (occ: gid ->
    ascending array of positions), or None."""
    chains, negs = chains_of(rule)
    if any(len(occ.get(g, ())) for g in negs):
        return None
    position = -1
    for chain in chains:
        feasible = np.asarray(occ.get(chain[0][0], ()), dtype=np.int64)
        for g, d in chain[1:]:
            if not len(feasible):
                break
            o = np.asarray(occ.get(g, ()), dtype=np.int64)
            # o[k] is feasible iff some feasible f has f + d + L <= o[k]: every pair is looked at
            ok = (feasible[:, None] + d + int(plen[g]) <= o[None, :]).any(axis=0) if len(o) else np.zeros(0, bool)
            feasible = o[ok]
        if not len(feasible):
            return None
        position = max(position, int(feasible.min()))
    return position


def stream_occurrences(events, offsets):
    """Per stream, gid -> ascending array of the distinct positions of its
    events inside the stream."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    pos = (events >> np.uint64(GID_BITS)).astype(np.int64)
    gid = (events & np.uint64(GID_MAX)).astype(np.int64)
    j = np.searchsorted(offs, pos, side="right") - 1
    keep = (j >= 0) & (j < nseg)
    out = {}
    for s, g, p in zip(j[keep].tolist(), gid[keep].tolist(), pos[keep].tolist()):
        out.setdefault(s, {}).setdefault(g, set()).add(p)
    return {s: {g: np.array(sorted(v), dtype=np.int64) for g, v in d.items()} for s, d in out.items()}


def reference_seq_rules(events, offsets, rules, plen):
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


def seq_csr(rules, fast=None):
    """(term_ptr u32, terms u32, gaps u32) of pm_hip_set_seq_rules; fast[r] a
    gid or None (the flag goes on the first positive term of that gid)."""
    ptr = np.zeros(len(rules) + 1, dtype=np.uint32)
    terms, gaps = [], []
    for r, rule in enumerate(rules):
        f = None if fast is None else fast[r]
        for g, gap in rule:
            if g == f:
                terms.append(g | FAST)
                f = None
            else:
                terms.append((-g | NEGATED) if g < 0 else g)
            gaps.append(FREE if gap is None else gap)
        ptr[r + 1] = len(terms)
    return ptr, np.array(terms, dtype=np.uint32), np.array(gaps, dtype=np.uint32)


def free_rules(rules):
    """Unordered rules (rule_inputs' form) as ordered rules with every gap free."""
    return [[(g, None) for g in r] for r in rules]


def random_seq_rules(rng, nrules, gids, max_pos=4, negated=0.3, follow=0.6, max_gap=6):
    """nrules ordered rules of 1..max_pos positive terms drawn from gids.  The
    first positive term is free; a later one follows with probability
    `follow` (at a distance 0..max_gap, and it may repeat a gid the rule has
    already: A ... A), else it is a free term of a gid the rule has not yet.
    A share `negated` has one or two negated terms, put anywhere in the list."""
    gids = [int(g) for g in gids]
    rules = []
    for _ in range(nrules):
        k = int(rng.integers(1, max_pos + 1))
        rule, used = [], set()
        for i in range(k):
            if i and rng.random() < follow:
                g = int(rng.choice(gids))
                rule.append((g, int(rng.integers(0, max_gap + 1))))
            else:
                rest = [g for g in gids if g not in used]
                if not rest:
                    break
                g = int(rng.choice(rest))
                rule.append((g, None))
            used.add(g)
        if rng.random() < negated:
            for _ in range(int(rng.integers(1, 3))):
                rest = [g for g in gids if g not in used]
                if rest:
                    g = int(rng.choice(rest))
                    used.add(g)
                    rule.insert(int(rng.integers(0, len(rule) + 1)), (-g, None))
        rules.append(rule)
    return rules


# ---- the planted kinds ----------------------------------------------------------------
# gids 1..5 are A, B, C, D, E; every planted stream is 400 bytes long.
KINDS = ("later_occurrence", "wrong_order", "fails_by_one", "passes_by_zero", "aa_one", "aa_two", "overlap",
         "two_chains", "negation", "neighbour")
SPAN = 400


def planted_case(seed, ngid=12, noise=True, plen=None):
    """(events, offsets, rules, plen, plan): a list in shuffled order with
    duplicated events, over planted streams (one or two per kind of KINDS)
    and random ones.  plan maps a kind to (stream, rule, expected position or
    None).  Rules 0..4 are the planted ones, random ones follow.  plen: the
    lengths of gids 0..ngid at least (None: random ones of 1 to 8 bytes; at
    most 100 bytes each, so that a planted stream holds its plants)."""
    rng = np.random.default_rng(seed)
    drawn = np.concatenate([[0], rng.integers(1, 9, size=ngid)]).astype(np.uint32)
    plen = drawn if plen is None else np.asarray(plen, dtype=np.uint32)
    assert len(plen) > ngid and plen[1:ngid + 1].max() <= 100
    A, B, C, D, E = 1, 2, 3, 4, 5
    dist = int(rng.integers(1, 40))
    rules = [[(A, None), (B, 0)], [(A, None), (B, dist)], [(A, None), (A, dist)],
             [(A, None), (B, 0), (C, None), (D, 0)], [(A, None), (-E, None), (B, 0)]]
    LB, LA, LD = int(plen[B]), int(plen[A]), int(plen[D])
    base = int(rng.integers(1, 1000))
    streams, plan = [], {}

    def stream(kind, rule, expect, ev):
        at = base + SPAN * len(streams)
        if kind:
            plan[kind] = (len(streams), rule, None if expect is None else at + expect)
        streams.append([(at + p, g) for p, g in ev])

    p = int(rng.integers(20, 60))
    # B's first occurrence lies before A: only its second one satisfies the link
    stream("later_occurrence", 0, p + LB + 3, [(5, B), (p, A), (p + LB + 3, B)])
    stream("wrong_order", 0, None, [(10, B), (p + 50, A)])
    stream("fails_by_one", 1, None, [(p, A), (p + dist + LB - 1, B)])
    stream("passes_by_zero", 1, p + dist + LB, [(p, A), (p + dist + LB, B)])
    stream("aa_one", 2, None, [(p, A)])
    stream("aa_two", 2, p + dist + LA, [(p, A), (p + dist + LA, A)])
    # B begins at A's last byte: p_B - L_B + 1 == p_A
    stream("overlap", 0, None, [(p, A), (p + LB - 1, B)])
    # the second chain ends later than the first: its end is the position
    stream("two_chains", 3, p + 100 + LD + 7, [(p, A), (p + LB, B), (p + 100, C), (p + 100 + LD + 7, D)])
    stream("negation", 4, None, [(p, A), (p + LB, B), (300, E)])
    # A in one stream, B only in the next one, near enough to satisfy the link were it the same stream
    stream("neighbour", 0, None, [(SPAN - 2, A)])
    stream(None, 0, None, [(LB + 1, B)])
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
        rules = rules + random_seq_rules(rng, int(rng.integers(5, 60)), range(1, ngid + 1))
    events = pack(pos, gid)
    events = np.concatenate([events, events[rng.integers(0, len(events), size=len(events) // 3)]])  # duplicates
    return rng.permutation(events), np.asarray(offs, dtype=np.int64), rules, plen, plan


def kinds_present(plan, ptr, hits):
    """kind -> whether the result (reference_seq_rules' form) shows it: the
    planted rule fires in the planted stream at the expected position, or
    does not fire there although every pattern of it that should be present
    is (the generator placed them)."""
    seen = {}
    for kind, (s, r, expect) in plan.items():
        mine = hits[ptr[s]:ptr[s + 1]]
        got = [int(h >> np.uint64(GID_BITS)) for h in mine if int(h & np.uint64(GID_MAX)) == r]
        seen[kind] = got == ([] if expect is None else [expect])
    return seen
