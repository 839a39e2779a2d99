"""References and generators of the rules tests (test_rules.py on the GPU,
test_rules_cpu.py without one).  TEST INFRASTRUCTURE; no device, nothing here
calls the library.

A rule is a list of ints: g is a positive term (gid g), -g a negated one.
reference_rules() is the dict-and-set statement of include/pm_hip.h "rules":
a rule fires in a stream iff every positive gid is in the stream's set and no
negated one is, at the largest of its positive terms' first positions.
"""
import numpy as np

GID_BITS = 24
GID_MAX = (1 << GID_BITS) - 1
NEGATED = 1 << 31
FAST = 1 << 30


def reference_rules(events, offsets, rules):
    """(rule_ptr int64 of nseg + 1, hits u64 of position << 24 | rule), each
    stream's range ascending.  The stream of a position is the first offset
    above it, minus one; events outside every stream are dropped."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    pos = (events >> np.uint64(GID_BITS)).astype(np.int64)
    gid = (events & np.uint64(GID_MAX)).astype(np.int64)
    j = np.searchsorted(offs, pos, side="right") - 1
    keep = (j >= 0) & (j < nseg)
    sets = {}
    for s, g, p in zip(j[keep].tolist(), gid[keep].tolist(), pos[keep].tolist()):
        first = sets.setdefault(s, {})
        first[g] = min(first.get(g, p), p)
    by_gid = {}
    for r, rule in enumerate(rules):
        by_gid.setdefault(next(g for g in rule if g > 0), []).append(r)
    ptr = np.zeros(nseg + 1, dtype=np.int64)
    hits = []
    for s in range(nseg):
        first = sets.get(s, {})
        mine = []
        for g in first:
            for r in by_gid.get(g, ()):
                rule = rules[r]
                if all((t in first) if t > 0 else (-t not in first) for t in rule):
                    mine.append((max(first[t] for t in rule if t > 0) << GID_BITS) | r)
        hits += sorted(mine)
        ptr[s + 1] = len(hits)
    return ptr, np.array(hits, dtype=np.uint64)


def csr(rules, fast=None):
    """(term_ptr u32, terms u32) of pm_hip_set_rules; fast[r] a gid or None."""
    ptr = np.zeros(len(rules) + 1, dtype=np.uint32)
    terms = []
    for r, rule in enumerate(rules):
        f = None if fast is None else fast[r]
        terms += [(-g | NEGATED) if g < 0 else (g | FAST) if g == f else g for g in rule]
        ptr[r + 1] = len(terms)
    return ptr, np.array(terms, dtype=np.uint32)


def random_rules(rng, nrules, gids, max_pos=4, negated=0.3):
    """nrules rules of 1..max_pos distinct positive terms drawn from gids, a
    share `negated` of them with one or two negated terms more."""
    gids = np.asarray(gids)
    rules = []
    for _ in range(nrules):
        k = int(rng.integers(1, min(max_pos, len(gids)) + 1))
        neg = int(rng.integers(1, 3)) if rng.random() < negated else 0
        pick = rng.choice(gids, size=min(k + neg, len(gids)), replace=False).tolist()
        rules.append([int(g) for g in pick[:k]] + [-int(g) for g in pick[k:]])
    return rules


def random_offsets(rng, nseg, max_len=40, base=None):
    """nseg stream lengths 0..max_len with runs of empty streams, from a base
    that is not 0."""
    lens = rng.integers(0, max_len + 1, size=nseg)
    at = 0
    while at < nseg:
        if rng.random() < 0.3:
            run = int(rng.integers(1, 40))
            lens[at:at + run] = 0
            at += run
        at += int(rng.integers(1, 60))
    base = int(rng.integers(1, 1000)) if base is None else base
    return base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)


def walk_tables(events, offsets, rules, anchor_ptr, anchor_rules):
    """The device's walk on the host, driven by pm_flat_rule_tables' index:
    every distinct (stream, gid) verifies the rules anchored at gid.  Returns
    reference_rules' form."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    sets = {}
    for e in events.tolist():
        p, g = e >> GID_BITS, e & GID_MAX
        s = int(np.searchsorted(offs, p, side="right")) - 1
        if 0 <= s < nseg:
            first = sets.setdefault(s, {})
            first[g] = min(first.get(g, p), p)
    ptr = np.zeros(nseg + 1, dtype=np.int64)
    hits = []
    for s in range(nseg):
        first = sets.get(s, {})
        mine = []
        for g in first:
            if g + 1 >= len(anchor_ptr):
                continue
            for r in anchor_rules[anchor_ptr[g]:anchor_ptr[g + 1]].tolist():
                rule = rules[r]
                if all((t in first) if t > 0 else (-t not in first) for t in rule):
                    mine.append((max(first[t] for t in rule if t > 0) << GID_BITS) | r)
        hits += sorted(mine)
        ptr[s + 1] = len(hits)
    return ptr, np.array(hits, dtype=np.uint64)
