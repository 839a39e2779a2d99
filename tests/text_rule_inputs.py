"""Rules stated on the text (test_text_rules.py on the GPU,
test_text_rules_cpu.py without one).  TEST INFRASTRUCTURE; no device, nothing
here calls the library.

The references of rule_inputs, seq_rule_inputs and flow_rule_inputs work on
events (position << 24 | gid) and, for a link, on the formula p_t >= p_u + d +
L_t with L from the library.  Here an occurrence is a row (stream, start,
end_exclusive, id): where the pattern's bytes lie in the stream's text, in
stream-relative coordinates (call 2 of a flow counts from the flow's first
byte, so a match that began in call 1 has start < len(A_j)).  The lengths are
those of the oracle's own patterns (event_inputs.code_lengths), or the brute
force's starts (nocase_inputs.brute).  id is the oracle's code, or the gid
once to_gids() has mapped it: the terms of a rule are gids.

rules_from_text, seq_rules_from_text and flow_rules_from_text state
include/pm_hip.h "rules", "ordered rules" (the link written on the text: the
occurrence chosen for t has start_t >= end_exclusive_u + d; no pattern length)
and the prefix sentence of "flow rules" on such rows, a rule at a time over
all streams at once.  exhaustive_seq tries every choice of one stream.
derived_rules builds rules from what selected streams hold, so that firing --
and failing by one byte -- is by construction.
"""
import itertools

import numpy as np

from event_inputs import code_lengths
from rule_inputs import GID_BITS, random_rules
from seq_rule_inputs import chains_of, random_seq_rules

INF = np.iinfo(np.int64).max
FIRING = ("unordered", "neg_absent", "pair_max", "chain3", "two_chains")
NOT_FIRING = ("neg_present", "pair_plus1", "overlap", "adjacent")
AA = ("aa_exact", "aa_plus1")
CALL2 = ("straddle_head", "straddle_follower")
CASE_PAIR = ("case_pair", "case_pair_seq")
PER_KIND = 40  # rules of one kind per list (the CPU file asks for 32 that show it) ...
MIN_STREAMS = 48  # ... or more, until so many streams have given a rule


# ---- occurrences ------------------------------------------------------------------------------
def rows_of_list(key, pos, codes, offs, before=None):
    """Rows (stream, start, end_exclusive, code) of an oracle-derived (buffer
    positions, codes) list over the offsets; before[j]: the bytes stream j's
    flow had before this call (None: none)."""
    offs = np.asarray(offs, dtype=np.int64)
    pos = np.asarray(pos, dtype=np.int64)
    cl, ll = code_lengths(key)
    k = np.searchsorted(cl, codes)
    assert np.array_equal(cl[k], codes)
    j = np.searchsorted(offs, pos, side="right") - 1
    assert len(pos) == 0 or (j.min() >= 0 and pos.max() < offs[-1])
    end = pos - offs[j] + 1 + (0 if before is None else np.asarray(before, dtype=np.int64)[j])
    return np.stack([j, end - ll[k], end, np.asarray(codes).astype(np.int64)], axis=1)


def occurrences(c, which, form):
    """The rows of a fuzz case's text `which` ("a": A, every stream from its
    first byte; "b": B continuing A) in a form of test_fuzz_by_stream_cpu.FORMS."""
    from test_fuzz_by_stream_cpu import want
    pos, codes = want(c, which, form)
    return rows_of_list(c.key, pos, codes, c.offs, None if which == "a" else np.diff(c.offs))


def nocase_occurrences(brute_rows, lens, which):
    """The rows of nocase_inputs.brute over whole flows (stream, end, gid,
    start), cut to call `which`: "a" the ends inside the first lens[j] bytes,
    "b" those behind them."""
    r = np.asarray(brute_rows, dtype=np.int64)
    first = r[:, 1] < np.asarray(lens, dtype=np.int64)[r[:, 0]]
    r = r[first if which == "a" else ~first]
    return np.stack([r[:, 0], r[:, 3], r[:, 1] + 1, r[:, 2]], axis=1)


def to_gids(rows, code_of_gid):
    """The rows with the code replaced by its gid; code_of_gid[g] is the code
    of gid g ([0] unused): the matcher's _codes or the image's gid table."""
    tab = np.asarray(code_of_gid, dtype=np.int64)
    assert len(np.unique(tab[1:])) == len(tab) - 1, "a code names one gid"
    order = np.argsort(tab[1:], kind="stable")
    k = np.minimum(np.searchsorted(tab[1:][order], rows[:, 3]), len(order) - 1)
    g = order[k] + 1
    assert np.array_equal(tab[g], rows[:, 3])
    out = rows.copy()
    out[:, 3] = g
    return out


def events_of(rows, offs, before=None):
    """The rows as u64 events position << 24 | id in buffer coordinates."""
    offs = np.asarray(offs, dtype=np.int64)
    j = rows[:, 0]
    pos = offs[j] + rows[:, 2] - 1 - (0 if before is None else np.asarray(before, dtype=np.int64)[j])
    return (pos.astype(np.uint64) << np.uint64(GID_BITS)) | rows[:, 3].astype(np.uint64)


class _ById:
    """The rows of each id, ascending by (stream, end_exclusive)."""

    def __init__(self, rows, nseg):
        self.nseg = nseg
        order = np.lexsort((rows[:, 2], rows[:, 0], rows[:, 3]))
        r = rows[order]
        ids, at = np.unique(r[:, 3], return_index=True)
        cut = np.append(at, len(r))
        self.of = {int(g): r[cut[k]:cut[k + 1]] for k, g in enumerate(ids.tolist())}
        self._first = {}
        self.none = np.zeros((0, 4), np.int64)

    def rows(self, g):
        return self.of.get(g, self.none)

    def smallest_end(self, r):
        """Per stream the smallest end_exclusive among rows r (a subset of one
        id's rows, in their order), INF where there is none."""
        out = np.full(self.nseg, INF, np.int64)
        streams, at = np.unique(r[:, 0], return_index=True)  # (ends ascend inside a stream: the first is the smallest)
        out[streams] = r[at, 2]
        return out

    def first_end(self, g):
        """Per stream the smallest end_exclusive of id g, INF where it has none."""
        if g not in self._first:
            self._first[g] = self.smallest_end(self.rows(g))
        return self._first[g]


def _csr(found, nseg, offs, before):
    """found: per rule (streams, end_exclusive of the hit).  (rule_ptr, hits)
    in buffer coordinates, each stream's range ascending."""
    offs = np.asarray(offs, dtype=np.int64)
    s = np.concatenate([f[0] for f in found] + [np.zeros(0, np.int64)])
    e = np.concatenate([f[1] for f in found] + [np.zeros(0, np.int64)])
    r = np.concatenate([np.full(len(f[0]), k, np.int64) for k, f in enumerate(found)] + [np.zeros(0, np.int64)])
    pos = offs[s] + e - 1 - (0 if before is None else np.asarray(before, dtype=np.int64)[s])
    order = np.lexsort((r, pos, s))
    ptr = np.searchsorted(s[order], np.arange(nseg + 1), side="left").astype(np.int64)
    return ptr, (pos[order].astype(np.uint64) << np.uint64(GID_BITS)) | r[order].astype(np.uint64)


def _unordered(by, rule):
    """(streams, end_exclusive): where every positive id occurs and no negated
    one does, the largest of the positive ids' first ends."""
    hit = np.zeros(by.nseg, np.int64)
    ok = np.ones(by.nseg, bool)
    for t in rule:
        first = by.first_end(abs(t))
        if t > 0:
            ok &= first < INF
            hit = np.maximum(hit, first)
        else:
            ok &= first == INF
    s = np.nonzero(ok)[0]
    return s, hit[s]


def rules_from_text(rows, nseg, rules, offs, before=None):
    """(rule_ptr, hits) in buffer coordinates (offs; before[j]: the bytes flow
    j had before the call), as the event references give them.
    include/pm_hip.h "rules" on the rows: rule r fires in a stream iff every
    positive term occurs in it and no negated one does, at the largest of its
    positive terms' first ends."""
    by = rows if isinstance(rows, _ById) else _ById(rows, nseg)
    return _csr([_unordered(by, rule) for rule in rules], nseg, offs, before)


def _seq(by, rule):
    """(streams, end_exclusive) of one ordered rule.  Per chain the feasible
    sets level by level: an occurrence of t is feasible iff SOME feasible
    occurrence of the term before it has end_exclusive + d <= start_t, which
    the smallest feasible end decides for all of them; the minimum of the last
    level's ends, the maximum over the chains."""
    chains, negs = chains_of(rule)
    ok = np.ones(by.nseg, bool)
    for g in negs:
        ok &= by.first_end(g) == INF
    hit = np.zeros(by.nseg, np.int64)
    for chain in chains:
        low = by.first_end(chain[0][0])  # per stream the smallest end of the level's feasible set
        for g, d in chain[1:]:
            r = by.rows(g)
            bound = low[r[:, 0]]
            feasible = r[(bound < INF) & (r[:, 1] >= np.where(bound < INF, bound, 0) + d)]
            low = by.smallest_end(feasible)
        ok &= low < INF
        hit = np.maximum(hit, low)
    s = np.nonzero(ok)[0]
    return s, hit[s]


def seq_rules_from_text(rows, nseg, rules, offs, before=None):
    """include/pm_hip.h "ordered rules" on the rows, the link written on the
    text: start_t >= end_exclusive_u + d."""
    by = rows if isinstance(rows, _ById) else _ById(rows, nseg)
    return _csr([_seq(by, rule) for rule in rules], nseg, offs, before)


def seq_positions(rows, nseg, rules):
    """Per rule {stream: end_exclusive of the hit}, for exhaustive_seq's check."""
    by = _ById(rows, nseg)
    return [dict(zip(*(a.tolist() for a in _seq(by, rule)))) for rule in rules]


def flow_rules_from_text(rows_whole_flow, before, lens, rules):
    """The prefix sentence of include/pm_hip.h "flow rules": rule r hits in the
    call that gives every flow j the bytes [before[j], before[j] + lens[j]) iff,
    over the flow's bytes through this call, every positive term occurs and no
    negated one does, and the largest of the positive terms' first ends lies in
    this call's bytes.  No set is carried.  The buffer holds the streams one
    after the other from 0."""
    before = np.asarray(before, dtype=np.int64)
    lens = np.asarray(lens, dtype=np.int64)
    nseg = len(lens)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    r = np.asarray(rows_whole_flow, dtype=np.int64)
    by = _ById(r[r[:, 2] <= (before + lens)[r[:, 0]]], nseg)
    found = []
    for rule in rules:
        s, e = _unordered(by, rule)
        mine = e > before[s]
        found.append((s[mine], e[mine]))
    return _csr(found, nseg, offs, before)


def flow_bits_from_text(rows_whole_flow, before, lens, rules):
    """Per stream the set of term ids the flow's text holds through the call."""
    named = {abs(t) for rule in rules for t in rule}
    r = np.asarray(rows_whole_flow, dtype=np.int64)
    r = r[r[:, 2] <= (np.asarray(before) + np.asarray(lens))[r[:, 0]]]
    held = _ids_by_stream(r)
    return [held.get(s, set()) & named for s in range(len(lens))]


# ---- every choice ------------------------------------------------------------------------------
def occurrences_by_stream(rows):
    """stream -> {id: [(start, end_exclusive)]}."""
    out = {}
    for s, a, b, g in np.asarray(rows).tolist():
        out.setdefault(s, {}).setdefault(g, []).append((a, b))
    return out


class _Streams:
    """Per stream what derived_rules reads of its occurrences, from sorted
    arrays: get(j) is {id: (smallest end_exclusive, the start and end_exclusive
    of the occurrence that begins last, how many)}."""

    def __init__(self, rows, nseg):
        r = rows[np.lexsort((rows[:, 1], rows[:, 3], rows[:, 0]))]  # by (stream, id, start): one id's ends ascend too
        self.rows, self.nseg = r, nseg
        new = np.concatenate([[True], (r[1:, 0] != r[:-1, 0]) | (r[1:, 3] != r[:-1, 3])]) if len(r) else np.zeros(0, bool)
        at = np.nonzero(new)[0]
        end = np.append(at[1:], len(r)) - 1
        self.key = r[at][:, [0, 3]]
        self.val = np.stack([r[at, 2], r[end, 1], r[end, 2], end - at + 1], axis=1)
        self.cut = np.searchsorted(self.key[:, 0], np.arange(nseg + 1))
        self.row_cut = np.searchsorted(r[:, 0], np.arange(nseg + 1))

    def get(self, j):
        if not 0 <= j < self.nseg:
            return {}
        a, b = self.cut[j], self.cut[j + 1]
        return dict(zip(self.key[a:b, 1].tolist(), map(tuple, self.val[a:b].tolist())))

    def touching(self, j):
        """The (U, T) of stream j of which an occurrence of T begins at the
        last byte of one of U, ascending."""
        r = self.rows[self.row_cut[j]:self.row_cut[j + 1]]
        by_end = r[np.argsort(r[:, 2], kind="stable")]
        lo = np.searchsorted(by_end[:, 2], r[:, 1] + 1, side="left")
        hi = np.searchsorted(by_end[:, 2], r[:, 1] + 1, side="right")
        pairs = {(int(u), int(t)) for a, b, t in zip(lo.tolist(), hi.tolist(), r[:, 3].tolist()) if b > a
                 for u in by_end[a:b, 3].tolist()}
        return sorted(pairs)

    def first_from(self, j, T, bound):
        """The smallest end_exclusive of the occurrences of T in stream j that
        begin at or behind bound, or None."""
        r = self.rows[self.row_cut[j]:self.row_cut[j + 1]]
        ends = r[(r[:, 3] == T) & (r[:, 1] >= bound), 2]
        return int(ends.min()) if len(ends) else None


def product_size(occ_of_stream, rule):
    n = 1
    for g, _ in rule:
        if g > 0:
            n *= len(occ_of_stream.get(g, ()))
    return n


def exhaustive_seq(occ_of_stream, rule):
    """The hit of an ordered rule in one stream as end_exclusive, or None:
    itertools.product over one occurrence per positive term, the choices that
    satisfy every link, the minimum over them of the largest end."""
    if any(occ_of_stream.get(-g) for g, _ in rule if g < 0):
        return None
    positive = [(g, gap) for g, gap in rule if g > 0]
    best = None
    for choice in itertools.product(*(occ_of_stream.get(g, ()) for g, _ in positive)):
        if all(gap is None or choice[i][0] >= choice[i - 1][1] + gap for i, (_, gap) in enumerate(positive)):
            end = max(b for _, b in choice)
            best = end if best is None else min(best, end)
    return best


# ---- rules from what the streams hold ----------------------------------------------------------
def named_streams(lens):
    """The head streams of 1 to 17 bytes, then the neighbours of empty streams."""
    lens = np.asarray(lens)
    nseg = len(lens)
    first = [j for j in range(min(nseg, 22)) if 1 <= lens[j] <= 17]
    for j in np.nonzero(lens == 0)[0].tolist():
        first += [k for k in (j - 1, j + 1) if 0 <= k < nseg and lens[k] > 0]
    return list(dict.fromkeys(first))


def _stream_order(lens):
    """Every stream once: the named streams first, then the others spread over
    the offset array."""
    nseg = len(lens)
    step = next(k for k in range(max(nseg // 3, 1) | 1, 2 * nseg + 3, 2) if np.gcd(k, nseg) == 1)
    order = list(dict.fromkeys(named_streams(lens) + [(5 + step * k) % nseg for k in range(nseg)]))
    assert sorted(order) == list(range(nseg))
    return order


def derived_rules(rows, nseg, rng, lens, before=None, nrandom=100, pairs=()):
    """Rules built from rows whose id is a gid.  Returns a dict: rules (the
    unordered ones, rule_inputs' form) and seq (the ordered ones,
    seq_rule_inputs' form), fast and seq_fast (a gid or None per rule),
    plan and seq_plan: lists of (kind, stream, rule, end_exclusive of the hit
    the rows give there, or None for a rule that must not fire there), and
    streams, the streams that gave a rule.  before: the bytes every flow had
    before the call (a call-2 list; it adds the kinds of CALL2).  pairs: (g, h)
    gid pairs that get a rule wherever both occur (kinds of CASE_PAIR).  At
    most PER_KIND rules of a kind once MIN_STREAMS streams gave one; a named
    stream (head, neighbour of an empty one) gives a one-term rule whatever it
    holds (kind "single").  nrandom random rules of each sort over the list's
    most frequent gids follow the derived ones, PM_RULE_FAST drawn for half."""
    occ = _Streams(rows, nseg)
    allg = np.unique(rows[:, 3])
    rules, seq, plan, seq_plan, made, used = [], [], [], [], {}, set()

    def room(kind):
        return made.get(kind, 0) < PER_KIND or len(used) < MIN_STREAMS

    def add(kind, j, rule, end, ordered):
        (seq if ordered else rules).append(rule)
        (seq_plan if ordered else plan).append((kind, j, len(seq if ordered else rules) - 1, end))
        made[kind] = made.get(kind, 0) + 1
        used.add(j)

    kinds = FIRING + NOT_FIRING + AA[:1] + (CALL2 if before is not None else ()) + (CASE_PAIR[:1] if pairs else ())
    order = _stream_order(lens)
    named = set(named_streams(lens))
    for j in order:
        if not any(room(kind) for kind in kinds):
            break
        o = occ.get(j)
        P = [int(g) for g in rng.permutation(sorted(o))][:24]
        first = {g: v[0] for g, v in o.items()}
        if P and j in named:  # whatever a named stream holds, it gives a rule
            add("single", j, [P[0]], first[P[0]], False)
            add("single", j, [(P[0], None)], first[P[0]], True)
        last = {g: v[1:3] for g, v in o.items()}  # the occurrence that begins last

        def far(o, U, T):
            """The largest distance at which T follows U, and T's end then."""
            return last[T][0] - first[U], last[T][1]

        if len(P) >= 2:
            pos = P[:min(int(rng.integers(2, 5)), max(len(P) - 1, 2))]  # (a present pattern is left to negate)
            end = max(first[g] for g in pos)
            rest = [g for g in P if g not in pos]
            if room("unordered"):
                add("unordered", j, list(pos), end, False)
            if rest and room("neg_present"):
                add("neg_present", j, pos + [-rest[0]], None, False)
            absent = [int(g) for g in rng.choice(allg, size=min(8, len(allg)), replace=False) if int(g) not in o]
            if absent and room("neg_absent"):
                add("neg_absent", j, pos + [-absent[0]], end, False)
        # ordered pairs: every (U, T) with T beginning at or behind the first end of U
        good = [(U, T) for U in P for T in P if U != T and far(o, U, T)[0] >= 0]
        if good and room("pair_max"):
            U, T = good[0]
            d, end = far(o, U, T)
            add("pair_max", j, [(U, None), (T, d)], end, True)
            add("pair_plus1", j, [(U, None), (T, d + 1)], None, True)
        twice = [g for g in P if far(o, g, g)[0] >= 0]
        if twice and room("aa_exact"):
            d, end = far(o, twice[0], twice[0])
            add("aa_exact", j, [(twice[0], None), (twice[0], d)], end, True)
            add("aa_plus1", j, [(twice[0], None), (twice[0], d + 1)], None, True)
        # an occurrence of T begins at the last byte of one of U: at distance 0 the rule does not fire from
        # those two.  First the pairs whose best occurrences do so (far == -1: it fires nowhere in the
        # stream), else any such pair, with the hit the stream's other occurrences give
        if room("overlap"):
            lap = occ.touching(j)
            if lap:
                U, T = next((p for p in lap if far(o, *p)[0] == -1), lap[0])
                add("overlap", j, [(U, None), (T, 0)], occ.first_from(j, T, first[U]), True)
        if room("chain3"):
            for U, T in good:
                V = [g for g in P if g not in (U, T) and last[g][0] >= far(o, U, T)[1]]
                if V:
                    d1, e1 = far(o, U, T)
                    v = last[V[0]]
                    add("chain3", j, [(U, None), (T, d1), (V[0], v[0] - e1)], v[1], True)
                    break
        if room("two_chains"):
            # (the second head is in neither term of the first chain; its follower may repeat one)
            two = next(((a, b) for a in good[:40] for b in good[:40]
                        if b[0] not in a and b[1] != a[0] and far(o, *b)[1] > far(o, *a)[1]), None)
            if two:
                (U, T), (X, Y) = two
                add("two_chains", j, [(U, None), (T, far(o, U, T)[0]), (X, None), (Y, far(o, X, Y)[0])],
                    far(o, X, Y)[1], True)
            else:  # a second chain of one term, as a stream of three patterns allows
                one = next(((a, X) for a in good[:40] for X in P if X not in a and first[X] > far(o, *a)[1]), None)
                if one:
                    (U, T), X = one
                    add("two_chains", j, [(U, None), (T, far(o, U, T)[0]), (X, None)], first[X], True)
        if before is not None:
            early = [g for g in P if o[g][3] == 1 and o[g][1] < before[j]]
            head = [(U, T) for U in early for T in P if T != U and far(o, U, T)[0] >= 0]
            if head and room("straddle_head"):
                U, T = head[0]
                d, end = far(o, U, T)
                add("straddle_head", j, [(U, None), (T, d)], end, True)
            # the head ends in this call's bytes, the follower begins before them
            tail = [(U, T) for T in early for U in P if U != T]
            if tail and room("straddle_follower"):
                add("straddle_follower", j, [(tail[0][0], None), (tail[0][1], 0)], None, True)
        # a pattern of this stream with one that only a neighbouring stream holds (the next one, else the
        # one before); where there is one, a pattern of this stream that the neighbour lacks, so that the
        # rule's terms lie in the two streams only
        for nxt in (occ.get(j + 1), occ.get(j - 1)):
            theirs = [int(g) for g in sorted(nxt) if g not in o]
            if P and theirs and room("adjacent"):
                mine = [g for g in P if g not in nxt] + P
                add("adjacent", j, [mine[0], theirs[0]], None, False)
                add("adjacent", j, [(mine[0], None), (theirs[0], 0)], None, True)
                made["adjacent"] -= 1
                break
        for g, h in pairs:
            if g in o and h in o and room("case_pair"):
                add("case_pair", j, [g, h], max(first[g], first[h]), False)
                d, end = far(o, g, h)
                add("case_pair_seq", j, [(g, None), (h, max(d, 0))], end if d >= 0 else None, True)
    counts = np.bincount(rows[:, 3])
    top = [int(g) for g in np.argsort(-counts, kind="stable")[:8] if counts[g]]
    rules += random_rules(rng, nrandom, top)
    seq += random_seq_rules(rng, nrandom, top, max_gap=30)
    fast = [None if rng.random() < 0.5 else int(rng.choice([g for g in r if g > 0])) for r in rules]
    seq_fast = [None if rng.random() < 0.5 else int(rng.choice([g for g, _ in r if g > 0])) for r in seq]
    return dict(rules=rules, seq=seq, fast=fast, seq_fast=seq_fast, plan=plan, seq_plan=seq_plan, streams=sorted(used))


def _ids_by_stream(rows):
    """stream -> the set of ids that occur in it."""
    keys = np.unique((rows[:, 0] << 32) | rows[:, 3])
    out = {}
    for s, g in zip((keys >> 32).tolist(), (keys & 0xFFFFFFFF).tolist()):
        out.setdefault(s, set()).add(g)
    return out


def derived_flow_rules(rows_a, rows_b, nseg, rng, nrandom=100):
    """Unordered rules over the two calls of every flow, from rows whose id is
    a gid.  Returns (rules, plan); plan: (kind, stream, rule) with kind
      carried   a term of call 1 with one only call 2 has: completes in call 2
      neg_call1 a term of call 2 (one only call 2 has where there is one), negated one only call 1 has: never hits
      once      two terms of call 1, one of them again in call 2 where there is one: hits in call 1 only
    and nrandom random rules over the most frequent gids of both lists."""
    A, B = _ids_by_stream(rows_a), _ids_by_stream(rows_b)
    rules, plan, made = [], [], {}

    def add(kind, j, rule):
        if made.get(kind, 0) < PER_KIND:
            rules.append(rule)
            plan.append((kind, j, len(rules) - 1))
            made[kind] = made.get(kind, 0) + 1

    for j in rng.permutation(nseg).tolist():
        a, b = set(A.get(j, ())), set(B.get(j, ()))
        only_a, only_b, both = sorted(a - b), sorted(b - a), sorted(a & b)
        if a and only_b:
            add("carried", j, [int(rng.choice(sorted(a))), int(rng.choice(only_b))])
        if only_a and b:
            add("neg_call1", j, [int(rng.choice(only_b if only_b else sorted(b))), -int(rng.choice(only_a))])
        if len(a) >= 2:
            x = int(rng.choice(both if both else sorted(a)))
            add("once", j, [x, int(rng.choice([g for g in sorted(a) if g != x]))])
    counts = np.bincount(np.concatenate([rows_a[:, 3], rows_b[:, 3]]))
    top = [int(g) for g in np.argsort(-counts, kind="stable")[:12] if counts[g]]
    return rules + random_rules(rng, nrandom, top, max_pos=3, negated=0.35), plan


def shown(plan, ptr, hits, offs, before=None):
    """kind -> [number of planned rules the result (rule_ptr, hits) shows: the
    rule fires in its stream at the derived byte, or, where it must not fire
    there, does not; the number planned]."""
    offs = np.asarray(offs, dtype=np.int64)
    out = {}
    for kind, j, r, end in plan:
        mine = hits[ptr[j]:ptr[j + 1]]
        got = [int(h) >> GID_BITS for h in mine[(mine & np.uint64((1 << GID_BITS) - 1)) == np.uint64(r)].tolist()]
        want = [] if end is None else [int(offs[j]) + end - 1 - (0 if before is None else int(before[j]))]
        n = out.setdefault(kind, [0, 0])
        n[0] += got == want
        n[1] += 1
    return out


# ---- the expected values of the two test files, made once ---------------------------------------
_lists, _flows = {}, {}
FLOW_ROWS_SEED = 77


def _seed(*parts):
    import zlib
    return zlib.crc32("-".join(parts).encode())


def expected(c, which, form, code_of_gid, nrandom=100):
    """Of one list of a fuzz case: rows (ids are gids), before (None for text
    "a"), derived (derived_rules' dict), rules and seq (the expected (rule_ptr,
    hits) of the rules call and the ordered-rules call).  Cached per (case,
    text, form); callers do not modify it."""
    k = (c.key, which, form)
    if k in _lists:
        assert np.array_equal(_lists[k]["code_of_gid"], code_of_gid), "another code-to-gid map than the cached values have"
    else:
        rows = to_gids(occurrences(c, which, form), code_of_gid)
        lens = np.diff(c.offs)
        before = None if which == "a" else lens
        d = derived_rules(rows, c.nseg, np.random.default_rng(_seed(*k)), lens, before, nrandom)
        by = _ById(rows, c.nseg)  # (sorted once for both)
        _lists[k] = dict(rows=rows, before=before, derived=d, code_of_gid=np.array(code_of_gid),
                         rules=rules_from_text(by, c.nseg, d["rules"], c.offs, before),
                         seq=seq_rules_from_text(by, c.nseg, d["seq"], c.offs, before))
    return _lists[k]


def expected_flow(c, form, code_of_gid, nrandom=100):
    """Of the two flow calls of a form: rules, plan (derived_flow_rules'),
    flow (the whole flows' rows), calls (the expected (rule_ptr, hits) of call
    1 and call 2), held (per stream the term gids the flow's text holds),
    d_rows (the fixed permutation of the rows)."""
    k = (c.key, form)
    a = expected(c, "a", form, code_of_gid)["rows"]  # (checks the map against the cached one)
    b = expected(c, "b", form, code_of_gid)["rows"]
    if k not in _flows:
        lens = np.diff(c.offs)
        rules, plan = derived_flow_rules(a, b, c.nseg, np.random.default_rng(_seed(*k, "flow")), nrandom)
        flow = np.concatenate([a, b])
        zero = np.zeros(c.nseg, np.int64)
        _flows[k] = dict(rules=rules, plan=plan, flow=flow,
                         calls=[flow_rules_from_text(flow, zero, lens, rules), flow_rules_from_text(flow, lens, lens, rules)],
                         held=flow_bits_from_text(flow, lens, lens, rules),
                         d_rows=np.random.default_rng(FLOW_ROWS_SEED).permutation(c.nseg).astype(np.int64))
    return _flows[k]


_nocase = {}


def expected_nocase(gid_of_index):
    """Of nocase_inputs.fuzz_dictionary(0) with flags crc32 & 1 over two texts
    of 49,152 bytes, B continuing A: pats, flags, A, B, offs, pairs (the gid
    pairs of patterns equal up to case whose flags differ), began_before (the
    events of call 2 whose match began in call 1) and, per text "a" / "b",
    expected()'s dict.  gid_of_index: the gid of the k-th added pattern."""
    if _nocase:
        assert np.array_equal(_nocase["gid_of_index"], gid_of_index), "other gids than the cached values have"
    else:
        from nocase_inputs import brute, flag_of, fold, fuzz_dictionary, fuzz_text, stream_offsets
        pats = fuzz_dictionary(0)
        flags = [flag_of(p) for p in pats]
        A, B = fuzz_text(pats, 0, 49152), fuzz_text(pats, 50, 49152)
        offs = stream_offsets(len(A), 0)
        nseg, lens = len(offs) - 1, np.diff(offs)
        whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
        found, stats = brute(pats, flags, whole, gid_of_index, 1)
        assert stats["rejected"] > 0
        last = {p: k for k, p in enumerate(pats)}  # (a byte string added twice: the later add wins)
        pairs = [(int(gid_of_index[k]), int(gid_of_index[q])) for p, k in last.items() for r, q in last.items()
                 if k != q and fold(p) == fold(r) and flags[k] != flags[q]]
        _nocase.update(gid_of_index=np.array(gid_of_index), pats=pats, flags=flags, A=A, B=B, offs=offs, pairs=pairs)
        for which, before in (("a", None), ("b", lens)):
            rows = nocase_occurrences(found, lens, which)
            d = derived_rules(rows, nseg, np.random.default_rng(_seed("nocase", which)), lens, before, pairs=pairs)
            by = _ById(rows, nseg)
            _nocase[which] = dict(rows=rows, before=before, derived=d,
                                  rules=rules_from_text(by, nseg, d["rules"], offs, before),
                                  seq=seq_rules_from_text(by, nseg, d["seq"], offs, before))
        b = _nocase["b"]["rows"]
        _nocase["began_before"] = int(np.count_nonzero(b[:, 1] < lens[b[:, 0]]))
    return _nocase
