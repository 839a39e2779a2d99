"""Reference and generators of the flow-rules tests (test_flow_rules.py on the
GPU, test_flow_rules_cpu.py without one).  TEST INFRASTRUCTURE; no device,
nothing here calls the library.

A rule is a list of ints: g is a positive term (gid g), -g a negated one.
reference_flow_rules() is the dict-and-set statement of include/pm_hip.h "flow
rules": per flow a set C of carried gids; per call N, the term gids the
flow's stream holds that C lacks, each at its first position.  A rule hits iff
every positive term is in C u N, at least one is in N and no negated term is
in C u N, at the largest first position of its positive terms in N; then N
joins C (not under keep).
"""
import numpy as np

from rule_inputs import GID_BITS, GID_MAX, random_rules

NO_BIT = 0xFFFFFFFF


def rule_bits(rules):
    """gid -> bit: the rank among the distinct gids of all terms, ascending."""
    return {g: b for b, g in enumerate(sorted({abs(t) for r in rules for t in r}))}


def words_of(rules):
    return max(1, (len(rule_bits(rules)) + 63) // 64)


def sets_array(carried, rules, nrows):
    """The (nrows, W) u64 sets of a {row: set of gids} state."""
    bit = rule_bits(rules)
    sets = np.zeros((nrows, words_of(rules)), dtype=np.uint64)
    for row, gids in carried.items():
        for g in gids:
            sets[row, bit[g] >> 6] |= np.uint64(1 << (bit[g] & 63))
    return sets


def reference_flow_rules(events, offsets, rules, carried, nrows, rows=None, keep=False, trace=None):
    """(rule_ptr int64 of nseg + 1, hits u64 of position << 24 | rule), each
    stream's range ascending.  carried: {row: set of term gids}, updated in
    place unless keep.  The stream of a position is the first offset above it,
    minus one; events outside every stream, of a gid that no term names or in
    a stream whose row lies outside [0, nrows) are dropped.  trace, a list,
    gets one record per stream with new terms: (stream, row, N, [(rule, kind)])
    with kind "hit", "carried_negation" or "new_negation" for every rule whose
    positive terms are complete with one of them new."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    named = {abs(t) for r in rules for t in r}
    pos = (events >> np.uint64(GID_BITS)).astype(np.int64)
    gid = (events & np.uint64(GID_MAX)).astype(np.int64)
    j = np.searchsorted(offs, pos, side="right") - 1
    keep_ev = (j >= 0) & (j < nseg)
    new = {}
    for s, g, p in zip(j[keep_ev].tolist(), gid[keep_ev].tolist(), pos[keep_ev].tolist()):
        row = s if rows is None else int(rows[s])
        if g not in named or not 0 <= row < nrows or g in carried.get(row, ()):
            continue
        first = new.setdefault(s, {})
        first[g] = min(first.get(g, p), p)
    ptr = np.zeros(nseg + 1, dtype=np.int64)
    hits = []
    for s in range(nseg):
        N = new.get(s)
        if N:
            row = s if rows is None else int(rows[s])
            C = carried.get(row, set())
            mine, kinds = [], []
            for r, rule in enumerate(rules):
                positive = [t for t in rule if t > 0]
                if not all(t in C or t in N for t in positive) or not any(t in N for t in positive):
                    continue
                if any(-t in C for t in rule if t < 0):
                    kinds.append((r, "carried_negation"))
                elif any(-t in N for t in rule if t < 0):
                    kinds.append((r, "new_negation"))
                else:
                    kinds.append((r, "hit"))
                    mine.append((max(N[t] for t in positive if t in N) << GID_BITS) | r)
            hits += sorted(mine)
            if trace is not None:
                trace.append((s, row, dict(N), kinds))
        ptr[s + 1] = len(hits)
    if not keep:
        for s, N in new.items():
            row = s if rows is None else int(rows[s])
            carried.setdefault(row, set()).update(N)
    return ptr, np.array(hits, dtype=np.uint64)


def pack(pos, gid):
    return (np.asarray(pos, dtype=np.uint64) << np.uint64(GID_BITS)) | np.asarray(gid, dtype=np.uint64)


def flow_case(seed, nflows=40, ngid=14, nrules=80, negated=0.35, max_calls=4, gid_pool=None):
    """Flows cut into calls.  Every flow has a length, events (flow position,
    gid) -- some positions shared by two gids -- and 1 to max_calls cuts; call
    c holds segment c of every flow that has one, in shuffled stream order,
    each stream's row given by a permutation (rows beyond the flows stay
    untouched), beside streams whose row lies out of range and events outside
    every stream.  Some segments are empty, and the third call is an extra one
    without a byte or an event.
    Returns a dict: rules, nrows, flow_len, flow_events [(pos, gid)], calls --
    a list of dicts events, offsets, rows, flow (the flow of each stream, -1
    for an inert one) and base (the flow position of each stream's first
    byte)."""
    rng = np.random.default_rng(seed)
    pool = np.arange(1, ngid + 1) if gid_pool is None else np.asarray(gid_pool)
    rules = random_rules(rng, nrules, pool, max_pos=3, negated=negated)
    nrows = nflows + 3
    row_of = rng.permutation(nrows)[:nflows]
    flow_len, flow_events, cuts = [], [], []
    for f in range(nflows):
        L = int(rng.integers(0, 60))
        n = int(rng.integers(0, 9)) if L else 0
        p = rng.integers(0, max(L, 1), size=n)
        g = rng.choice(pool, size=n)
        twin = rng.random(n) < 0.3  # a second gid at the same position
        p = np.concatenate([p, p[twin]])
        g = np.concatenate([g, rng.choice(pool, size=int(twin.sum()))])
        flow_len.append(L)
        flow_events.append((p.astype(np.int64), g.astype(np.int64)))
        k = int(rng.integers(1, max_calls + 1))
        cuts.append(np.concatenate([[0], np.sort(rng.integers(0, L + 1, size=k - 1)), [L]]).astype(np.int64))
    calls = []
    for c in range(max_calls):
        flows = [f for f in range(nflows) if len(cuts[f]) - 1 > c]
        order = rng.permutation(len(flows)).tolist()
        stream_flow = [flows[i] for i in order] + [-1, -1]
        lens = [int(cuts[f][c + 1] - cuts[f][c]) for f in stream_flow[:-2]] + [7, 5]
        base = int(rng.integers(1, 500))
        offs = base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = [int(row_of[f]) for f in stream_flow[:-2]] + [-1, nrows + int(rng.integers(0, 5))]
        ev_pos, ev_gid = [offs[0] - 1, offs[-1], offs[-1] + 3], [int(pool[0])] * 3  # outside every stream
        for j, f in enumerate(stream_flow):
            if f < 0:
                ev_pos += [int(offs[j]), int(offs[j + 1]) - 1]
                ev_gid += [int(pool[0]), int(pool[-1])]
                continue
            p, g = flow_events[f]
            inside = (p >= cuts[f][c]) & (p < cuts[f][c + 1])
            ev_pos += (offs[j] + p[inside] - cuts[f][c]).tolist()
            ev_gid += g[inside].tolist()
        mix = rng.permutation(len(ev_pos))
        calls.append(dict(events=pack(np.array(ev_pos, dtype=np.int64)[mix], np.array(ev_gid, dtype=np.int64)[mix]),
                          offsets=offs, rows=np.array(rows, dtype=np.int64), flow=stream_flow,
                          base=[int(cuts[f][c]) if f >= 0 else 0 for f in stream_flow]))
    # an empty call in the middle: five flows' streams without a byte, and no event
    idle = list(range(min(5, nflows)))
    calls.insert(2, dict(events=np.empty(0, dtype=np.uint64), offsets=np.full(len(idle) + 1, 77, dtype=np.int64),
                         rows=np.array([int(row_of[f]) for f in idle], dtype=np.int64), flow=idle, base=[0] * len(idle)))
    return dict(rules=rules, nrows=nrows, flow_len=flow_len, flow_events=flow_events, calls=calls, row_of=row_of)


def kinds_of_case(case):
    """The reference over the case's calls, with what the non-vacuity checks
    count: a dict of kind -> occurrences.
      all_new_later      a hit in a call after the first, none of its positive terms carried
      carried_positive   a hit with at least one positive term carried
      carried_negation   positives complete in a call, a negated term carried from an earlier one
      negation_after     positives complete, a negated term first in this call behind the completing byte
      tie                a hit two of whose new positive terms share the first position
      negation_next_call a hit in one call, a negated term of the rule new to the flow in a later one
    and the per-call (rule_ptr, hits, sets after the call)."""
    rules, nrows = case["rules"], case["nrows"]
    carried = {}
    count = dict(all_new_later=0, carried_positive=0, carried_negation=0, negation_after=0, tie=0, negation_next_call=0)
    results = []
    hit_so_far = {}  # row -> the rules that hit in the flow's earlier calls
    for c, call in enumerate(case["calls"]):
        before = {row: set(g) for row, g in carried.items()}
        trace = []
        ptr, hits = reference_flow_rules(call["events"], call["offsets"], rules, carried, nrows, call["rows"],
                                         trace=trace)
        now = set()
        for s, row, N, kinds in trace:
            C = before.get(row, set())
            for r in hit_so_far.get(row, ()):
                if any(-t in N for t in rules[r] if t < 0):
                    count["negation_next_call"] += 1
            for r, kind in kinds:
                positive = [t for t in rules[r] if t > 0]
                firsts = sorted(N[t] for t in positive if t in N)
                if kind == "hit":
                    now.add((row, r))
                    if any(t in C for t in positive):
                        count["carried_positive"] += 1
                    elif c > 0:
                        count["all_new_later"] += 1
                    if len(firsts) != len(set(firsts)):
                        count["tie"] += 1
                elif kind == "carried_negation":
                    count["carried_negation"] += 1
                elif all(N[-t] > firsts[-1] for t in rules[r] if t < 0 and -t in N):
                    count["negation_after"] += 1
        for row, r in now:
            hit_so_far.setdefault(row, set()).add(r)
        results.append((ptr, hits, sets_array(carried, rules, nrows)))
    return count, results
