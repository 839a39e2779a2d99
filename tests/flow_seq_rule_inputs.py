"""Reference and generators of the flow ordered-rules tests
(test_flow_seq_rules.py on the GPU, test_flow_seq_rules_cpu.py without one).
TEST INFRASTRUCTURE; no device, nothing here calls the library.

A rule is seq_rule_inputs' list of (g, gap) pairs.  The reference keeps, per
row, every occurrence the flow has had so far, as flow positions.  Per call it
evaluates every rule over the flow's whole prefix by seq_rule_inputs'
rule_in_stream (the feasible sets, level by level: no greedy argument and no
carried state) and keeps the hits whose position lies in this call's bytes
(include/pm_hip.h "flow ordered rules").  The expected rows come from the
layout's definition over the same prefix.
"""
import numpy as np

from seq_rule_inputs import GID_BITS, GID_MAX, chains_of, pack, random_seq_rules, rule_in_stream

NO_WORD = 0xFFFFFFFF
MAX_BYTES = 1 << 57


def layout_of(rules):
    """(chain_word: {(rule, term index): word} for the heads of the chains of
    two or more positive terms, numbered by rule and then by the head's place;
    bit: {gid: bit}, the rank among the gids of one-term chains and negated
    terms, ascending; C; K; S)."""
    chain_word, bit_gids, c = {}, set(), 0
    for r, rule in enumerate(rules):
        heads = [i for i, (g, gap) in enumerate(rule) if g > 0 and gap is None]
        for h in heads:
            n = 1
            for g, gap in rule[h + 1:]:
                if g < 0:
                    continue
                if gap is None:
                    break
                n += 1
            if n >= 2:
                chain_word[(r, h)] = c
                c += 1
            else:
                bit_gids.add(rule[h][0])
        bit_gids |= {-g for g, _ in rule if g < 0}
    bit = {g: b for b, g in enumerate(sorted(bit_gids))}
    return chain_word, bit, c, len(bit), max(1, c + (len(bit) + 63) // 64)


def chain_progress(occ, chain, plen):
    """The word of a chain over a flow's occurrences (gid -> ascending array):
    0, or (E + 1) << 6 | k for the deepest level k with a feasible occurrence,
    E the smallest of them."""
    feasible = np.asarray(occ.get(chain[0][0], ()), dtype=np.int64)
    if not len(feasible):
        return 0
    k = 0
    for g, d in chain[1:]:
        o = np.asarray(occ.get(g, ()), dtype=np.int64)
        nxt = o[(feasible[:, None] + d + int(plen[g]) <= o[None, :]).any(axis=0)] if len(o) else o
        if not len(nxt):
            break
        feasible = nxt
        k += 1
    return ((int(feasible.min()) + 1) << 6) | k


def rows_array(state, rules, plen, nrows):
    """The (nrows, S) u64 rows of a {row: {gid: set of flow positions}} state."""
    chain_word, bit, C, _, S = layout_of(rules)
    prog = np.zeros((nrows, S), dtype=np.uint64)
    for row, seen in state.items():
        occ = {g: np.array(sorted(v), dtype=np.int64) for g, v in seen.items() if v}
        for r, rule in enumerate(rules):
            chains, _ = chains_of(rule)
            heads = [i for i, (g, gap) in enumerate(rule) if g > 0 and gap is None]
            for h, chain in zip(heads, chains):
                if (r, h) in chain_word:
                    prog[row, chain_word[(r, h)]] = np.uint64(chain_progress(occ, chain, plen))
        for g in occ:
            if g in bit:
                prog[row, C + (bit[g] >> 6)] |= np.uint64(1 << (bit[g] & 63))
    return prog


def reference_flow_seq_rules(state, events, offsets, pos_in, rules, plen, nrows, rows=None, keep=False):
    """(rule_ptr int64 of nseg + 1, hits u64 of position << 24 | rule), each
    stream's range ascending, the positions buffer-global.  state: {row: {gid:
    set of flow positions}}, updated in place unless keep.  Events outside
    every stream or in an inert stream (a row outside [0, nrows), pos_in +
    length above 2^57) are dropped."""
    events = np.asarray(events, dtype=np.uint64)
    offs = np.asarray(offsets, dtype=np.int64)
    nseg = len(offs) - 1
    pos = (events >> np.uint64(GID_BITS)).astype(np.int64)
    gid = (events & np.uint64(GID_MAX)).astype(np.int64)
    j = np.searchsorted(offs, pos, side="right") - 1
    inside = (j >= 0) & (j < nseg)
    new = {}
    for s, g, p in zip(j[inside].tolist(), gid[inside].tolist(), pos[inside].tolist()):
        new.setdefault(s, {}).setdefault(g, set()).add(p - int(offs[s]) + int(pos_in[s]))
    ptr = np.zeros(nseg + 1, dtype=np.int64)
    hits = []
    for s in range(nseg):
        row = s if rows is None else int(rows[s])
        live = 0 <= row < nrows and int(pos_in[s]) + int(offs[s + 1] - offs[s]) <= MAX_BYTES
        if s in new and live:
            seen = {g: set(v) for g, v in state.get(row, {}).items()}
            for g, v in new[s].items():
                seen.setdefault(g, set()).update(v)
            occ = {g: np.array(sorted(v), dtype=np.int64) for g, v in seen.items()}
            mine = []
            for r, rule in enumerate(rules):
                p = rule_in_stream(occ, rule, plen)
                if p is not None and p >= int(pos_in[s]):  # in this call's bytes
                    mine.append(((p - int(pos_in[s]) + int(offs[s])) << GID_BITS) | r)
            hits += sorted(mine)
            if not keep:
                state[row] = seen
        ptr[s + 1] = len(hits)
    return ptr, np.array(hits, dtype=np.uint64)


# ---- the planted kinds ----------------------------------------------------------------
# gids 1..5 are A, B, C, D, E; a planted flow has 4 * SEG bytes in two, three or four calls: the first
# calls have SEG bytes each and the last one has the rest.
SEG = 100
KINDS = ("head_then_follower", "too_close_then_ok", "chain_of_three", "two_levels_one_call", "aa_across_cut",
         "straddle", "overlap_across_cut", "two_chains_two_calls", "carried_negation", "negation_behind",
         "negation_later", "done_suppressed")


def planted_cuts(ncalls):
    assert ncalls in (2, 3, 4)
    return np.array([SEG * c for c in range(ncalls)] + [4 * SEG], dtype=np.int64)


def planted_flows(rng, plen, ncalls=4):
    """(rules 0..5, flows, plan): flows a list of [(flow position, gid)], plan
    kind -> (flow, rule, (call, flow position) of the one expected hit, or
    None for a rule that never fires in the flow), for planted flows cut into
    ncalls calls (planted_cuts).  In two calls the chain of three ends in
    call 2, and the later negation follows a hit of call 1."""
    A, B, C, D, E = 1, 2, 3, 4, 5
    LA, LB = int(plen[A]), int(plen[B])
    assert LB >= 2 and max(LA, LB) <= 8
    dist = int(rng.integers(1, 40))
    rules = [[(A, None), (B, 0)], [(A, None), (B, dist)], [(A, None), (B, 0), (C, 0)], [(A, None), (A, dist)],
             [(A, None), (B, 0), (C, None), (D, 0)], [(A, None), (-E, None), (B, 0)]]
    flows, plan = [], {}

    cuts = planted_cuts(ncalls)

    def flow(kind, rule, expect, ev):
        if expect is not None:  # the call that holds the expected position
            expect = (int(np.searchsorted(cuts, expect[1], side="right")) - 1, expect[1])
        plan[kind] = (len(flows), rule, expect)
        flows.append(ev)

    flow("head_then_follower", 0, (1, 150), [(50, A), (150, B)])
    # B is there in call 1, one byte too close; only the B of call 2 satisfies the link
    flow("too_close_then_ok", 1, (1, 160), [(40, A), (40 + dist + LB - 1, B), (160, B)])
    flow("chain_of_three", 2, (2, 250), [(50, A), (150, B), (250, C)])
    flow("two_levels_one_call", 2, (1, 140), [(50, A), (120, B), (140, C)])
    flow("aa_across_cut", 3, (1, 110 + dist + LA), [(50, A), (110 + dist + LA, A)])
    # B begins in call 1 and ends at the first byte of call 2
    flow("straddle", 0, (1, SEG), [(50, A), (SEG, B)])
    # A ends at the last byte of call 1 and B begins at that byte: it ends in call 2, one byte short
    flow("overlap_across_cut", 0, None, [(SEG - 1, A), (SEG + LB - 2, B)])
    flow("two_chains_two_calls", 4, (1, 150), [(20, A), (40, B), (60, C), (150, D)])
    flow("carried_negation", 5, None, [(30, E), (50, A), (150, B)])
    flow("negation_behind", 5, None, [(50, A), (120, B), (180, E)])
    if ncalls == 2:
        flow("negation_later", 5, (0, 60), [(50, A), (60, B), (250, E)])
    else:
        flow("negation_later", 5, (1, 150), [(50, A), (150, B), (250, E)])
    # complete and suppressed in call 1; A and B again in call 2 must give nothing
    flow("done_suppressed", 5, None, [(50, A), (60, B), (70, E), (120, A), (150, B)])
    return rules, flows, plan


def flow_seq_case(seed, nflows=24, ngid=10, nrules=40, max_calls=4, big_base=0, cut_seed=0, real=None,
                  planted_calls=4):
    """Flows cut into calls: the planted flows (planted_calls calls: 2, 3 or 4) and
    nflows random ones (1 to max_calls cuts, lengths below 60, some positions
    shared by two gids).  Call c holds segment c of every flow that has one,
    in shuffled stream order, each stream's row given by a permutation (spare
    rows stay untouched), beside three inert streams -- a row of -1, one past
    nrows, and a spare row with pos_in past 2^57 -- and events outside every
    stream.  big_base is added to every flow's byte count.  cut_seed chooses
    the random flows' cuts and the calls' order, rows and offsets, and nothing
    else: the same seed with another cut_seed is the same flows cut elsewhere.
    real = (gid_map, plen): the case over a real dictionary's gids: gid g of the
    generator becomes gid_map[g], whose length plen[gid_map[g]] must be at
    most 8 (at least 2 for g = 2); the case's plen is then the real one.
    Returns a dict: rules, plen, nrows, plan, row_of, calls -- a list of dicts
    events, offsets, rows, pos_in, flow (the flow of each stream, -1: inert)."""
    rng = np.random.default_rng(seed)
    plen = np.concatenate([[0], rng.integers(1, 9, size=ngid)]).astype(np.uint32)
    plen[2] = max(int(plen[2]), 2)
    if real is not None:
        gid_map, real_plen = np.asarray(real[0], dtype=np.int64), np.asarray(real[1], dtype=np.uint32)
        plen = np.concatenate([[0], real_plen[gid_map[1:ngid + 1]]]).astype(np.uint32)
    planted_rules, flows, plan = planted_flows(rng, plen, planted_calls)
    nplanted = len(flows)
    rules = planted_rules + random_seq_rules(rng, nrules, range(1, ngid + 1), max_gap=12)
    cuts = [planted_cuts(planted_calls) for _ in flows]
    lengths = []
    for _ in range(nflows):
        L = int(rng.integers(0, 60))
        lengths.append(L)
        n = int(rng.integers(0, 10)) if L else 0
        p = rng.integers(0, max(L, 1), size=n)
        g = rng.integers(1, ngid + 1, size=n)
        twin = rng.random(n) < 0.3
        flows.append(list(zip(np.concatenate([p, p[twin]]).tolist(),
                              np.concatenate([g, rng.integers(1, ngid + 1, size=int(twin.sum()))]).tolist())))
    rng = np.random.default_rng([seed, cut_seed])
    for L in lengths:
        k = int(rng.integers(1, max_calls + 1))
        cuts.append(np.concatenate([[0], np.sort(rng.integers(0, L + 1, size=k - 1)), [L]]).astype(np.int64))
    nrows = len(flows) + 4
    perm = rng.permutation(nrows)
    row_of, spare = perm[:len(flows)], int(perm[len(flows)])
    calls = []
    for c in range(max_calls):
        have = [f for f in range(len(flows)) if len(cuts[f]) - 1 > c]
        stream_flow = [have[i] for i in rng.permutation(len(have)).tolist()] + [-1, -1, -1]
        lens = [int(cuts[f][c + 1] - cuts[f][c]) for f in stream_flow[:-3]] + [7, 5, 9]
        base = int(rng.integers(1, 500))
        offs = base + np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
        rows = [int(row_of[f]) for f in stream_flow[:-3]] + [-1, nrows + int(rng.integers(0, 5)), spare]
        pos_in = [big_base + int(cuts[f][c]) for f in stream_flow[:-3]] + [3, 0, MAX_BYTES - 8]
        ev_pos, ev_gid = [int(offs[0]) - 1, int(offs[-1]), int(offs[-1]) + 3], [1, 2, 3]  # outside every stream
        for j, f in enumerate(stream_flow):
            if f < 0:
                ev_pos += [int(offs[j]), int(offs[j + 1]) - 1]
                ev_gid += [1, 2]
                continue
            for p, g in flows[f]:
                if cuts[f][c] <= p < cuts[f][c + 1]:
                    ev_pos.append(int(offs[j]) + p - int(cuts[f][c]))
                    ev_gid.append(g)
        events = pack(ev_pos, ev_gid)
        events = np.concatenate([events, events[rng.integers(0, len(events), size=len(events) // 4)]])  # duplicates
        calls.append(dict(events=rng.permutation(events), offsets=offs, rows=np.array(rows, dtype=np.int64),
                          pos_in=np.array(pos_in, dtype=np.uint64), flow=stream_flow))
    if real is not None:
        rules = [[(int(np.sign(g)) * int(gid_map[abs(g)]), gap) for g, gap in rule] for rule in rules]
        flows = [[(p, int(gid_map[g])) for p, g in ev] for ev in flows]
        for call in calls:
            ev = call["events"]
            call["events"] = (ev & ~np.uint64(GID_MAX)) | gid_map[(ev & np.uint64(GID_MAX)).astype(np.int64)].astype(np.uint64)
        plen = real_plen
    return dict(rules=rules, plen=plen, nrows=nrows, plan=plan, row_of=row_of, nplanted=nplanted, calls=calls,
                flows=flows, cuts=cuts, big_base=big_base)


def run_reference(case):
    """The reference over the case's calls: [(rule_ptr, hits, rows after the call)]."""
    state, out = {}, []
    for call in case["calls"]:
        ptr, hits = reference_flow_seq_rules(state, call["events"], call["offsets"], call["pos_in"], case["rules"],
                                             case["plen"], case["nrows"], call["rows"])
        out.append((ptr, hits, rows_array(state, case["rules"], case["plen"], case["nrows"])))
    return out


def kinds_present(case, results):
    """kind -> whether the per-call results show it: the planted rule hits in
    the planted flow exactly in the expected call at the expected flow
    position, or in no call at all."""
    seen = {}
    for kind, (f, r, expect) in case["plan"].items():
        got = []
        for c, (call, (ptr, hits, _)) in enumerate(zip(case["calls"], results)):
            if f not in call["flow"]:
                continue
            s = call["flow"].index(f)
            for h in hits[ptr[s]:ptr[s + 1]].tolist():
                if h & GID_MAX == r:
                    got.append((c, (h >> GID_BITS) - int(call["offsets"][s]) + int(call["pos_in"][s])
                                - case["big_base"]))
        seen[kind] = got == ([] if expect is None else [expect])
    return seen


def whole_flows(case):
    """The uncut flows as one list: (events, offsets) with flow f the stream f,
    positions from 0, for the cut-invariance tests."""
    lens = [int(c[-1]) for c in case["cuts"]]
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    pos = [int(offs[f]) + p for f, ev in enumerate(case["flows"]) for p, _ in ev]
    gid = [g for ev in case["flows"] for _, g in ev]
    return pack(pos, gid), offs
