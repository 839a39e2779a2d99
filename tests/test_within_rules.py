"""Within on the device (pm_hip_set_seq_rules_within,
pm_hip_seq_rules_within_run, pm_hip_seq_rules_by_stream_device; include/pm_hip.h
"ordered rules", within; csrc/pm_seqrules.hip sq_eval_within_kernel,
csrc/pm_seqwalk.h): ordered rules whose links carry an upper bound.  Hand-made
lists are written straight to the device and compared with the host twin
(pm_flat_seq_rules_by_stream_within), which test_within_rules_cpu.py pins to
the all-pairs reference and the exhaustive search; behind real scans the
expected hits come from the oracle's list through that reference.  Outputs and
scratch carry test_seq_rules.py's poisoned guard slots."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from rule_inputs import random_offsets, random_rules
from seq_rule_inputs import FREE, pack, random_seq_rules, seq_csr
from test_batch import _dev, _stream
from test_by_stream import _list_dev
from test_events import POISON64, Ev, _text_dev
from test_gpu_parity import _torch, fresh_matcher
from test_seq_rules import (LANE, LDS, Out, _aa_events, _assert_equal, _call, _planted_text, own_matcher, plen)
from within_rule_inputs import (KINDS, fuzz_case, kinds_shown, planted_case, reference_within_rules, with_bounds,
                                within_csr, within_run)

pytestmark = pytest.mark.gpu

u32p = ctypes.POINTER(ctypes.c_uint32)
BIG = 0x7FFFFFFF


def _run(events, offs, rules, fast=None, m=None, set_rules=True, lens=None, what=""):
    """The device call, once, on a hand-made list against the twin, with room
    for exactly the expected hits.  Returns (rule_ptr, expected hits)."""
    torch = _torch()
    m = own_matcher() if m is None else m
    lens = plen() if lens is None else lens
    if set_rules:
        m.set_seq_rules(rules, fast)
        assert m.seq_rule_count() == len(rules) and m.seq_rules_within_run() == within_run(rules)
    events = np.ascontiguousarray(events, dtype=np.uint64)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(events, offs, within_csr(rules), lens)
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, len(exp_hits))
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()
    ev.assert_guard(len(events))
    _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
    return ptr, exp_hits


def _fired(ptr, hits):
    """[(stream, rule, position)] of a result, sorted."""
    hp, hr = pm.unpack_events(hits)
    return sorted(zip(np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)).tolist(), hr.tolist(), hp.tolist()))


# ---- 1. the planted kinds -------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(3))
def test_planted_kinds(seed):
    events, offs, rules, lens, plan = planted_case(60 + seed, plen=plen()[:13])
    seen = kinds_shown(events, offs, rules, lens, plan)
    assert set(seen) == set(KINDS) and all(seen.values()), seen
    ref = reference_within_rules(events, offs, rules, lens)
    ptr, hits = _run(events, offs, rules)
    assert np.array_equal(ptr, ref[0]) and np.array_equal(hits, ref[1])


# ---- 2. run lengths: the levels in LDS --------------------------------------------------------
@pytest.mark.parametrize("run", [1, 2, 3, 62, 63])
def test_run_lengths(run):
    """A chain of run + 1 terms, every link bounded and met by exactly zero
    bytes on the upper side (five to spare on the lower), behind a decoy of
    every gid that lies before the head; then the same with one occurrence a
    byte late."""
    lens = plen()
    rule = [(1, None)] + [(g, 1, 1 + int(lens[g]) + 5) for g in range(2, run + 2)]
    p = [1000]
    for g in range(2, run + 2):
        p.append(p[-1] + 1 + int(lens[g]) + 5)
    decoys = pack(100 + 3 * (run - np.arange(run + 1)), np.arange(1, run + 2))  # in the wrong order
    events = pack(p, np.arange(1, run + 2))
    rng = np.random.default_rng(run)
    offs = [50, p[-1] + 3]
    fast = [int(rng.integers(1, run + 2))]
    ptr, hits = _run(rng.permutation(np.concatenate([decoys, events])), offs, [rule], fast=fast)
    assert own_matcher().seq_rules_within_run() == run
    assert hits.tolist() == [p[-1] << 24]
    late = events.copy()
    late[run // 2 + 1] += np.uint64(1 << 24)  # (the next link, if any, now has six bytes to spare)
    ptr, hits = _run(rng.permutation(np.concatenate([decoys, late])), offs, [rule], fast=fast)
    assert ptr[-1] == 0


# ---- 3. divergent lanes ----------------------------------------------------------------------
def test_65_rules_on_one_slot_with_mixed_run_lengths():
    """gid 7 is the PM_RULE_FAST anchor of 65 rules whose run lengths are 0, 1,
    2 and 5 lane by lane: neighbouring lanes are on different levels of the
    LDS array, and the 65th rule is walked in a second turn of 64."""
    lens = plen()
    runs = (0, 1, 2, 5)
    rules = []
    for k in range(65):
        run = runs[k % 4]
        tail = [(100 + (k + i) % 12, 0, int(lens[100 + (k + i) % 12]) + 12) for i in range(run)]
        rules.append([(7, None)] + (tail if run else [(100 + k % 12, 3)]))
    rng = np.random.default_rng(65)
    pos = np.concatenate([rng.integers(5, 2000, size=6), rng.integers(5, 2000, size=3000)])
    events = pack(pos, np.concatenate([[7] * 6, rng.integers(100, 112, size=3000)]))
    ptr, hits = _run(events, [5, 1000, 1000, 2000], rules, fast=[7] * 65)
    assert own_matcher().seq_rules_within_run() == 5
    fired = {r for _, r, _ in _fired(ptr, hits)}
    assert {r % 4 for r in fired} == {0, 1, 2, 3} and 64 in fired and len(fired) < 65 * 2


def test_the_anchor_at_the_first_a_middle_and_the_last_term_of_a_bounded_run():
    rng = np.random.default_rng(66)
    offs = random_offsets(rng, 60, max_len=300)
    events = pack(rng.integers(offs[0], offs[-1], size=4000), rng.integers(1, 7, size=4000))
    rules = with_bounds(rng, random_seq_rules(rng, 80, np.arange(1, 7), max_pos=4, follow=0.9, max_gap=10), plen(),
                        share=0.9, slack=30)
    want = None
    for turn in range(3):
        fast = []
        for r in rules:
            positive = [t[0] for t in r if t[0] > 0]
            fast.append(positive[(0, len(positive) // 2, len(positive) - 1)[turn]])
        ptr, hits = _run(events, offs, rules, fast=fast)
        want = (ptr, hits) if want is None else want
        assert ptr[-1] > 0 and np.array_equal(ptr, want[0]) and np.array_equal(hits, want[1])


# ---- 4. ranges of every sort tier, a failed candidate per position -----------------------------------
@pytest.mark.parametrize("n", [LANE, LANE + 1, LDS + 1])
def test_every_candidate_but_the_last_fails_by_one_byte(n):
    """n A's four bytes apart and n B's, each B but the last beginning one byte
    before its A has ended and too far behind the A before: the walk places n
    candidates in turn, each one position further (the gallop's first step),
    and asks A's level n times.  Ranges of 16, 17 and 4,097 positions: one
    from each tier of the sort."""
    L = int(plen()[2])
    a = 1000 + 4 * np.arange(n)
    b = a + L - 1
    b[-1] = a[-1] + L
    rng = np.random.default_rng(n)
    events = rng.permutation(np.concatenate([pack(a, np.full(n, 1)), pack(b, np.full(n, 2))]))
    rules = [[(1, None), (2, 0, L + 1)], [(1, None), (2, 0, L)], [(1, None), (2, 1, L + 1)]]
    ptr, hits = _run(events, [900, int(b[-1]) + 2], rules)
    assert _fired(ptr, hits) == [(0, 0, int(b[-1])), (0, 1, int(b[-1]))]


# ---- 5. the largest bound ----------------------------------------------------------------------
def test_within_0x7fffffff_above_2_33_and_a_head_below_the_bound():
    L2, L3 = int(plen()[2]), int(plen()[3])
    a = (1 << 33) + 5
    # the low stream: candidate - w lies below 0 and must not wrap; the high one: met by zero bytes, missed by one
    events = pack([100, 100 + L2 + 2, 100 + L2 + 2 + L3, a, a + BIG, a + BIG + 1], [1, 2, 3, 1, 2, 3])
    rules = [[(1, None), (2, 0, BIG)], [(1, None), (3, 0, BIG)], [(1, None), (2, 0, BIG), (3, 0, BIG)]]
    ptr, hits = _run(events, [10, 5000, 1 << 33, (1 << 33) + (1 << 32)], rules)
    low = 100 + L2 + 2
    high = [(2, 0, a + BIG)] + ([(2, 2, a + BIG + 1)] if L3 == 1 else [])  # (a pattern of one byte may follow at once)
    assert _fired(ptr, hits) == [(0, 0, low), (0, 1, low + L3), (0, 2, low + L3)] + high


# ---- 6. hits_cap ---------------------------------------------------------------------------------
@pytest.mark.parametrize("short", ["one", "all"])
def test_hits_cap_short_keeps_rule_ptr_exact(short):
    torch = _torch()
    m = own_matcher()
    rng = np.random.default_rng(67)
    events = pack(rng.integers(0, 900, size=3000), rng.integers(1, 20, size=3000))
    offs = np.arange(0, 1001, 100, dtype=np.int64)
    nseg = len(offs) - 1
    rules = with_bounds(rng, random_seq_rules(rng, 400, np.arange(1, 22), max_pos=3, follow=0.7), plen())
    m.set_seq_rules(rules)
    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(events, offs, rules, plen())
    total = int(exp_ptr[-1])
    assert total > 100 and m.seq_rules_within_run() > 0
    hits_cap = total - 1 if short == "one" else 0
    ev = _list_dev(torch, events, len(events), len(events))
    o = Out(torch, m, len(events), nseg, hits_cap)
    _call(m, torch, ev, _dev(torch, offs), nseg, o)
    torch.cuda.synchronize()
    ptr, hits = o.result()  # (the guard behind hits_cap is checked there)
    assert np.array_equal(ptr, exp_ptr)
    seg = np.repeat(np.arange(nseg), np.diff(exp_ptr))
    want = set(zip(seg.tolist(), exp_hits.tolist()))
    got = list(zip(seg[:hits_cap].tolist(), hits.tolist()))
    assert len(set(got)) == len(got) == hits_cap and set(got) <= want


# ---- 7. rule sets ----------------------------------------------------------------------------------
def test_sets_replaced_in_turn_bounded_unbounded_bounded():
    m = own_matcher()
    rng = np.random.default_rng(68)
    events = pack(rng.integers(0, 300, size=2000), rng.integers(1, 12, size=2000))
    offs = np.arange(0, 301, 30)
    plain = random_rules(rng, 100, np.arange(1, 13))
    flow = random_rules(rng, 50, np.arange(1, 13), negated=0.0)
    m.set_rules(plain)
    m.set_flow_rules(flow)
    sets = np.zeros((len(offs) - 1, m.flow_rule_words), dtype=np.uint64)
    r0, f0 = m.rules_by_stream(events, offs), m.flow_rules(events, offs, sets, keep=True)
    loose = random_seq_rules(rng, 200, np.arange(1, 13), max_pos=4, follow=0.8)
    bounded = with_bounds(rng, loose, plen(), share=1.0, slack=10)
    a, ha = _run(events, offs, bounded)
    base = m.table_bytes
    assert m.seq_rules_within_run() == within_run(bounded) > 1
    b, hb = _run(events, offs, loose)
    nterms = sum(len(r) for r in loose)
    assert m.seq_rules_within_run() == 0 and m.table_bytes == base - 4 * nterms  # the bounds: a word per term
    assert a[-1] > 0 and b[-1] > a[-1]  # the bounds kill hits: the two sets ran different kernels' walks
    c, hc = _run(events, offs, bounded)
    assert np.array_equal(a, c) and np.array_equal(ha, hc) and m.table_bytes == base
    assert m.rule_count() == 100 and m.flow_rule_count() == 50
    r1, f1 = m.rules_by_stream(events, offs), m.flow_rules(events, offs, sets, keep=True)
    assert r0[0][-1] > 0 and f0[0][-1] > 0
    for x, y in ((r0, r1), (f0, f1)):
        assert np.array_equal(x[0], y[0]) and np.array_equal(x[1], y[1])


def test_every_within_free_through_the_new_setter_gives_set_seq_rules_hits():
    m = own_matcher()
    rng = np.random.default_rng(69)
    offs = random_offsets(rng, 300)
    events = pack(rng.integers(offs[0], offs[-1], size=10000), rng.integers(1, 12, size=10000))
    rules = random_seq_rules(rng, 300, np.arange(1, 14), max_gap=20)
    want = _run(events, offs, rules)  # pm_hip_set_seq_rules
    tptr, terms, gaps = seq_csr(rules)
    free = np.full(len(terms), FREE, np.uint32)
    for withins in (free.ctypes.data_as(u32p), None):
        assert m.lib.pm_hip_set_seq_rules_within(m.obj, tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                                 gaps.ctypes.data_as(u32p), withins, len(rules)) == 0
        assert m.seq_rules_within_run() == 0 and m.seq_rule_count() == len(rules)
        got = _run(events, offs, rules, set_rules=False)
        assert want[0][-1] > 0 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_every_bad_rule_set_is_minus_2_and_the_rules_stay():
    from test_within_rules_cpu import bad_within_rule_sets
    m = own_matcher()
    rules = [[(1, None), (2, 0, 8)], [(2, None), (-3, None)]]
    events = pack([1, 8, 50, 60, 70], [1, 2, 2, 3, 2])
    offs = [0, 40, 60, 90]
    want = _run(events, offs, rules)
    before = m.table_bytes
    for name, raw in bad_within_rule_sets(int(plen()[2])):
        rc = m.lib.pm_hip_set_seq_rules_within(m.obj, *[None if x is None else x.ctypes.data_as(u32p) for x in raw],
                                               len(raw[0]) - 1)
        assert rc == -2, name
        msg = m.lib.pm_hip_last_error()
        for word in (b"2^24", b"positive", b"PM_SEQ_FREE", b"0x7FFFFFFF", b"following", b"within", b"length"):
            assert word in msg, (name, word)
        assert m.seq_rule_count() == 2 and m.table_bytes == before and m.seq_rules_within_run() == 1, name
    got = _run(events, offs, rules, set_rules=False)
    assert want[0][-1] == 3 and np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def test_before_any_set_the_device_call_is_minus_10():
    torch = _torch()
    m = fresh_matcher("et", "rt")
    try:
        assert m.seq_rules_within_run() == 0 and m.seq_rule_count() == 0
        events = pack([1, 2, 3, 3], [1, 1, 2, 2])
        offs = np.array([0, 2, 4], dtype=np.int64)
        ev = _list_dev(torch, events, 4, 4)
        o = Out(torch, m, 4, 2, 4)
        args = [ev.buf.data_ptr(), 4, ev.nev.data_ptr(), _dev(torch, offs).data_ptr(), 2, o.hits.data_ptr(), 4,
                o.ptr.data_ptr(), o.scratch.data_ptr(), o.bytes, _stream(torch)]
        assert m.lib.pm_hip_seq_rules_by_stream_device(m.obj, *args) == -10
        torch.cuda.synchronize()
        assert o.untouched()
        # a rejected first set leaves it so
        raw = within_csr([[(1, None), (2, 0, 0)]])  # below d + L
        assert m.lib.pm_hip_set_seq_rules_within(m.obj, *[x.ctypes.data_as(u32p) for x in raw], 1) == -2
        assert m.lib.pm_hip_seq_rules_by_stream_device(m.obj, *args) == -10 and m.seq_rules_within_run() == 0
    finally:
        m.free()


# ---- 8. fuzz ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_fuzz(seed):
    """test_within_rules_cpu.py's fuzz inputs (whose condition is asserted
    there) with the object's own pattern lengths and a random PM_RULE_FAST."""
    events, offs, rules, lens = fuzz_case(seed, scale=0.2, plen=plen()[:8])
    rng = np.random.default_rng(seed)
    fast = [None if rng.random() < 0.5 else int(rng.choice([t[0] for t in r if t[0] > 0])) for r in rules]
    ptr, hits = _run(events, offs, rules, fast=fast)
    assert ptr[-1] > 0


# ---- 9. behind real scans ----------------------------------------------------------------------------
def test_behind_the_batched_and_the_flow_scan():
    """test_seq_rules' planted text of seed4: P x* Q with 0 to 40 bytes of
    filler.  P, then Q within L_Q + k for k at, one below and one above
    planted gaps; the hits are the all-pairs reference's on the oracle's list."""
    torch = _torch()
    m, text, offs, events, seq_rules, lens = _planted_text("seed4")
    try:
        P, Q = seq_rules[0][0][0], seq_rules[0][1][0]
        LQ = int(lens[Q])
        ks = (0, 1, 9, 10, 11, 24, 25, 26, 39, 40, 41)
        rules = [[(P, None), (Q, 0, LQ + k)] for k in ks] + [[(Q, None), (P, None, int(lens[P]) + 15)]]
        exp_ptr, exp_hits = reference_within_rules(events, offs, rules, lens)
        counts = np.bincount((exp_hits & np.uint64(0xFFFFFF)).astype(np.int64), minlength=len(rules))
        assert counts[0] < counts[3] < counts[6] < counts[-2] and counts[-1] > 0, counts
        m.set_seq_rules(rules)
        assert m.seq_rules_within_run() == 1
        min_len = m.seq_rules_min_len()
        nseg, n = len(offs) - 1, len(text)
        d_text, d_offs = _text_dev(torch, text), _dev(torch, offs)

        def batch(ev):
            m.scan_batch_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, min_len, ev.buf.data_ptr(),
                                        ev.cap, ev.nev.data_ptr(), _stream(torch))

        def flow(ev):
            m.scan_flows_matches_device(d_text.data_ptr(), d_offs.data_ptr(), nseg, n, None, None, min_len,
                                        ev.buf.data_ptr(), ev.cap, ev.nev.data_ptr(), _stream(torch))
        for what, scan in (("batch", batch), ("flow", flow)):
            ev = Ev(torch, 16 * n)
            o = Out(torch, m, ev.cap, nseg, len(exp_hits))
            scan(ev)
            _call(m, torch, ev, d_offs, nseg, o)  # no synchronize between
            torch.cuda.synchronize()
            assert 0 < ev.total() <= ev.cap, what
            ptr, hits = o.result()
            _assert_equal(ptr, hits, exp_ptr, exp_hits, what)
        # the host form and read_many_seq_rules take the bounded set too
        ptr, hits = m.seq_rules_by_stream(events, offs)
        assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits)
        js = [int(j) for j in np.argsort(-np.diff(exp_ptr))[:5]]
        for j, (gpos, grule) in zip(js, m.read_many_seq_rules([bytes(text[offs[j]:offs[j + 1]]) for j in js])):
            hp, hr = pm.unpack_events(exp_hits[exp_ptr[j]:exp_ptr[j + 1]])
            assert len(hr) > 0 and gpos.tolist() == (hp - offs[j]).tolist() and grule.tolist() == hr.tolist(), j
    finally:
        m.free()


# ---- 10. captured -----------------------------------------------------------------------------------
def test_captured_once_and_replayed_over_three_lists_with_a_bounded_set():
    """test_seq_rules._replayed with bounds: 40 ranges of 17 positions of gid
    5, then 3 of gid 6 and fewer events, then 40 of gid 7; the rules gid ... gid
    whose link only the last position meets, now exactly (w == d + L), and
    random bounded rules.  The scratch holds poison before the first replay;
    nothing is reset between the replays but what the call resets itself."""
    torch = _torch()
    m = fresh_matcher("et", "rt")  # no read_block call: no resident server to stop inside the capture
    try:
        lens = plen()
        rng = np.random.default_rng(70)
        nseg, n, step = 40, LANE + 1, 64
        offs = np.arange(nseg + 1, dtype=np.int64) * 2000 + 11
        noise = pack(rng.integers(offs[0], offs[-1], size=3000), rng.choice([1, 2, 3, 4, 8], size=3000))
        lists, rules = [], []
        for g, streams, keep in ((5, range(nseg), 3000), (6, (3, 17, 39), 1000), (7, range(nseg), 3000)):
            events, by_gid = _aa_events([(j, g) for j in streams], offs, rng, n=n, step=step)
            lists.append(np.concatenate([events, noise[:keep]]))
            (g0, _), (g1, d) = by_gid[g]
            rules.append([(g0, None), (g1, d, d + int(lens[g]))])
        rules += with_bounds(rng, random_seq_rules(rng, 50, np.arange(1, 9), max_pos=5, follow=0.8, max_gap=30), lens,
                             share=0.8, slack=60)
        m.set_seq_rules(rules)
        assert m.seq_rules_within_run() >= 2
        cap = len(lists[0]) + 50
        ev = Ev(torch, cap)
        d_offs = _dev(torch, offs)
        o = Out(torch, m, cap, nseg, 20000)
        st = torch.cuda.Stream()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr, stream=st):
            _call(m, torch, ev, d_offs, nseg, o, stream=st.cuda_stream)
        torch.cuda.synchronize()
        seen = []
        for replay, lst in enumerate(lists):
            ev.buf[:len(lst)] = torch.from_numpy(lst.view(np.int64)).cuda()
            ev.nev.fill_(len(lst))
            o.hits[:o.hits_cap].fill_(POISON64 - (1 << 64))
            torch.cuda.synchronize()
            gr.replay()
            torch.cuda.synchronize()
            ptr, hits = o.result()
            exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, rules, lens)
            assert 0 < exp_ptr[-1] <= o.hits_cap, replay
            _assert_equal(ptr, hits[:ptr[-1]], exp_ptr, exp_hits, f"list {replay}")
            assert np.all(hits[ptr[-1]:] == POISON64)
            seen.append(int(np.count_nonzero((exp_hits & np.uint64(0xFFFFFF)) == replay)))
        assert seen == [40, 3, 40]
    finally:
        m.free()

