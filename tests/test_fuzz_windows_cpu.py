"""The random dictionaries of tests/fuzz_inputs.py through the host twins of
the window scans: pm_flat_window_tables and pm_flat_expand_windows over every
case, text A from byte 0 and text B continuing it, with window tables scaled to
the fuzz streams (window_inputs.fuzz_window_of); the same twin and the nocase
host scan with flow positions around 2^32, at 2^40 and at 2^62
(window_inputs.far_pos_in, far_window_of); and the guards that keep the GPU file
(test_fuzz_windows.py) from being vacuous.  Expected lists come from the
oracle's codes, its pattern bytes and the tests' own tables; the library's
parent, reach and win tables are never their source.  CPU only."""
import numpy as np
import pytest

import patternmatching_amd as pm
from fuzz_inputs import ALPHABETS, CASES, GPU_CASES, SEEDS, case
from group_inputs import masks_by_index, stream_masks
from match_inputs import suffix_chains
from nocase_inputs import brute, call_events, flag_of, fuzz_dictionary, fuzz_text, group_of, stream_groups, stream_offsets
from test_fuzz_lists_cpu import _assert_events
from test_matches_cpu import _gids_of
from test_nocase_cpu import Twin
from test_tables_cpu import image
from test_windows_cpu import _expand, _tables
from window_inputs import (INF, chain_stats, code_windows, expected_windows, far_pos_in, far_stats, far_window_of,
                           fuzz_window_of, window_sel, window_stats, windows_by_index)

MIN_LENS = (1, 3)
CHAIN_DEPTH = 8


def _lens(c):
    return np.diff(c.offs).astype(np.uint64)


def _check(img, tab, gids, key, exp, offs, pos_in, sg, by_index, win, min_len, all_matches, fn, what):
    want = expected_windows(key, exp, offs, pos_in, sg, min_len, all_matches, fn=fn)
    rc, ev, total = _expand(img, gids, offs, pos_in, sg, by_index if sg is not None else None, win, min_len,
                            all_matches, len(want[0]))
    assert rc == 0
    _assert_events(ev, total, tab, want, what)
    return total


def _assert_window_tables(name, img, tab, d, fn):
    """win[g]: the pattern's need and max_end, and their folds over the
    suffixes the oracle's byte-string lookup finds."""
    lo, hi = windows_by_index(d, fn)
    rc, win = _tables(img, lo, hi)
    assert rc == 0
    win = win.reshape(-1, 4)
    iog = img.array("index_of_gid")
    lens = np.array([len(p) for p in d.patterns()], dtype=np.int64)
    assert win[0].tolist() == [INF, 0, INF, 0]
    assert np.array_equal(win[1:, 0], lo[iog[1:]] + lens[iog[1:]])
    assert np.array_equal(win[1:, 1], hi[iog[1:]])
    chains = suffix_chains(name)
    codes, clo, chi, _ = code_windows(name, fn)
    for g in range(1, len(tab)):
        ch = chains.get(int(tab[g]))
        if ch is not None:  # a code that is not a lookup's answer is a shadowed duplicate
            k = np.searchsorted(codes, ch[0])
            assert int(win[g, 2]) == int(np.min(clo[k] + ch[1])), g
            assert int(win[g, 3]) == int(np.max(chi[k])), g


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("name", CASES)
def test_host_windows_equal_the_oracles_lists(name, kind):
    """A with every stream at byte 0, then B with every stream at its length of
    A; both forms, min_len 1 and 3, with and without group masks."""
    c = case(name)
    d, img, tab = image(name, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    by_index, win = masks_by_index(d), windows_by_index(d, fuzz_window_of)
    _assert_window_tables(name, img, tab, d, fuzz_window_of)
    seen = 0
    for exp, pos_in, which in ((c.ea, None, "A"), (c.eb, _lens(c), "B")):
        gids = _gids_of(img, tab, exp)
        for sg in (None, stream_masks(c.nseg)):
            for min_len in MIN_LENS:
                for all_matches in (True, False):
                    seen += _check(img, tab, gids, name, exp, c.offs, pos_in, sg, by_index, win, min_len, all_matches,
                                   fuzz_window_of, f"{which}, masks {sg is not None}, min_len {min_len}, "
                                   f"all {all_matches}")
    assert seen > 0


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("name", CASES)
def test_host_windows_far_positions(name, kind):
    """A from far_pos_in, then B from far_pos_in plus the lengths: the host
    twin's 64-bit E against int64 arithmetic in numpy."""
    c = case(name)
    d, img, tab = image(name, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    by_index, win = masks_by_index(d), windows_by_index(d, far_window_of)
    _assert_window_tables(name, img, tab, d, far_window_of)
    far = far_pos_in(c.offs)
    after = far + _lens(c)
    assert after.dtype == np.uint64 and int(after.max()) <= (1 << 62) + 4097
    seen = 0
    for exp, pos_in, which in ((c.ea, far, "A"), (c.eb, after, "B")):
        gids = _gids_of(img, tab, exp)
        for sg in (None, stream_masks(c.nseg)):
            for all_matches in (True, False):
                seen += _check(img, tab, gids, name, exp, c.offs, pos_in, sg, by_index, win, 1 if all_matches else 3,
                               all_matches, far_window_of, f"far {which}, masks {sg is not None}, all {all_matches}")
    assert seen > 0


def test_far_pos_in():
    c = case("unary")
    lens = np.diff(c.offs).tolist()
    far = far_pos_in(c.offs).tolist()
    assert len(far) == c.nseg and max(far) == 1 << 62
    for j in range(22):
        n, want = lens[j], [None] * 11
        want[:9] = [(1 << 32) - x for x in (n + 1, n, n // 2, 17, 16, 1, 0, -1, -4096)]
        want[9:] = [1 << 40, 1 << 62]
        assert far[j] == want[j % 11], j
    # every entry of the cycle meets streams with bytes, the first three longer than a 16-byte block
    for r in range(11):
        assert sum(1 for j in range(r, c.nseg, 11) if lens[j] > 32) >= 10, r


# ---- the nocase host twin, far positions -------------------------------------------------
def nocase_far_inputs():
    """fuzz_dictionary(1) with its crc32 flags, group_of's groups and
    far_window_of's windows; two texts over one set of offsets; far_pos_in."""
    pats = fuzz_dictionary(1)
    flags = [flag_of(p) for p in pats]
    groups = np.array([group_of(p) for p in pats], dtype=np.uint32)
    w = [far_window_of(p) for p in pats]
    windows = (np.array([a for a, _ in w], np.uint32), np.array([b for _, b in w], np.uint32))
    A, B = fuzz_text(pats, 1, 12288), fuzz_text(pats, 51, 12288)
    offs = stream_offsets(len(A), 1)
    return pats, flags, groups, windows, A, B, offs, far_pos_in(offs)


def test_nocase_twin_far_positions():
    pats, flags, groups, windows, A, B, offs, far = nocase_far_inputs()
    tw = Twin(pats, flags, pm.KIND_AC)
    nseg = len(offs) - 1
    lens = np.diff(offs)
    sg = stream_groups(nseg)
    whole = [bytes(A[offs[j]:offs[j + 1]]) + bytes(B[offs[j]:offs[j + 1]]) for j in range(nseg)]
    base = [int(x) for x in far]
    sel = np.array([window_sel(p) for p in pats])
    gid_sel = np.zeros(len(pats) + 1, np.int64)
    gid_sel[tw.gid_of_index] = sel
    for all_matches in (True, False):
        rows, _ = brute(pats, flags, whole, tw.gid_of_index, 1, groups, sg, windows, all_matches, base=base)
        open_rows, _ = brute(pats, flags, whole, tw.gid_of_index, 1, groups, sg, None, all_matches)
        kw = dict(sgroups=sg, groups=groups, windows=windows, min_len=1, all_matches=all_matches)
        ev, st, pos, hist = tw.scan(A, offs, pos=far, **kw)
        want_a = call_events(rows, offs, np.zeros(nseg, np.int64))[0]
        assert np.array_equal(ev, want_a), ("A", all_matches)
        assert pos.dtype == np.uint64 and pos.tolist() == [b + int(n) for b, n in zip(base, lens)]
        ev, _, pos2, _ = tw.scan(B, offs, state=st, pos=pos, case=hist, **kw)
        want_b = call_events(rows, offs, lens)[0]
        assert np.array_equal(ev, want_b), ("B", all_matches)
        assert pos2.tolist() == [b + 2 * int(n) for b, n in zip(base, lens)]
        assert len(want_a) > 0 and len(want_b) > 0
        if all_matches:  # the windows keep and drop events of every selector that can do either here
            kept = np.bincount(gid_sel[rows[:, 2]], minlength=8)
            cand = np.bincount(gid_sel[open_rows[:, 2]], minlength=8)
            assert np.array_equal(kept[:3], cand[:3]) and np.all(kept[:3] > 0)
            for s in (3, 5):  # an end of 0xFFFFFFFE: kept below the edge only
                assert 0 < kept[s] < cand[s], (s, kept[s], cand[s])
            assert kept[4] == cand[4] > 0  # a start of 0x7FFFFFFF: every flow is past it
            assert cand[6] > 0 and kept[6] == 0 and cand[7] > 0 and kept[7] == 0


# ---- non-vacuity guards ------------------------------------------------------------------
def test_fuzz_windows_keep_and_drop():
    """Summed over the cases, A and B, min_len 1 and 3: every bounded kind of
    window of fuzz_window_of has candidates, keeps some and drops some; the
    unsatisfiable one has candidates and keeps none."""
    for min_len in MIN_LENS:
        tot = {s: [0, 0] for s in range(3, 8)}
        for name in CASES:
            c = case(name)
            for exp, pos_in in ((c.ea, None), (c.eb, _lens(c))):
                per_sel = window_stats(name, exp, c.offs, pos_in, min_len, fuzz_window_of)[0]
                for s, (cand, kept) in per_sel.items():
                    tot[s][0] += cand
                    tot[s][1] += kept
        for s in (3, 4, 5, 6):
            assert 0 < tot[s][1] < tot[s][0], (min_len, s, tot[s])
        assert tot[7][0] > 0 and tot[7][1] == 0, (min_len, tot[7])


def test_deep_chain_members_pass_and_fail_apart_from_their_heads():
    """The all-matches list of A or B at min_len 1: positions where a member
    at chain depth >= 8 (the head is depth 1) is kept while a shallower one is
    dropped, and positions where one is dropped while a shallower one is kept.
    Both occur in unary and in two more cases.  The seeds over 2 symbols have
    no chain of 8 members (the deepest has 7, test_fuzz_lists_cpu.GUARDS); one of
    them meets both conditions at depth >= 5, the depth all three reach."""
    def both(name, depth):
        c = case(name)
        rows = [chain_stats(name, exp, c.offs, pos_in, depth, fuzz_window_of)
                for exp, pos_in in ((c.ea, None), (c.eb, _lens(c)))]
        return sum(r[0] for r in rows) > 0 and sum(r[1] for r in rows) > 0

    deep = [name for name in CASES if both(name, CHAIN_DEPTH)]
    assert "unary" in deep and len(deep) >= 3, deep
    assert len([name for name in deep if name in GPU_CASES]) >= 2, deep
    two = [f"seed{s}" for s in SEEDS if ALPHABETS[s % len(ALPHABETS)] == 2]
    assert max(len(ch[0]) for name in two for ch in suffix_chains(case(name).key).values()) < CHAIN_DEPTH
    assert [name for name in two if name in GPU_CASES and both(name, 5)], two


def test_longest_visible_differs_from_the_dictionarys_answer():
    """In at least half of the cases the longest form's pattern is not the
    dictionary's answer at more than 1% of the positions that have a
    candidate (text A, min_len 1)."""
    often = []
    for name in CASES:
        c = case(name)
        differ = window_stats(name, c.ea, c.offs, None, 1, fuzz_window_of)[3]
        positions = chain_stats(name, c.ea, c.offs, None, 1, fuzz_window_of)[2]
        assert positions == int(np.count_nonzero(c.ea))
        if differ > 0.01 * positions:
            often.append(name)
    assert 2 * len(often) >= len(CASES), often
    assert 2 * len([name for name in often if name in GPU_CASES]) >= len(GPU_CASES), often


def test_far_positions_cross_the_32_bit_edge():
    """Of the candidates of every bounded kind of window of far_window_of, A
    from far_pos_in and B continuing it: some end where the stream has had
    fewer than 0xFFFFFFFF bytes, some exactly that many, some more.  Per case
    for below and above, and for the exact count over the case's kinds
    together (a sparse case has a dozen such candidates); per kind over the
    cases the GPU file runs."""
    tot = {s: [0, 0, 0, 0] for s in range(3, 8)}
    for name in CASES:
        c = case(name)
        far = far_pos_in(c.offs)
        rows = [far_stats(name, exp, c.offs, pos_in, 1) for exp, pos_in in ((c.ea, far), (c.eb, far + _lens(c)))]
        per = {s: [a + b for a, b in zip(rows[0][s], rows[1][s])] for s in range(3, 8)}
        for s, (below, at, above, kept) in per.items():
            assert below > 0 and above > 0, (name, s, per[s])
            if name in GPU_CASES:
                tot[s] = [x + y for x, y in zip(tot[s], per[s])]
        assert sum(v[1] for v in per.values()) > 0, (name, per)
        # what each kind keeps: all below the edge, everything, nothing
        assert per[3][3] == per[3][0] and per[5][3] == per[5][0], (name, per)
        assert per[4][3] == sum(per[4][:3]) and per[6][3] == 0 and per[7][3] == 0, (name, per)
    for s, (below, at, above, kept) in tot.items():
        assert below > 0 and at > 0 and above > 0, (s, tot[s])
