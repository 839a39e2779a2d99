"""The host-only pieces of the pattern windows (pm_hip.h, "pattern windows"):
pm_flat_window_tables and pm_flat_expand_windows against the oracle's suffix
lookup and the tests' own tables, their argument rules, a brute-force case
without the oracle, and the guards that keep the GPU tests' inputs from being
vacuous.  CPU only."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from flow_inputs import F_FLOWS, input_f
from group_inputs import masks_by_index, stream_masks
from match_inputs import sort_matches, suffix_chains
from table_emulator import FlatImage
from test_groups_cpu import _expand as _expand_groups
from test_matches_cpu import POISON64, U32P, U64P, _gids_of
from test_tables_cpu import image
from window_inputs import (INF, code_windows, expected_windows, f_pos_in, flows_as_streams, packet_vs_flow, unbounded,
                           window_stats, windows_by_index)

I64P = ctypes.POINTER(ctypes.c_int64)


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _expand(img, gids, offs, pos_in, sgroups, by_index, win, min_len, all_matches, cap, n=None):
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(12345)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    pos_in = None if pos_in is None else np.ascontiguousarray(pos_in, dtype=np.uint64)
    lo, hi = win
    rc = img.lib.pm_flat_expand_windows(img.h, _p(gids, U32P), len(gids) if n is None else n, _p(offs, I64P),
                                        len(offs) - 1, _p(pos_in, U64P), _p(sgroups, U32P), _p(by_index, U32P),
                                        _p(lo, U32P), _p(hi, U32P), min_len, int(all_matches), _p(ev, U64P), cap,
                                        ctypes.byref(total))
    return rc, ev, total.value


def _tables(img, lo, hi, n=None):
    G = len(img.array("index_of_gid"))
    win = np.full(4 * G, 0x5A5A5A5A, np.uint32)
    rc = img.lib.pm_flat_window_tables(img.h, _p(lo, U32P), _p(hi, U32P), (len(lo) if n is None else n), _p(win, U32P))
    return rc, win


def _check(img, tab, gids, key, exp, offs, pos_in, sg, by_index, win, min_len, all_matches, what):
    pos, codes = expected_windows(key, exp, offs, pos_in, sg, min_len, all_matches)
    rc, ev, total = _expand(img, gids, offs, pos_in, sg, by_index if sg is not None else None, win, min_len,
                            all_matches, len(pos))
    assert rc == 0 and total == len(pos), (what, total, len(pos))
    assert np.all(ev[len(pos):] == POISON64)
    ev = ev[:len(pos)]
    assert np.all(ev[1:] > ev[:-1]), "ascending as plain u64, no event twice"
    gp, gg = pm.unpack_events(ev)
    gp, gc = sort_matches(gp, tab[gg])
    assert np.array_equal(gp, pos) and np.array_equal(gc, codes), what
    return len(pos)


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_expand_windows_input_t(key, kind):
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    _, offs, exp = input_t(key)
    gids = _gids_of(img, tab, exp)
    by_index, win = masks_by_index(d), windows_by_index(d)
    for sg in (None, stream_masks(len(offs) - 1)):
        for min_len in (1, 3, 5):
            for all_matches in (True, False):
                assert _check(img, tab, gids, key, exp, offs, None, sg, by_index, win, min_len, all_matches,
                              (sg is None, min_len, all_matches)) > 0


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_expand_windows_input_f_calls(key, kind):
    """Every call of input F, each flow's position taken from its packet
    offsets; a form per call in turn so that every form meets every min_len."""
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    F = input_f(key)
    by_index, win = masks_by_index(d), windows_by_index(d)
    masks = stream_masks(F_FLOWS)
    seen = 0
    for r, (data, offs, exp) in enumerate(F.calls):
        gids = _gids_of(img, tab, exp)
        pos_in = f_pos_in(F, r)
        for min_len in (1, 3, 5):
            for sg in (None, masks):
                all_matches = bool((r + min_len + (sg is None)) & 1)
                seen += _check(img, tab, gids, key, exp, offs, pos_in, sg, by_index, win, min_len, all_matches,
                               (r, min_len, sg is None, all_matches))
                if r < 4:
                    seen += _check(img, tab, gids, key, exp, offs, pos_in, sg, by_index, win, min_len,
                                   not all_matches, (r, min_len, sg is None, not all_matches))
    assert seen > 0


@pytest.mark.parametrize("key", ["et", "merged"])
def test_unbounded_windows_give_the_groups_lists(key):
    d, img, tab = image(key, pm.KIND_RT)
    _, offs, exp = input_t(key)
    gids = _gids_of(img, tab, exp)
    by_index, win = masks_by_index(d), windows_by_index(d, unbounded)
    ones = np.full(len(by_index), 0xFFFFFFFF, np.uint32)
    sg = stream_masks(len(offs) - 1)
    for min_len in (1, 3, 5):
        for all_matches in (True, False):
            cap = 2 * len(exp)
            rc, want, total = _expand_groups(img, gids, offs, sg, by_index, min_len, all_matches, cap)
            rc2, got, total2 = _expand(img, gids, offs, None, sg, by_index, win, min_len, all_matches, cap)
            assert rc == 0 and rc2 == 0 and total == total2 > 0
            assert np.array_equal(got, want)
            # no group tables: the groups list with every pattern in every group
            rc, want, total = _expand_groups(img, gids, offs, None, ones, min_len, all_matches, cap)
            rc2, got, total2 = _expand(img, gids, offs, None, None, None, win, min_len, all_matches, cap)
            assert rc == 0 and rc2 == 0 and total == total2 > 0
            assert np.array_equal(got, want)


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_window_tables(key, kind):
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    lo, hi = windows_by_index(d)
    rc, win = _tables(img, lo, hi)
    assert rc == 0
    win = win.reshape(-1, 4)
    iog = img.array("index_of_gid")
    lens = np.array([len(p) for p in d.patterns()], dtype=np.int64)
    assert win[0].tolist() == [INF, 0, INF, 0]
    assert np.array_equal(win[1:, 0], lo[iog[1:]] + lens[iog[1:]])
    assert np.array_equal(win[1:, 1], hi[iog[1:]])
    # the folds: over the suffixes the oracle's byte-string lookup finds
    chains = suffix_chains(key)
    codes, clo, chi, _ = code_windows(key)
    seen = 0
    for g in range(1, len(tab)):
        c = int(tab[g])
        if c in chains:  # a code that is not a lookup's answer is a shadowed duplicate
            k = np.searchsorted(codes, chains[c][0])
            assert int(win[g, 2]) == int(np.min(clo[k] + chains[c][1])), g
            assert int(win[g, 3]) == int(np.max(chi[k])), g
            seen += 1
    assert seen == len(chains)
    assert np.any(win[1:, 2] < win[1:, 0]) and np.any(win[1:, 3] > win[1:, 1])
    # refused: a wrong n, NULL arrays, min_start above 0x7FFFFFFF; nothing written
    big = lo.copy()
    big[len(big) // 2] = 0x80000000
    for rc, w in (_tables(img, lo, hi, len(lo) - 1), _tables(img, None, hi, len(hi)), _tables(img, lo, None, len(lo)),
                  _tables(img, big, hi)):
        assert rc == -2 and np.all(w == 0x5A5A5A5A)
    big[len(big) // 2] = 0x7FFFFFFF
    assert _tables(img, big, hi)[0] == 0


def test_a_shadowed_duplicates_window_is_ignored():
    pats = [b"admin", b"xadmin", b"admin", b"zzadmin"]
    lo = np.array([50, 0, 0, 0], dtype=np.uint32)
    hi = np.array([60, INF, 5, INF], dtype=np.uint32)
    for kind in (pm.KIND_RT, pm.KIND_AC):
        img = FlatImage(pats, kind)
        rc, win = _tables(img, lo, hi)
        assert rc == 0
        win = win.reshape(-1, 4)
        iog = img.array("index_of_gid").tolist()
        g = {k: iog.index(k, 1) for k in range(4)}
        assert win[g[0]].tolist()[:2] == [55, 60] and win[g[2]].tolist() == [5, 5, 5, 5]
        assert win[g[1]].tolist() == [6, INF, 5, INF] and win[g[3]].tolist() == [7, INF, 5, INF]
        # "xadmin" ending at byte 6 of its stream: "admin" (the later add, window (0, 5)) does not pass
        gids = np.array([0, 0, 0, 0, g[2], g[1]], dtype=np.uint32)
        rc, ev, total = _expand(img, gids, [0, 6], None, None, None, (lo, hi), 1, True, 8)
        assert rc == 0
        p, h = pm.unpack_events(ev[:total])
        assert list(zip(p.tolist(), h.tolist())) == [(4, g[2]), (5, g[1])]


def test_expand_windows_capacity_and_arguments():
    d, img, tab = image("et", pm.KIND_RT)
    _, offs, exp = input_t("et")
    gids = _gids_of(img, tab, exp)
    by_index, sg, win = masks_by_index(d), stream_masks(len(offs) - 1), windows_by_index(d)
    rc, full, total = _expand(img, gids, offs, None, sg, by_index, win, 3, True, len(exp) * 2)
    assert rc == 0 and total == len(expected_windows("et", exp, offs, None, sg, 3, True)[0])
    for cap in (0, 1, total // 2, total - 1):
        rc, ev, t = _expand(img, gids, offs, None, sg, by_index, win, 3, True, cap)
        assert rc == 0 and t == total, cap
        assert np.array_equal(ev[:cap], full[:cap]) and np.all(ev[cap:] == POISON64), cap
    # rejected, nothing written: min_len 0, a NULL window array, stream masks without pattern
    # masks, offsets that descend, a min_start above 0x7FFFFFFF, n > 2^40
    big = win[0].copy()
    big[3] = 0x80000000
    for kw in (dict(min_len=0), dict(win=(None, win[1])), dict(win=(win[0], None)), dict(by_index=None),
               dict(win=(big, win[1])), dict(n=(1 << 40) + 1)):
        a = dict(sg=sg, by_index=by_index, win=win, min_len=3, n=None)
        a.update(kw)
        rc, ev, t = _expand(img, gids, offs, None, a["sg"], a["by_index"], a["win"], a["min_len"], True, 16, a["n"])
        assert rc == -2 and t == 12345 and np.all(ev == POISON64), kw
    rc, ev, t = _expand(img, gids[:20], np.array([0, 10, 5, 20]), None, sg[:3].copy(), by_index, win, 3, True, 16)
    assert rc == -2 and t == 12345 and np.all(ev == POISON64)
    # no input, no streams, and gids that are none or out of range: no events
    rc, ev, t = _expand(img, np.zeros(0, np.uint32), np.array([0, 0]), None, None, None, win, 1, True, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, gids, np.array([0]), None, None, None, win, 1, True, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, np.array([0, len(tab), 0xFFFFFFFF], np.uint32), np.array([0, 3]), None, None, None, win, 1,
                        True, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    # a position past 2^32: the comparison is made in 64 bits
    one = np.array([int(np.nonzero(gids)[0][0])])
    g1 = gids[one[0]:one[0] + 1].copy()
    unb = windows_by_index(d, unbounded)
    far = np.array([(1 << 33) + 5], np.uint64)
    rc, ev, t = _expand(img, g1, np.array([0, 1]), far, None, None, unb, 1, True, 64)
    assert rc == 0 and t >= 1
    capped = (unb[0], np.full(len(unb[1]), 0xFFFFFFFE, np.uint32))
    rc, ev, t = _expand(img, g1, np.array([0, 1]), far, None, None, capped, 1, True, 64)
    assert rc == 0 and t == 0


def test_brute_force_without_the_oracle():
    """A dozen patterns with nested suffixes, a few hundred bytes, every
    occurrence found by bytes.find, windows and longest-visible in plain
    Python; the dense gids come from the longest occurrence per position."""
    pats = [b"/admin", b"admin", b"min", b"n", b"GET ", b"ET ", b"T ", b"MZ", b"Z", b"login", b"in", b"xlogin"]
    wins = [(0, INF), (5, INF), (0, 40), (30, 200), (0, 4), (0, INF), (2, 9), (0, 2), (100, INF), (0, INF), (7, 7),
            (20, 26)]
    rng = np.random.default_rng(17)
    words = pats + [b" ", b"ab", b"mi", b"ad", b"/", b"GE"]
    streams = []
    for k in range(6):
        body = b"".join(words[rng.integers(0, len(words))] for _ in range(25))
        streams.append([b"GET ", b"MZ", b"/admin", b"xlogin", b"", b"n"][k] + body)
    text = b"".join(streams)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in streams])]).astype(np.int64)
    pos_in = np.array([0, 0, 3, 0, 9, 1 << 32], dtype=np.uint64)
    assert 200 < len(text) < 1000
    occ = {}  # position of the last byte -> the pattern indexes ending there, inside one stream
    for j, s in enumerate(streams):
        for k, p in enumerate(pats):
            at = s.find(p)
            while at >= 0:
                occ.setdefault(int(offs[j]) + at + len(p) - 1, []).append(k)
                at = s.find(p, at + 1)
    lo = np.array([w[0] for w in wins], dtype=np.uint32)
    hi = np.array([w[1] for w in wins], dtype=np.uint32)
    for kind in (pm.KIND_RT, pm.KIND_AC):
        img = FlatImage(pats, kind)
        iog = img.array("index_of_gid").tolist()
        gid = {k: iog.index(k, 1) for k in range(len(pats))}
        gids = np.zeros(len(text), np.uint32)
        for i, ks in occ.items():
            gids[i] = gid[max(ks, key=lambda k: len(pats[k]))]
        for min_len in (1, 2, 3):
            for all_matches in (True, False):
                want = []
                for i in sorted(occ):
                    j = int(np.searchsorted(offs, i, side="right") - 1)
                    E = int(pos_in[j]) + i - int(offs[j]) + 1
                    vis = [k for k in occ[i] if len(pats[k]) >= min_len and E - len(pats[k]) >= wins[k][0]
                           and (wins[k][1] == INF or E <= wins[k][1])]
                    if vis and not all_matches:
                        vis = [max(vis, key=lambda k: len(pats[k]))]
                    want += sorted((i, gid[k]) for k in vis)
                rc, ev, total = _expand(img, gids, offs, pos_in, None, None, (lo, hi), min_len, all_matches,
                                        4 * len(text))
                assert rc == 0
                p, h = pm.unpack_events(ev[:total])
                assert list(zip(p.tolist(), h.tolist())) == want, (kind, min_len, all_matches)
                assert len(want) > 10
        # the anchors do what they are for
        rc, ev, total = _expand(img, gids, offs, pos_in, None, None, (lo, hi), 1, True, 4 * len(text))
        p, h = pm.unpack_events(ev[:total])
        got = set(zip(p.tolist(), h.tolist()))
        assert (3, gid[4]) in got and (int(offs[1]) + 1, gid[7]) in got
        assert sum(1 for _, g in got if g == gid[4]) == 1 and sum(1 for _, g in got if g == gid[7]) == 1


def _assert_stats(st, what):
    per_sel, cand, kept, differ, multi = st
    for s in (3, 4, 5, 6):
        assert 0 < per_sel[s][1] < per_sel[s][0], (what, s, per_sel[s])
    assert per_sel[7][0] > 0 and per_sel[7][1] == 0, (what, per_sel[7])
    assert 0 < kept < cand, (what, cand, kept)
    assert differ > 0 and multi > 0, (what, differ, multi)


def test_inputs_are_not_vacuous():
    """On inputs T and F every kind of window keeps some events and loses
    some, the unsatisfiable one has candidates and keeps none, the longest
    visible pattern differs from the dictionary's answer somewhere, and on
    input F a flow form that counted from the packet's first byte would both
    lose and gain events."""
    for key in ("et", "merged"):
        _, offs, exp = input_t(key)
        F = input_f(key)
        for min_len in (1, 3):
            _assert_stats(window_stats(key, exp, offs, None, min_len), ("T", key, min_len))
            _assert_stats(window_stats(key, F.exp, flows_as_streams(), None, min_len), ("F", key, min_len))
            lost, gained = packet_vs_flow(key, F, min_len)
            assert lost > 0 and gained > 0, (key, min_len, lost, gained)
