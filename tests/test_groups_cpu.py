"""The host-only pieces of the pattern groups (pm_hip.h, "pattern groups"):
pm_flat_group_tables and pm_flat_expand_groups against the oracle's suffix
lookup and the tests' own tables, their capacity and argument rules, and the
guards that keep the GPU tests' inputs from being vacuous.  CPU only."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from event_inputs import expected_events
from flow_inputs import F_FLOW_BYTES, F_FLOWS, input_f
from group_inputs import (ALL_GROUPS, all_ones, code_masks, expected_groups, group_stats, masks_by_index, pattern_mask,
                          stream_masks)
from match_inputs import expected_matches, sort_matches, suffix_chains
from table_emulator import FlatImage
from test_matches_cpu import POISON64, U32P, U64P, _gids_of
from test_tables_cpu import image

I64P = ctypes.POINTER(ctypes.c_int64)


def _expand(img, gids, offs, sgroups, by_index, min_len, all_matches, cap):
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(12345)
    offs = np.ascontiguousarray(offs, dtype=np.int64)
    rc = img.lib.pm_flat_expand_groups(img.h, gids.ctypes.data_as(U32P), len(gids), offs.ctypes.data_as(I64P),
                                       len(offs) - 1, None if sgroups is None else sgroups.ctypes.data_as(U32P),
                                       None if by_index is None else by_index.ctypes.data_as(U32P), min_len,
                                       int(all_matches), ev.ctypes.data_as(U64P), cap, ctypes.byref(total))
    return rc, ev, total.value


def _tables(img, by_index, n=None):
    G = len(img.array("index_of_gid"))
    gmask, reach = np.full(G, 0x5A5A5A5A, np.uint32), np.full(G, 0x5A5A5A5A, np.uint32)
    rc = img.lib.pm_flat_group_tables(img.h, None if by_index is None else by_index.ctypes.data_as(U32P),
                                      len(by_index) if n is None else n, gmask.ctypes.data_as(U32P),
                                      reach.ctypes.data_as(U32P))
    return rc, gmask, reach


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_expand_groups_equals_the_expected_lists(key, kind):
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    _, offs, exp = input_t(key)
    gids = _gids_of(img, tab, exp)
    by_index, sg = masks_by_index(d), stream_masks(len(offs) - 1)
    for min_len in (1, 3, 5):
        for all_matches in (True, False):
            pos, codes = expected_groups(key, exp, offs, sg, min_len, all_matches)
            rc, ev, total = _expand(img, gids, offs, sg, by_index, min_len, all_matches, len(pos))
            assert rc == 0 and total == len(pos), (min_len, all_matches, total, len(pos))
            assert np.all(ev[len(pos):] == POISON64)
            ev = ev[:len(pos)]
            assert np.all(ev[1:] > ev[:-1]), "ascending as plain u64, no event twice"
            gp, gg = pm.unpack_events(ev)
            gp, gc = sort_matches(gp, tab[gg])
            assert np.array_equal(gp, pos) and np.array_equal(gc, codes), (min_len, all_matches)


@pytest.mark.parametrize("key", ["et", "merged"])
def test_all_ones_tables_give_the_matches_and_the_events_lists(key):
    d, img, tab = image(key, pm.KIND_RT)
    tab = np.asarray(tab, dtype=np.uint32)
    _, offs, exp = input_t(key)
    gids = _gids_of(img, tab, exp)
    ones = masks_by_index(d, all_ones)
    for sg in (None, np.full(len(offs) - 1, ALL_GROUPS, np.uint32), np.full(len(offs) - 1, 1 << 31, np.uint32)):
        for min_len in (1, 3, 5):
            for all_matches, want in ((True, expected_matches(key, exp, min_len)),
                                      (False, expected_events(key, exp, min_len))):
                rc, ev, total = _expand(img, gids, offs, sg, ones, min_len, all_matches, len(want[0]))
                assert rc == 0 and total == len(want[0])
                gp, gg = pm.unpack_events(ev[:total])
                gp, gc = sort_matches(gp, tab[gg])
                assert np.array_equal(gp, want[0]) and np.array_equal(gc, want[1]), (min_len, all_matches)


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_group_tables(key, kind):
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    by_index = masks_by_index(d)
    rc, gmask, reach = _tables(img, by_index)
    assert rc == 0
    iog = img.array("index_of_gid")
    assert gmask[0] == 0 and reach[0] == 0
    assert np.array_equal(gmask[1:], by_index[iog[1:]])
    # reach: the OR over the suffixes the oracle's byte-string lookup finds
    chains = suffix_chains(key)
    codes, masks = code_masks(key)
    want = {c: int(np.bitwise_or.reduce(masks[np.searchsorted(codes, ch[0])])) for c, ch in chains.items()}
    seen = 0
    for g in range(1, len(tab)):
        c = int(tab[g])
        if c in want:  # a code that is not a lookup's answer is a shadowed duplicate (below)
            assert int(reach[g]) == want[c], g
            seen += 1
    assert seen == len(want)
    assert np.any(reach != gmask) and np.any(gmask == 0) and np.any((gmask == 0) & (reach != 0))
    # refused: a wrong n, NULL groups; nothing written
    for rc, a, b in (_tables(img, by_index, len(by_index) - 1), _tables(img, None, len(by_index))):
        assert rc == -2 and np.all(a == 0x5A5A5A5A) and np.all(b == 0x5A5A5A5A)


def test_a_shadowed_duplicates_mask_is_ignored():
    """A byte string added twice: the later add wins (pm_assign_gids), its
    mask is the pattern's, and the earlier add's mask reaches nobody's chain."""
    pats = [b"admin", b"xadmin", b"admin", b"zzadmin"]
    by_index = np.array([1 << 5, 1 << 1, 1 << 2, 1 << 3], dtype=np.uint32)
    for kind in (pm.KIND_RT, pm.KIND_AC):
        img = FlatImage(pats, kind)
        rc, gmask, reach = _tables(img, by_index)
        assert rc == 0
        iog = img.array("index_of_gid").tolist()
        g = {k: iog.index(k, 1) for k in range(4)}
        assert [int(gmask[g[k]]) for k in range(4)] == [1 << 5, 1 << 1, 1 << 2, 1 << 3]
        assert int(reach[g[2]]) == 1 << 2
        assert int(reach[g[1]]) == (1 << 1) | (1 << 2) and int(reach[g[3]]) == (1 << 3) | (1 << 2)
        # a scan answers "admin" with the later add: group 5 sees nothing, group 2 the pattern
        gids = np.array([g[1], g[2], g[3]], dtype=np.uint32)
        offs = np.array([0, 3], dtype=np.int64)
        for sm, want in ((1 << 5, []), (1 << 2, [(0, g[2]), (1, g[2]), (2, g[2])]), (1 << 1, [(0, g[1])])):
            for all_matches in (True, False):
                rc, ev, total = _expand(img, gids, offs, np.array([sm], np.uint32), by_index, 1, all_matches, 8)
                assert rc == 0
                p, h = pm.unpack_events(ev[:total])
                assert list(zip(p.tolist(), h.tolist())) == want, (sm, all_matches)


def test_expand_groups_capacity_and_arguments():
    d, img, tab = image("et", pm.KIND_RT)
    _, offs, exp = input_t("et")
    gids = _gids_of(img, tab, exp)
    by_index, sg = masks_by_index(d), stream_masks(len(offs) - 1)
    rc, full, total = _expand(img, gids, offs, sg, by_index, 3, True, len(exp) * 2)
    assert rc == 0 and total == len(expected_groups("et", exp, offs, sg, 3, True)[0])
    for cap in (0, 1, total // 2, total - 1):
        rc, ev, t = _expand(img, gids, offs, sg, by_index, 3, True, cap)
        assert rc == 0 and t == total, cap
        assert np.array_equal(ev[:cap], full[:cap]) and np.all(ev[cap:] == POISON64), cap
    # count only, no array at all
    t = ctypes.c_size_t(0)
    assert img.lib.pm_flat_expand_groups(img.h, gids.ctypes.data_as(U32P), len(gids), offs.ctypes.data_as(I64P),
                                         len(offs) - 1, sg.ctypes.data_as(U32P), by_index.ctypes.data_as(U32P), 3, 1,
                                         None, 0, ctypes.byref(t)) == 0 and t.value == total
    # rejected: min_len 0, no pattern masks, offsets that descend, n > 2^40; nothing written
    rc, ev, t = _expand(img, gids, offs, sg, by_index, 0, True, 16)
    assert rc == -2 and t == 12345 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, gids, offs, sg, None, 3, True, 16)
    assert rc == -2 and t == 12345 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, gids[:20], np.array([0, 10, 5, 20]), sg[:3].copy(), by_index, 3, True, 16)
    assert rc == -2 and t == 12345 and np.all(ev == POISON64)
    t = ctypes.c_size_t(7)
    assert img.lib.pm_flat_expand_groups(img.h, gids.ctypes.data_as(U32P), (1 << 40) + 1, offs.ctypes.data_as(I64P),
                                         len(offs) - 1, sg.ctypes.data_as(U32P), by_index.ctypes.data_as(U32P), 3, 1,
                                         None, 0, ctypes.byref(t)) == -2 and t.value == 7
    # no input, no streams, and gids that are none or out of range: no events
    rc, ev, t = _expand(img, np.zeros(0, np.uint32), np.array([0, 0]), sg[:1].copy(), by_index, 1, True, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, gids, np.array([0]), None, by_index, 1, True, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, np.array([0, len(tab), 0xFFFFFFFF], np.uint32), np.array([0, 3]), None, by_index, 1, True,
                        4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)


# unmasked all events / masked all events / masked longest events / those whose
# pattern is not the full dictionary's answer / positions with >= 2 masked
# events / streams with an event, computed on the CPU from the oracle
STATS_T = {("et", 1): (78702, 16199, 14251, 1552, 1485, 317), ("et", 3): (11774, 2290, 1957, 318, 274, 278),
           ("et", 5): (7242, 1379, 1261, 115, 111, 250),
           ("merged", 1): (98249, 19877, 15760, 2940, 2926, 319), ("merged", 3): (18256, 3906, 2832, 638, 680, 270),
           ("merged", 5): (10306, 2204, 1651, 380, 345, 240)}
# input F: its 256 flows as the streams (flow f keeps mask TABLE[f % 14] in every call)
STATS_F = {("et", 1): (1274546, 287574, 246714, 24765, 28602, 220), ("et", 3): (203186, 45210, 36512, 5452, 6205, 220),
           ("merged", 1): (1542021, 341059, 269148, 41488, 51232, 220),
           ("merged", 3): (268194, 60654, 46251, 7156, 9125, 220)}


def test_inputs_are_not_vacuous():
    """On every input the GPU tests use, the masks remove events, leave some,
    leave positions with several, and the longest visible pattern differs
    from the full dictionary's answer somewhere: the case a mask-filtered
    events list gets wrong."""
    for (key, min_len), want in STATS_T.items():
        _, offs, exp = input_t(key)
        got = group_stats(key, exp, offs, stream_masks(len(offs) - 1), min_len)
        assert got[0] > got[1] > got[2] > got[3] > 0 and got[4] > 0, (key, min_len, got)
        assert got == want, (key, min_len, got)
    flows = np.arange(F_FLOWS + 1, dtype=np.int64) * F_FLOW_BYTES
    for (key, min_len), want in STATS_F.items():
        got = group_stats(key, input_f(key).exp, flows, stream_masks(F_FLOWS), min_len)
        assert got[0] > got[1] > got[2] > got[3] > 0 and got[4] > 0, (key, min_len, got)
        assert got == want, (key, min_len, got)
    # every call of input F on its own (the flow tests' unit)
    for r, (data, offs, exp) in enumerate(input_f("et").calls[:20]):
        got = group_stats("et", exp, offs, stream_masks(F_FLOWS), 1)
        assert got[3] > 0 and got[4] > 0, (r, got)
