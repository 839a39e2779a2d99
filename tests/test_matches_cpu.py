"""The host-only pieces of the all-matches list (pm_hip.h, "all matches"):
pm_flat_expand_matches against the oracle's suffix lookup, its capacity and
argument rules, and the guards that keep the GPU tests' inputs from being
vacuous.  CPU only."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from event_inputs import expected_events
from flow_inputs import input_f
from match_inputs import expected_matches, longest_per_position, match_stats, sort_matches, suffix_chains
from oracle_lib import oracle_for
from test_tables_cpu import image

U32P = ctypes.POINTER(ctypes.c_uint32)
U64P = ctypes.POINTER(ctypes.c_uint64)
POISON64 = 0xA5A5A5A5A5A5A5A5


def _gids_of(img, tab, exp):
    """The dense gids of expected codes, through the image's index_of_gid
    (tab: gid -> code, table_emulator.gid_to_code)."""
    tab = np.asarray(tab, dtype=np.uint32)
    order = np.argsort(tab[1:], kind="stable")
    k = np.searchsorted(tab[1:][order], exp)
    k = np.minimum(k, len(order) - 1)
    g = (order[k] + 1).astype(np.uint32)
    g[exp == 0] = 0
    assert np.array_equal(tab[g][exp != 0], exp[exp != 0])
    return g


def _expand(img, gids, min_len, cap):
    ev = np.full(cap + 8, POISON64, dtype=np.uint64)
    total = ctypes.c_size_t(12345)
    rc = img.lib.pm_flat_expand_matches(img.h, gids.ctypes.data_as(U32P), len(gids), min_len,
                                        ev.ctypes.data_as(U64P), cap, ctypes.byref(total))
    return rc, ev, total.value


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_expand_matches_equals_the_oracles_suffix_lookup(key, kind):
    d, img, tab = image(key, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    _, _, exp = input_t(key)
    gids = _gids_of(img, tab, exp)
    for min_len in (1, 3, 5, 8):
        pos, codes = expected_matches(key, exp, min_len)
        rc, ev, total = _expand(img, gids, min_len, len(pos))
        assert rc == 0 and total == len(pos), (min_len, total, len(pos))
        assert np.all(ev[len(pos):] == POISON64)
        ev = ev[:len(pos)]
        assert np.all(ev[1:] > ev[:-1]), "ascending as plain u64, no event twice"
        gp, gg = pm.unpack_events(ev)
        gp, gc = sort_matches(gp, tab[gg])
        assert np.array_equal(gp, pos) and np.array_equal(gc, codes), min_len
        # consistency: the longest pattern per position is the events list
        hp, hc = longest_per_position(key, pos, codes)
        wp, wc = expected_events(key, exp, min_len)
        assert np.array_equal(hp, wp) and np.array_equal(hc, wc), min_len


def test_expand_matches_capacity_and_arguments():
    d, img, tab = image("et", pm.KIND_RT)
    _, _, exp = input_t("et")
    gids = _gids_of(img, tab, exp)
    rc, full, total = _expand(img, gids, 3, len(exp) * 2)
    assert rc == 0 and total == len(expected_matches("et", exp, 3)[0])
    for cap in (0, 1, total // 2, total - 1):
        rc, ev, t = _expand(img, gids, 3, cap)
        assert rc == 0 and t == total, cap
        assert np.array_equal(ev[:cap], full[:cap]) and np.all(ev[cap:] == POISON64), cap
    # count only, no array at all
    t = ctypes.c_size_t(0)
    assert img.lib.pm_flat_expand_matches(img.h, gids.ctypes.data_as(U32P), len(gids), 3, None, 0,
                                          ctypes.byref(t)) == 0 and t.value == total
    # rejected: min_len 0, n > 2^40; nothing written
    rc, ev, t = _expand(img, gids, 0, 16)
    assert rc == -2 and t == 12345 and np.all(ev == POISON64)
    t = ctypes.c_size_t(7)
    assert img.lib.pm_flat_expand_matches(img.h, gids.ctypes.data_as(U32P), (1 << 40) + 1, 3, None, 0,
                                          ctypes.byref(t)) == -2 and t.value == 7
    # no input, and gids that are none or out of range: no events
    rc, ev, t = _expand(img, np.zeros(0, np.uint32), 1, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)
    rc, ev, t = _expand(img, np.array([0, len(tab), 0xFFFFFFFF], np.uint32), 1, 4)
    assert rc == 0 and t == 0 and np.all(ev == POISON64)


def test_the_oracle_answers_with_the_looked_up_code():
    """match_inputs finds a suffix's code by its bytes; the oracle's own
    answers must be codes such a lookup gives (two patterns of equal bytes)."""
    for key in ("et", "merged"):
        chains = suffix_chains(key)
        _, _, exp = input_t(key)
        assert set(np.unique(exp[exp != 0]).tolist()) <= set(chains)


# heads / all events / positions with >= 3 events / most events at one position,
# computed on the CPU from the oracle
STATS_T = {("et", 1): (61467, 78702, 3711, 12), ("et", 3): (8211, 11774, 775, 10), ("et", 5): (5774, 7242, 209, 8),
           ("snort", 1): (61495, 89263, 5302, 18), ("snort", 3): (9234, 14602, 1024, 16),
           ("snort", 5): (5183, 7671, 425, 14),
           ("merged", 1): (64446, 98249, 6581, 24), ("merged", 3): (10947, 18256, 1470, 22),
           ("merged", 5): (6451, 10306, 671, 20)}
STATS_F = {("et", 1): (984177, 1274546, 63027, 17), ("et", 3): (139310, 203186, 13997, 15),
           ("et", 5): (100774, 129415, 4752, 13),
           ("merged", 1): (1029818, 1542021, 102922, 24), ("merged", 3): (173884, 268194, 19885, 22),
           ("merged", 5): (105601, 149982, 7819, 20)}


def test_inputs_are_not_vacuous():
    """On every input and min_len the GPU tests use there are more events
    than heads and a position with at least 3 events; at min_len 1 the list
    is longer than the buffer."""
    for (key, min_len), want in STATS_T.items():
        exp = input_t(key)[2]
        got = match_stats(key, exp, min_len)
        assert got[1] > got[0] and got[3] >= 3 and got[2] > 0, (key, min_len, got)
        assert got == want, (key, min_len, got)
        if min_len == 1:
            assert got[1] > len(exp)
    for (key, min_len), want in STATS_F.items():
        F = input_f(key)
        got = match_stats(key, F.exp, min_len)
        assert got[1] > got[0] and got[3] >= 3 and got[2] > 0, (key, min_len, got)
        assert got == want, (key, min_len, got)
        if min_len == 1:
            assert got[1] > len(F.exp)
    for key in ("et", "merged"):
        assert match_stats(key, input_f(key).exp, 8)[3] >= 3
