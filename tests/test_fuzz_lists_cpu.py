"""The random dictionaries of tests/fuzz_inputs.py through the host path of
the batch, flow and match-list scans: the numpy emulation of both kernels cut
per stream, pm_flat_expand_matches, pm_flat_expand_groups and
pm_flat_group_tables, against lists derived from the oracle's codes and its
pattern bytes alone; the table invariants the kernels lean on; the pinned
digests of test_fuzz.py's 36 pairs; and the guards that keep the GPU file
(test_fuzz_lists.py) from being vacuous.  CPU only."""
import zlib

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import oracle_per_stream
from event_inputs import expected_events
from fuzz_inputs import CASES, FAMILIES, GPU_CASES, N, UNARY_DEPTH, case, fuzz_case, stream_starts
from group_inputs import all_ones, code_masks, expected_groups, masks_by_index, stream_masks
from match_inputs import expected_matches, sort_matches, suffix_chains
from oracle_lib import oracle_for
from table_emulator import dfa_scan, rt_scan
from test_groups_cpu import _expand as _expand_groups
from test_groups_cpu import _tables
from test_matches_cpu import POISON64, _expand, _gids_of
from test_tables_cpu import image

MIN_LENS = (1, 2, 3, 4)

# crc32 of (the dictionary file, the 256 KiB text) of fuzz_case(seed, 256 << 10),
# seeds 0..35, taken before the generator moved out of test_fuzz.py
FUZZ_DIGESTS = [
    (2223674751, 2315478643), (3479903239, 3910823771), (2532715106, 3722357680), (772626932, 2130233888),
    (3252580983, 2584617707), (1323104984, 658375696), (756464403, 1556749913), (490489209, 2031587946),
    (564585600, 4041405422), (2866470057, 1245521783), (3718559287, 1909718678), (4267713332, 3320646502),
    (2923174910, 3730989338), (2286285763, 4259113137), (320545868, 671040724), (2663329304, 1768032154),
    (4141759384, 320532014), (910472724, 559371063), (612334620, 3912791217), (1170398219, 4272699509),
    (3399487461, 3744826188), (3605730504, 1093433432), (2294298169, 265159671), (1248227794, 539190644),
    (1199917589, 3639092588), (3271279824, 2517676734), (1964081344, 1231056708), (3047255264, 3920068825),
    (275965677, 2336888963), (1151499577, 1965043768), (2356592227, 771762379), (2341783319, 2756050490),
    (1076791844, 4036310327), (2995884858, 2264279639), (1593341767, 102186579), (1313440746, 3144168903)]


@pytest.mark.parametrize("seed", range(36))
def test_fuzz_pairs_are_byte_identical(seed):
    data, text = fuzz_case(seed, 256 << 10)
    assert (zlib.crc32(data), zlib.crc32(text.tobytes())) == FUZZ_DIGESTS[seed]
    # a shorter stream is a prefix of it (test_fuzz_images_cpu's 6,000 bytes)
    data6, text6 = fuzz_case(seed, 6000)
    assert data6 == data and np.array_equal(text6, text[:6000])


def test_rt_scan_emulation_takes_short_texts():
    d, img, tab = image("et", pm.KIND_RT)
    text = np.frombuffer(b"GET", np.uint8)
    want = tab[rt_scan(img, np.concatenate([text, text]))][:3]
    for n in range(4):
        assert np.array_equal(tab[rt_scan(img, text[:n])], want[:n]), n


# ---- the host path -----------------------------------------------------------------
def _emulated_gids(c, kind, img):
    """(gids of A per stream, gids of B continuing A per stream or None)."""
    if kind == pm.KIND_RT:
        return rt_scan(img, c.A, stream_start=stream_starts(c.offs, N)), None
    ga, gb = np.zeros(N, np.uint32), np.zeros(N, np.uint32)
    for a, b in zip(c.offs[:-1].tolist(), c.offs[1:].tolist()):
        if b > a:
            both = dfa_scan(img, np.concatenate([c.A[a:b], c.B[a:b]]))
            ga[a:b], gb[a:b] = both[:b - a], both[b - a:]
    return ga, gb


def _assert_events(ev, total, tab, want, what):
    assert total == len(want[0]), f"{what}: {total} events, expected {len(want[0])}"
    assert np.all(ev[total:] == POISON64)
    ev = ev[:total]
    assert np.all(ev[1:] > ev[:-1]), f"{what}: ascending as plain u64, no event twice"
    gp, gg = pm.unpack_events(ev)
    gp, gc = sort_matches(gp, tab[gg])
    assert np.array_equal(gp, want[0]) and np.array_equal(gc, want[1]), what


@pytest.mark.parametrize("kind", [pm.KIND_RT, pm.KIND_AC])
@pytest.mark.parametrize("name", CASES)
def test_host_path_equals_the_oracles_lists(name, kind):
    c = case(name)
    d, img, tab = image(name, kind)
    tab = np.asarray(tab, dtype=np.uint32)
    if kind == pm.KIND_RT:
        assert img.fits()
    by_index, ones, sg = masks_by_index(d), masks_by_index(d, all_ones), stream_masks(c.nseg)
    # the oracle answers with codes the suffix lookup knows (two lines of equal bytes)
    chains = suffix_chains(name)
    for exp in (c.ea, c.eb):
        assert set(np.unique(exp[exp != 0]).tolist()) <= set(chains)
    for gids, exp in zip(_emulated_gids(c, kind, img), (c.ea, c.eb)):
        if gids is None:
            continue
        assert np.array_equal(tab[gids], exp), "the emulated scan, per stream"
        assert np.array_equal(gids, _gids_of(img, tab, exp))
        for min_len in MIN_LENS:
            want = expected_matches(name, exp, min_len)
            rc, ev, total = _expand(img, gids, min_len, len(want[0]))
            assert rc == 0
            _assert_events(ev, total, tab, want, f"matches, min_len {min_len}")
            heads = expected_events(name, exp, min_len)
            for all_matches in (True, False):
                want_g = expected_groups(name, exp, c.offs, sg, min_len, all_matches)
                rc, ev, total = _expand_groups(img, gids, c.offs, sg, by_index, min_len, all_matches, len(want_g[0]))
                assert rc == 0
                _assert_events(ev, total, tab, want_g, f"groups, all {all_matches}, min_len {min_len}")
                # all-ones pattern masks, no stream masks: the matches list and the events list
                plain = want if all_matches else heads
                rc, ev, total = _expand_groups(img, gids, c.offs, None, ones, min_len, all_matches, len(plain[0]))
                assert rc == 0
                _assert_events(ev, total, tab, plain, f"all-ones groups, all {all_matches}, min_len {min_len}")
    # the group tables: gmask by pattern, reach the OR over the oracle's suffix lookup
    rc, gmask, reach = _tables(img, by_index)
    assert rc == 0 and gmask[0] == 0 and reach[0] == 0
    iog = img.array("index_of_gid")
    assert np.array_equal(gmask[1:], by_index[iog[1:]])
    codes, masks = code_masks(name)
    for g in range(1, len(tab)):
        ch = chains.get(int(tab[g]))
        if ch is not None:
            assert int(reach[g]) == int(np.bitwise_or.reduce(masks[np.searchsorted(codes, ch[0])])), g


@pytest.mark.parametrize("name", CASES)
def test_table_invariants(name):
    """What the kernels take from the tables without checking: gids
    1..n_short are exactly the patterns of <= 2 bytes (also when there are
    none, and when there are no others), parent[] is the longest proper suffix
    that is a pattern, and max_depth (the largest depth[]) bounds every chain."""
    case(name)
    d, img, _ = image(name, pm.KIND_RT)
    _, ac, _ = image(name, pm.KIND_AC)
    pats = d.patterns()
    assert len(set(pats)) == len(pats)
    for im in (img, ac):
        idx = im.array("index_of_gid").astype(np.int64)
        ln = im.array("len").astype(np.int64)
        parent = im.array("parent").astype(np.int64)
        depth = im.array("depth").astype(np.int64)
        assert len(idx) == len(pats) + 1 and ln[0] == 0
        assert np.array_equal(ln[1:], np.array([len(pats[k]) for k in idx[1:]]))
        n_short = int(im.lib.pm_flat_short_gids(im.h))
        assert n_short == sum(len(p) <= 2 for p in pats)
        assert np.all(ln[1:n_short + 1] <= 2) and np.all(ln[n_short + 1:] > 2)
        gid_of = {pats[k]: g for g, k in enumerate(idx.tolist()) if g}
        deepest = 0
        for g in range(1, len(idx)):
            b = pats[idx[g]]
            sufs = [gid_of[b[k:]] for k in range(1, len(b)) if b[k:] in gid_of]
            assert parent[g] == (sufs[0] if sufs else 0), g
            assert depth[g] == len(sufs) + 1, g
            deepest = max(deepest, len(sufs) + 1)
        assert int(depth.max()) >= deepest > 0


# ---- non-vacuity guards ----------------------------------------------------------------
def guard_row(name):
    """(patterns, n_short, positions of A answered by a gid >= 4,095, by one
    below, the deepest suffix chain, all events of A at min_len 1, heads of A
    at min_len 3, positions >= 8 bytes into their stream whose per-stream
    answer differs from the unsegmented scan of A, positions >= 8 bytes into
    their stream whose call-2 answer differs from a fresh scan of B)."""
    c = case(name)
    d, img, tab = image(name, pm.KIND_AC)
    gids = _gids_of(img, tab, c.ea)
    chains = suffix_chains(name)
    deep = np.arange(N) - stream_starts(c.offs, N) >= 8
    o = oracle_for(name)
    o.reset()
    whole = o.scan_codes(c.A)
    o.reset()
    fresh = oracle_per_stream(name, c.B, c.offs)
    return (len(tab) - 1, int(img.lib.pm_flat_short_gids(img.h)), int(np.count_nonzero(gids >= 4095)),
            int(np.count_nonzero((gids > 0) & (gids < 4095))), max(len(ch[0]) for ch in chains.values()),
            len(expected_matches(name, c.ea, 1)[0]), len(expected_events(name, c.ea, 3)[0]),
            int(np.count_nonzero((whole != c.ea) & deep)), int(np.count_nonzero((fresh != c.eb) & deep)))


GUARDS = {
    'no_short': (158, 0, 0, 43717, 5, 65662, 43717, 254, 254),
    'only_short': (34, 34, 0, 47756, 2, 73807, 0, 0, 0),
    'many': (6606, 72, 287, 48865, 6, 146449, 40621, 232, 231),
    'unary': (53, 4, 0, 49152, 48, 921776, 42590, 6010, 5454),
    'seed0': (27, 3, 0, 29950, 7, 76612, 18008, 226, 224),
    'seed1': (232, 12, 0, 49152, 7, 145897, 35108, 233, 232),
    'seed2': (2142, 20, 0, 49152, 11, 185419, 48617, 265, 267),
    'seed3': (46, 2, 0, 4239, 3, 4781, 1163, 285, 281),
    'seed4': (329, 40, 0, 5869, 3, 6253, 1112, 242, 240),
    'seed5': (2860, 370, 0, 16094, 6, 16851, 1086, 249, 248),
    'seed6': (22, 4, 0, 49005, 5, 92946, 24141, 234, 233),
    'seed7': (239, 11, 0, 49152, 7, 136341, 33263, 271, 274),
    'seed8': (2153, 20, 0, 49152, 8, 187752, 48617, 267, 265),
    'seed9': (45, 1, 0, 1540, 2, 1645, 1254, 307, 307),
    'seed10': (327, 40, 0, 6828, 4, 7181, 1130, 254, 254),
    'seed11': (2845, 428, 0, 18816, 7, 19694, 1143, 251, 251),
    'seed12': (26, 3, 0, 33055, 5, 77665, 21563, 236, 235),
    'seed13': (239, 11, 0, 49152, 7, 145320, 38360, 264, 263),
    'seed14': (2126, 20, 0, 49152, 9, 191049, 48617, 248, 246),
    'seed15': (45, 4, 0, 4657, 4, 5028, 1187, 235, 234),
    'seed16': (324, 50, 0, 7379, 6, 7911, 1081, 249, 248),
    'seed17': (2863, 388, 0, 15687, 7, 16492, 1158, 263, 261),
}


def test_guard_table():
    """Conditions on the case set, computed from the oracle; the figures are
    pinned so that a change of an input shows."""
    rows = {name: guard_row(name) for name in CASES}
    assert rows == GUARDS, rows
    # (of the cases the GPU file runs)
    by = lambda f: [name for name in GPU_CASES if f(rows[name])]  # noqa: E731
    assert by(lambda r: r[1] == 0), "a case without short patterns"
    assert by(lambda r: r[1] == r[0]), "a case with short patterns only"
    assert by(lambda r: r[2] >= 50 and r[3] >= 50), "a case with escaped and inline answers of the coded DFA"
    assert by(lambda r: r[4] >= UNARY_DEPTH and r[5] >= 16 * N), "a deep chain with >= 16 events per position"
    assert by(lambda r: r[6] >= 0.9 * N), "cases that take the flow kernels' direct path from the heads alone"
    assert by(lambda r: r[6] < 0.05 * N), "cases whose waves flush once at the end"
    for name, r in rows.items():
        if r[6] >= 0.2 * N:  # dense: the boundaries and the carried states matter deep inside the streams
            assert r[7] >= 100 and r[8] >= 100, (name, r)


def test_the_bytes_0x00_and_0xff():
    """Both are pattern bytes of the unary family and the first byte of streams
    of its A and of its B; a dictionary over all 256 byte values has both in
    the middle of patterns."""
    c = case("unary")
    pats = [b for _, _, b in oracle_for("unary").patterns()]
    first = c.offs[:-1][np.diff(c.offs) > 0]
    wide = [b for _, _, b in oracle_for(case("seed5").key).patterns()]
    for byte in (0x00, 0xFF):
        assert any(byte in p for p in pats)
        assert np.any(c.A[first] == byte) and np.any(c.B[first] == byte)
        assert any(byte in p[1:-1] for p in wide)
