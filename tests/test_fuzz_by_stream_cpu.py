"""The lists test_fuzz_by_stream.py groups on the device, grouped here on the
host from the oracle's lists alone: by_stream_inputs.grouped_from_list (numpy
sorting on (position, code) pairs) against by_stream_inputs.reference and
pm_flat_events_by_stream (both on position << 24 | gid events, through the
image's gid table) -- three derivations of one answer -- and the conditions on
the inputs that keep the GPU file from being vacuous.  The cases, forms and
launch options of both files are chosen here.  CPU only."""
import numpy as np
import pytest

import patternmatching_amd as pm
from by_stream_inputs import grouped_from_list, list_keys, pack, reference
from event_inputs import code_lengths, expected_events
from fuzz_inputs import GPU_CASES, case
from group_inputs import expected_groups, stream_masks
from match_inputs import expected_matches
from test_matches_cpu import _gids_of
from test_tables_cpu import image
from window_inputs import expected_windows, fuzz_window_of

CASES = ("unary", "many", "no_short", "seed0", "seed5")  # seed0: 2 symbols, seed5: 256
FORMS = ("events", "matches", "groups_all", "groups_longest", "windows")
TRUNCATED_CASES = ("unary", "seed0")
GROUP_MIN_LEN = 2

_want = {}


def want(c, which, form):
    """The oracle's (positions, codes) list, ascending by (position, code), of
    text `which` ("a": A, every stream from its first byte; "b": B continuing
    A, every stream len(A_j) bytes in) in a form: events and matches at min_len
    1, groups (all matches and longest) at min_len 2 under stream_masks,
    windows (all matches, min_len 1) under stream_masks and fuzz_window_of."""
    k = (c.key, which, form)
    if k not in _want:
        exp = c.ea if which == "a" else c.eb
        if form == "events":
            _want[k] = expected_events(c.key, exp, 1)
        elif form == "matches":
            _want[k] = expected_matches(c.key, exp, 1)
        elif form == "windows":
            pos_in = None if which == "a" else np.diff(c.offs).astype(np.uint64)
            _want[k] = expected_windows(c.key, exp, c.offs, pos_in, stream_masks(c.nseg), 1, True, fn=fuzz_window_of)
        else:
            _want[k] = expected_groups(c.key, exp, c.offs, stream_masks(c.nseg), GROUP_MIN_LEN, form == "groups_all")
    return _want[k]


def launch_option(name, form):
    """0 or 1: which value of rt_small_max (-1, 0) / flow_seg (0, 16) a form
    runs with in a case.  Consecutive forms alternate and consecutive cases
    start on the other value, so every form meets both across the cases."""
    return (CASES.index(name) + FORMS.index(form)) % 2


def test_every_form_meets_both_launch_shapes():
    assert set(CASES) <= set(GPU_CASES)
    for form in FORMS:
        assert {launch_option(name, form) for name in CASES} == {0, 1}, form


def _keys_of(tab, ptr, ev):
    """The twin's events as (position, code) keys, each stream's range
    ascending again: gids and codes order differently at one position."""
    p, g = pm.unpack_events(ev)
    keys = list_keys(p, tab[g])
    seg = np.repeat(np.arange(len(ptr) - 1), np.diff(ptr))
    return keys[np.lexsort((keys, seg))]


def _streams(offs, pos):
    return np.searchsorted(offs, pos, side="right") - 1


def _stats(c, which, form):
    """Figures of one list, from the oracle's list and the offsets alone."""
    pos, codes = want(c, which, form)
    offs, nseg = c.offs, c.nseg
    j = _streams(offs, pos)
    assert len(pos) and j.min() >= 0 and j.max() < nseg  # every event of a scan lies in a stream
    plain = len(pos)
    pair, per_pair = np.unique((j.astype(np.uint64) << np.uint64(32)) | codes.astype(np.uint64), return_counts=True)
    has = np.zeros(nseg, bool)
    has[j] = True
    lens = np.diff(offs)
    # an empty stream with an event-holding stream right before the run of empty streams it lies in, and one after
    between = any(lens[s] == 0 and has[:s].any() and has[s + 1:].any() for s in np.nonzero(lens == 0)[0].tolist())
    runs = j[:len(j) // 64 * 64].reshape(-1, 64)  # (the list is position-sorted: streams ascend)
    spans = runs[:, -1] - runs[:, 0]
    distinct = np.array([len(np.unique(r)) for r in runs[spans >= 7]]) if len(runs) else np.zeros(0, int)
    cl, ll = code_lengths(c.key)
    before = pos - ll[np.searchsorted(cl, codes)] + 1 < offs[j]  # the match began before the stream's first byte here
    return {"plain": plain, "unique": len(pair), "deepest_pair": int(per_pair.max()),
            "silent_streams": int(np.count_nonzero((lens > 0) & ~has)), "empty_between": between,
            "run_in_one_stream": bool(len(runs) and (spans == 0).any()),
            "run_over_8_streams": bool(len(distinct) and distinct.max() >= 8),
            "began_before": int(np.count_nonzero(before))}


@pytest.mark.parametrize("name", CASES)
def test_three_derivations_agree(name):
    """grouped_from_list == reference == pm_flat_events_by_stream on every list
    the GPU file makes, in the order a device never gives (shuffled)."""
    c = case(name)
    d, img, tab = image(name, pm.KIND_AC)
    tab = np.asarray(tab, dtype=np.uint32)
    assert len(np.unique(tab[1:])) == len(tab) - 1, "a code names one gid"
    rng = np.random.default_rng(7)
    for which in ("a", "b"):
        for form in FORMS:
            pos, codes = want(c, which, form)
            assert np.all(np.diff(list_keys(pos, codes).astype(np.int64)) > 0), "ascending, no event twice"
            events = pack(pos, _gids_of(img, tab, codes))
            rng.shuffle(events)
            for unique in (False, True):
                what = f"{name}, text {which}, {form}, unique {unique}"
                exp_ptr, exp_keys = grouped_from_list(pos, codes, c.offs, unique)
                for ptr, ev in (reference(events, c.offs, unique), pm.events_by_stream_host(events, c.offs, unique)):
                    assert np.array_equal(ptr, exp_ptr), what
                    assert np.array_equal(_keys_of(tab, ptr, ev), exp_keys), what
                if not unique:
                    assert exp_ptr[-1] == len(pos), what


def test_truncated_lists_are_any_subset():
    """What the GPU file asserts of a list that overflowed holds for any half
    of a list: the twin of a subset keeps members of the full list."""
    rng = np.random.default_rng(8)
    for name in TRUNCATED_CASES:
        c = case(name)
        d, img, tab = image(name, pm.KIND_AC)
        tab = np.asarray(tab, dtype=np.uint32)
        for which in ("a", "b"):
            pos, codes = want(c, which, "matches")
            full = list_keys(pos, codes)
            half = rng.permutation(len(pos))[:len(pos) // 2]
            events = pack(pos[half], _gids_of(img, tab, codes[half]))
            for unique in (False, True):
                exp_ptr, exp_keys = grouped_from_list(pos[half], codes[half], c.offs, unique)
                ptr, ev = pm.events_by_stream_host(events, c.offs, unique)
                keys = _keys_of(tab, exp_ptr, ev)
                assert np.array_equal(ptr, exp_ptr) and np.array_equal(keys, exp_keys)
                assert np.all(np.isin(keys, full))
                assert unique or ptr[-1] == len(half)


def test_the_lists_stress_the_grouping():
    """Conditions on the chosen cases, from the oracle's lists alone; each
    names the case it must hold in."""
    rows = {(name, which, form): _stats(case(name), which, form)
            for name in CASES for which in ("a", "b") for form in FORMS}
    # UNIQUE keeps fewer events than plain in every case (its events and matches lists, both texts: a
    # group form of seed5 keeps a few hundred events and may hold no pair twice); in unary under half,
    # in every form
    for k, r in rows.items():
        if k[2] in ("events", "matches"):
            assert r["unique"] < r["plain"], (k, r)
        if k[0] == "unary":
            assert 2 * r["unique"] < r["plain"], (k, r)
    # a whole wave on one table slot: unary, all matches (x^k ends at hundreds of positions of a stream)
    assert rows[("unary", "a", "matches")]["deepest_pair"] >= 64
    assert rows[("unary", "b", "matches")]["deepest_pair"] >= 64
    # a non-empty stream without an event: seed5's sparse lists (256 symbols), and the group forms of
    # every case (stream_masks has streams in no group)
    assert rows[("seed5", "a", "events")]["silent_streams"] > 0
    for name in CASES:
        assert rows[(name, "a", "groups_all")]["silent_streams"] > 0, name
    # an empty stream between two streams with events: the head lengths 4, 0, 0, 5 of every case
    assert rows[("unary", "a", "events")]["empty_between"] and rows[("seed0", "b", "matches")]["empty_between"]
    # an aligned run of 64 events in one stream and one over at least 8 streams, in one list:
    # unary's events (a 4,097-byte stream; the head lengths 1, 2, 3, 4, 5, 15, 16, 17 in 63 bytes)
    for which in ("a", "b"):
        r = rows[("unary", which, "events")]
        assert r["run_in_one_stream"] and r["run_over_8_streams"], which
    assert rows[("seed0", "a", "matches")]["run_in_one_stream"]
    # call 2's lists hold events of patterns that began in call 1 (plant_straddlers), call 1's none
    for name in CASES:
        assert case(name).planted > 0
        for form in FORMS:
            assert rows[(name, "a", form)]["began_before"] == 0, (name, form)
        assert rows[(name, "b", "matches")]["began_before"] > 0, name
        assert rows[(name, "b", "events")]["began_before"] > 0, name
