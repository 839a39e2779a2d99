"""The host-only pieces of the match list (pm_hip.h, "match list"): the length
table and gid order the events kernels filter by, the event packing, and the
guards that keep the GPU tests' inputs from being vacuous.  CPU only."""
import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t
from event_inputs import expected_events, lengths_of
from flow_inputs import input_f
from test_tables_cpu import image


@pytest.mark.parametrize("key", ["et", "merged"])
def test_len_table_and_short_gids_first(key):
    d, img, tab = image(key, pm.KIND_RT)
    pats = d.patterns()
    idx = img.array("index_of_gid")
    ln = img.array("len")
    assert ln.dtype == np.uint32 and ln.shape == idx.shape == (len(pats) + 1,)
    assert ln[0] == 0
    assert np.array_equal(ln[1:], np.array([len(pats[int(k)]) for k in idx[1:]], dtype=np.uint32))
    # the kernels' reject without a load: gids 1..n_short are exactly the
    # patterns of <= 2 bytes, every other gid is longer
    n_short = img.lib.pm_flat_short_gids(img.h)
    assert n_short == sum(len(p) <= 2 for p in pats) and 0 < n_short < len(pats)
    assert np.all(ln[1:n_short + 1] <= 2) and np.all(ln[n_short + 1:] >= 3)
    # the AC image numbers the patterns the same way
    _, ac, _ = image(key, pm.KIND_AC)
    assert np.array_equal(ac.array("len"), ln) and ac.lib.pm_flat_short_gids(ac.h) == n_short


def test_unpack_events_round_trip():
    pos = np.array([0, 1 << 24, (1 << 40) - 1, 5], dtype=np.int64)
    gid = np.array([1, (1 << 24) - 1, (1 << 24) - 1, 0], dtype=np.uint32)
    ev = (pos.astype(np.uint64) << np.uint64(24)) | gid.astype(np.uint64)
    p, g = pm.unpack_events(ev)
    assert p.dtype == np.int64 and g.dtype == np.uint32
    assert np.array_equal(p, pos) and np.array_equal(g, gid)
    # u64 order is position order
    assert np.array_equal(np.argsort(ev), np.argsort(pos))
    p, g = pm.unpack_events(np.zeros(0, np.uint64))
    assert p.size == 0 and g.size == 0


def _straddlers(key, min_len):
    """Events of input F whose pattern began in an earlier packet of the flow:
    at position p of its packet, p + 1 < the pattern's length."""
    F = input_f(key)
    count = 0
    for data, offs, exp in F.calls:
        ln = lengths_of(key, exp)
        pos = np.nonzero(ln >= min_len)[0]
        start = offs[np.searchsorted(offs, pos, side="right") - 1]
        count += int(np.count_nonzero(pos - start + 1 < ln[pos]))
    return count


def test_inputs_are_not_vacuous():
    """min_len 3 keeps some positions and drops some, on both inputs, and on
    input F many events belong to patterns that straddle a packet boundary (a
    scan from each packet's first byte cannot find them)."""
    text, offs, exp = input_t("et")
    pos, codes = expected_events("et", exp, 3)
    assert 0 < len(pos) < np.count_nonzero(exp)
    assert np.all(codes != 0) and np.all(np.diff(pos) > 0)
    all_pos, _ = expected_events("et", exp, 1)
    assert np.array_equal(all_pos, np.nonzero(exp)[0])
    F = input_f("et")
    pos, _ = expected_events("et", F.exp, 3)
    assert 0 < len(pos) < np.count_nonzero(F.exp)
    # measured on the CPU: 10,357 events of input F (et, min_len 3) straddle a
    # packet boundary (8,485 at min_len 8; merged at min_len 4: 10,637)
    assert _straddlers("et", 3) >= 10357 // 2
