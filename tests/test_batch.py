"""The batched scan (pm_hip_scan_batch_device*, pm_hip_read_batch*): many
independent streams in one launch, every stream scanned from its own first
byte.  Expected values come from the oracle, reset() before each stream
(tests/batch_inputs.py).  Bit-exact."""
import ctypes

import numpy as np
import pytest

import patternmatching_amd as pm
from batch_inputs import input_t, oracle_per_stream, precondition
from test_gpu_parity import SHIP, _torch, matcher

pytestmark = pytest.mark.gpu

POISON = 0xA5A5A5A5
FORMS = {"persistent": 0, "small": 1 << 30}  # the "rt_small_max" option of each kernel form


def _stream(torch):
    return torch.cuda.current_stream().cuda_stream


def _dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()  # (a copy: the shared inputs are read-only)


def _poisoned(torch, n, width):
    """n ids of `width` bytes on the device, every byte 0xA5."""
    if width == 4:
        return torch.full((max(n, 4),), POISON - (1 << 32), dtype=torch.int32, device="cuda")
    return torch.full((max(n, 4),), (POISON & 0xFFFF) - (1 << 16), dtype=torch.int16, device="cuda")


def _ids(out, n, width):
    return out.cpu().numpy().view(np.uint32 if width == 4 else np.uint16)[:n].astype(np.uint32)


def _batch(m, torch, text, offs, width=4, want_out=True):
    """One device batch call: (gids or None, count)."""
    n = len(text)
    d_text = _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, np.asarray(offs, dtype=np.int64))
    out = _poisoned(torch, n, width) if want_out else None
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    m.scan_batch_device(d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, n, out.data_ptr() if want_out else None,
                        cnt.data_ptr(), _stream(torch), out_width=width)
    torch.cuda.synchronize()
    return (_ids(out, n, width) if want_out else None), int(cnt.item())


def _each_form(m):
    try:
        for name, v in FORMS.items():
            assert m.set_option("rt_small_max", v) == 0
            yield name
    finally:
        m.set_option("rt_small_max", -1)


def _assert_codes(m, gids, exp, what):
    got = m._codes[gids]
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, f"{what}: {bad.size} mismatches, first at {bad[:8]}"


@pytest.mark.parametrize("out_width", [4, 2])
@pytest.mark.parametrize("kind", ["rt", "auto"])
@pytest.mark.parametrize("key", ["et", "merged"])
def test_batch_equals_oracle_per_stream(key, kind, out_width):
    torch = _torch()
    text, offs, exp = input_t(key)
    differ, deep = precondition(key)
    assert differ >= 300 and deep >= 100
    m = matcher(key, kind)
    for form in _each_form(m):
        gids, cnt = _batch(m, torch, text, offs, out_width)
        _assert_codes(m, gids, exp, form)
        assert cnt == int(np.count_nonzero(exp)), form
        assert m.kernel_last == pm.KIND_RT


def test_batch_count_only():
    torch = _torch()
    text, offs, exp = input_t("et")
    m = matcher("et", "rt")
    for form in _each_form(m):
        gids, cnt = _batch(m, torch, text, offs, want_out=False)
        assert gids is None and cnt == int(np.count_nonzero(exp)), form


def test_batch_tile_seams():
    """600 tiles (a 256-CU grid takes more than two each); streams beginning
    at, just before and just after 64 tile edges; 2,048 one-byte streams (two
    tiles with every mask bit set); one 300 KiB stream (292 tiles that no
    stream begins in)."""
    torch = _torch()
    n = 600 * 1024
    text = pm.gen_stream(n, seed=9, mode=0)
    k = np.arange(1, 65, dtype=np.int64) * 1024
    big = 200000
    offs = np.unique(np.concatenate([[0], k - 1, k, k + 1, 100000 + np.arange(2049), [big, big + 300 * 1024], [n]]))
    assert offs[0] == 0 and offs[-1] == n and np.count_nonzero(np.diff(offs) == 1) >= 2048
    assert (big + 300 * 1024) in offs and offs[np.searchsorted(offs, big) + 1] == big + 300 * 1024
    exp = oracle_per_stream("snort", text, offs)
    m = matcher("snort", "rt")
    for form in _each_form(m):
        gids, cnt = _batch(m, torch, text, offs)
        _assert_codes(m, gids, exp, form)
        assert cnt == int(np.count_nonzero(exp)), form


def test_batch_single_stream_equals_scan_device():
    torch = _torch()
    text, _, _ = input_t("merged")
    n = len(text)
    m = matcher("merged", "rt")
    d_text = _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))
    ref = torch.zeros(n, dtype=torch.int32, device="cuda")
    m.scan_device(d_text.data_ptr(), 0, 0, n, ref.data_ptr(), None, _stream(torch))
    torch.cuda.synchronize()
    ref = _ids(ref, n, 4)
    for form in _each_form(m):
        gids, cnt = _batch(m, torch, text, [0, n])
        assert np.array_equal(gids, ref), form
        assert cnt == int(np.count_nonzero(ref))
    # nothing to scan: 0, no launch, the ids untouched
    d_offs = _dev(torch, np.array([0, 0, 0], dtype=np.int64))
    out = _poisoned(torch, n, 4)
    fn = m.lib.pm_hip_scan_batch_device
    assert fn(m.obj, d_text.data_ptr(), d_offs.data_ptr(), 0, n, out.data_ptr(), None, _stream(torch)) == 0
    assert fn(m.obj, d_text.data_ptr(), d_offs.data_ptr(), 2, 0, out.data_ptr(), None, _stream(torch)) == 0
    torch.cuda.synchronize()
    assert np.all(_ids(out, n, 4) == POISON)


def test_batch_host_forms():
    text, offs, exp = input_t("merged")
    m = matcher("merged", "rt")
    assert np.array_equal(m.read_batch_codes(text, offs), exp)
    assert m.scratch_bytes >= len(text) * 5 + len(offs) * 8
    streams = [text[a:b] for a, b in zip(offs[:-1], offs[1:])]
    streams[7] = bytes(streams[7])
    streams[9] = bytearray(streams[9].tobytes())
    many = m.read_many_codes(streams)
    assert len(many) == len(streams)
    for j, (a, b) in enumerate(zip(offs[:-1], offs[1:])):
        assert np.array_equal(many[j], exp[a:b]), j
    assert m.read_many_codes([]) == []
    # read_batch: the add_pattern ids of the gids
    gids = m.read_batch_gids(text, offs)
    size = ctypes.sizeof(pm._lib.PmPattern)
    P = m.lib.pm_hip_n_patterns(m.obj)
    pid = m.gid_codes(np.uint64(m._dict.pattern_ptr(0)) + np.arange(P, dtype=np.uint64) * np.uint64(size))
    assert np.array_equal(m.read_batch_id_array(text, offs).astype(np.uint64), pid[gids])
    # offsets the host form refuses
    n = len(text)
    out = np.full(n, POISON, dtype=np.uint32)
    for bad in ([1, n], [0, 10, 5, n]):
        o = np.array(bad, dtype=np.int64)
        rc = m.lib.pm_hip_read_batch_gid(m.obj, text.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         o.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(bad) - 1,
                                         out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
        assert rc == -2 and np.all(out == POISON)
        with pytest.raises(RuntimeError):
            m.read_batch_gids(text, o)


@pytest.mark.parametrize("kind", ["rt", "auto"])
def test_batch_leaves_carried_state_alone(kind):
    text, offs, exp = input_t("et")
    m = matcher("et", kind)
    whole = m.read_block_codes(SHIP)
    h = len(SHIP) // 2
    m.reset()
    first = m.read_block_codes(SHIP[:h])
    assert np.array_equal(m.read_batch_codes(text, offs), exp)
    second = m.read_block_codes(SHIP[h:])
    assert np.array_equal(np.concatenate([first, second]), whole)
    # read_char after a batch call continues the stream
    m.reset()
    head = m.read_block_codes(SHIP[:700])
    assert np.array_equal(m.read_batch_codes(text, offs), exp)
    tail = [m.lib.pm_pattern_code(m.read_char(int(c))) for c in SHIP[700:1000].tolist()]
    assert np.array_equal(head, whole[:700]) and tail == whole[700:1000].tolist()
    # with the resident server live when the batch call arrives (shallow
    # text: an auto object's pick then holds the reverse trie, which is served)
    piece = 20 << 10
    ascii_text = pm.gen_stream(12 * piece, 9, 0)
    m.reset()
    whole = m.read_block_codes(ascii_text)
    m.reset()
    s0 = m.serve_stats()["calls"]
    parts = [m.read_block_codes(ascii_text[k * piece:(k + 1) * piece]) for k in range(6)]
    assert m.serve_stats()["calls"] > s0
    assert np.array_equal(m.read_batch_codes(text, offs), exp)
    parts += [m.read_block_codes(ascii_text[k * piece:(k + 1) * piece]) for k in range(6, 12)]
    assert np.array_equal(np.concatenate(parts), whole)


def test_batch_unsupported_on_ac():
    torch = _torch()
    text, offs, _ = input_t("et")
    n = len(text)
    m = matcher("et", "ac")
    d_text = _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, offs)
    out = _poisoned(torch, n, 4)
    args = (m.obj, d_text.data_ptr(), d_offs.data_ptr(), len(offs) - 1, n, out.data_ptr(), None, _stream(torch))
    assert m.lib.pm_hip_scan_batch_device(*args) == -6
    assert b"reverse-trie image" in m.lib.pm_hip_last_error()
    out16 = _poisoned(torch, n, 2)
    assert m.lib.pm_hip_scan_batch_device16(*(args[:5] + (out16.data_ptr(),) + args[6:])) == -6
    h_out = np.full(n, POISON, dtype=np.uint32)
    rc = m.lib.pm_hip_read_batch_gid(m.obj, text.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                     offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(offs) - 1,
                                     h_out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    assert rc == -6 and np.all(h_out == POISON)
    assert b"reverse-trie image" in m.lib.pm_hip_last_error()
    ids = np.zeros(n, dtype=np.uintp)
    rc = m.lib.pm_hip_read_batch(m.obj, text.ctypes.data_as(ctypes.c_char_p),
                                 offs.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), len(offs) - 1,
                                 ids.ctypes.data_as(ctypes.POINTER(ctypes.c_void_p)))
    assert rc == -6
    with pytest.raises(RuntimeError, match="reverse-trie image"):
        m.scan_batch_device(*args[1:])
    torch.cuda.synchronize()
    assert np.all(_ids(out, n, 4) == POISON)


def test_batch_bad_arguments():
    torch = _torch()
    text, offs, _ = input_t("et")
    n = len(text)
    m = matcher("et", "rt")
    d_text = _dev(torch, np.concatenate([text, np.zeros(16, np.uint8)]))
    d_offs = _dev(torch, offs)
    out = _poisoned(torch, n + 16, 4)
    fn, s, nseg = m.lib.pm_hip_scan_batch_device, _stream(torch), len(offs) - 1
    t, o, d = d_text.data_ptr(), d_offs.data_ptr(), out.data_ptr()
    assert fn(m.obj, t + 1, o, nseg, n - 1, d, None, s) == -2
    assert fn(m.obj, t, o, nseg, n, d + 4, None, s) == -2
    assert fn(m.obj, t, o, -1, n, d, None, s) == -2
    assert fn(m.obj, t, o, nseg, -1, d, None, s) == -2
    assert m.lib.pm_hip_scan_batch_device16(m.obj, t, o, nseg, n, d + 2, None, s) == -2
    torch.cuda.synchronize()
    assert np.all(_ids(out, n + 16, 4) == POISON)
    raw = pm.HipMatcher("rt")
    raw.add_pattern(b"abc")
    assert fn(raw.obj, t, o, nseg, n, d, None, s) == -1
    h_out = np.zeros(4, dtype=np.uint32)
    o2 = np.array([0, 4], dtype=np.int64)
    assert raw.lib.pm_hip_read_batch_gid(raw.obj, text.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                         o2.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), 1,
                                         h_out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))) == -1
    raw.free()
