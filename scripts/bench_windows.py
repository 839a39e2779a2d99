#!/usr/bin/env python3
"""The window calls (pm_hip_scan_batch_windows_device,
pm_hip_scan_flows_windows_device, all form) beside the group calls they were
built on.

scripts/bench_groups.py's cells, inputs and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream (dense deep matches), cut into 1,500-byte and 100 KiB streams;
hipEvent times of REPS repetitions after warm-up, min and median, all of one
cell in one process.  The group table is bench_groups.py's (8 disjoint groups,
pattern p in group crc32(p) & 7) and every stream is on all groups.  Per
dictionary, text, cut and family (batch: an auto object's reverse-trie walk;
flows: an ac object's dense-row walk with a state and a byte count in and out
per stream, every flow at its first byte), in this order:
  groups_a     (a) the group call, min_len 3: the baseline;
  unbounded    (b) the window call with every window (0, unbounded), min_len 3:
               the baseline's list, plus one 16-B table entry per surviving
               chain member;
  first256     (c) the window call with a third of the patterns (crc32(p) % 3
               == 0) limited to the first 256 bytes of a stream, min_len 3;
  anchored     (d) the window call at min_len 1 with every pattern of at most 2
               bytes anchored at (0, len) and the rest unbounded: the short
               patterns a rule engine can only ask for with a window;
  ids          the dense-id call, the yardstick for (d)'s absolute time;
  groups_b     the group call once more: groups_b / groups_a is the run-to-run
               spread of one call.
The cursor is zeroed before every repetition (outside the timed region) and the
lists have room for every event.  Each window list is checked on the host
against the dense ids of the same call expanded through
pm_flat_expand_windows.

Every step runs in a child process under its own time limit; the first one
that fails ends the run.  Writes one JSON file (--out).
"""
import argparse
import ctypes
import json
import os
import platform
import statistics
import subprocess
import sys
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_DEVICE = 64 << 20
EVENTS_CAP = N_DEVICE // 2  # the lines stream holds an all-matches event per 3 to 5 bytes
CUTS = {"1500B": 1500, "100KiB": 100 << 10}
DICTS = {"snort": ["snort.dict"], "merged": ["snort.dict", "et.dict"]}
REPS, WARM = 20, 3
INF = 0xFFFFFFFF
STEP_SECONDS = 540


def stat(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2)}


def timed(torch, s, fn, pre=None, reps=REPS, warm=WARM):
    us = []
    for r in range(warm + reps):
        if pre:
            pre()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        fn()
        e1.record(s)
        torch.cuda.synchronize()
        if r >= warm:
            us.append(e0.elapsed_time(e1) * 1e3)
    return us


def step_dict(key):
    import numpy as np
    import torch
    import patternmatching_amd as pm
    lib = pm.load()
    d = pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", f) for f in DICTS[key]])
    pats = d.patterns()
    groups = np.array([1 << (zlib.crc32(p) & 7) for p in pats], dtype=np.uint32)
    zeros = np.zeros(len(pats), dtype=np.uint32)
    tables = {
        "unbounded": (zeros, np.full(len(pats), INF, dtype=np.uint32)),
        "first256": (zeros, np.array([256 if zlib.crc32(p) % 3 == 0 else INF for p in pats], dtype=np.uint32)),
        "anchored": (zeros, np.array([len(p) if len(p) <= 2 else INF for p in pats], dtype=np.uint32)),
    }
    min_len = {"unbounded": 3, "first256": 3, "anchored": 1}
    objs = {}
    for kind in ("ac", "auto"):
        m = pm.HipMatcher(kind)
        m.add_dictionary(d)
        m.compile()
        m.set_groups(groups)
        objs[kind] = m
    ac, auto = objs["ac"], objs["auto"]
    # the host twin: the flat image's gid order is pm_assign_gids', whatever the kind
    arr = (ctypes.c_char_p * len(pats))(*pats)
    plen = (ctypes.c_uint32 * len(pats))(*[len(p) for p in pats])
    flat = lib.pm_flat_build(arr, plen, len(pats), pm.KIND_RT)
    U32P, U64P, I64P = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))

    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(N, dtype=torch.int32, device="cuda")
    events = torch.zeros(EVENTS_CAP, dtype=torch.int64, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = int(lib.pm_hip_n_patterns(ac.obj))
    res = {"bytes": N, "patterns": P, "events_cap": EVENTS_CAP, "window_table_bytes": 16 * (P + 1),
           "patterns_of_at_most_2_bytes": int(sum(len(p) <= 2 for p in pats)),
           "patterns_limited_to_256": int(sum(zlib.crc32(p) % 3 == 0 for p in pats))}
    tp, ep, np_, op_ = text.data_ptr(), events.data_ptr(), nev.data_ptr(), out.data_ptr()

    def check(what, offs, masks, leg):
        """The window list just written == the dense ids just written,
        expanded by pm_flat_expand_windows on the host (every stream at byte 0)."""
        total = int(nev.item())
        assert total <= EVENTS_CAP, (what, total)
        ids = out.cpu().numpy().view(np.uint32)
        want = np.empty(total + 1, dtype=np.uint64)
        n_want = ctypes.c_size_t(0)
        lo, hi = tables[leg]
        rc = lib.pm_flat_expand_windows(flat, ids.ctypes.data_as(U32P), N, offs.ctypes.data_as(I64P), len(offs) - 1,
                                        None, masks.ctypes.data_as(U32P), groups.ctypes.data_as(U32P),
                                        lo.ctypes.data_as(U32P), hi.ctypes.data_as(U32P), min_len[leg], 1,
                                        want.ctypes.data_as(U64P), total + 1, ctypes.byref(n_want))
        assert rc == 0 and n_want.value == total, (what, rc, n_want.value, total)
        got = torch.sort(events[:total]).values.cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want[:total]), what
        return total

    for stream in ("ascii", "lines"):
        if stream == "ascii":
            lib.pm_hip_gen_stream_device(tp, 0, N + 64, 3, 0, sp)
        else:
            ac.gen_lines_device(tp, N + 64, 3, sp)
        torch.cuda.synchronize()
        for cut, L in CUTS.items():
            offs = np.append(np.arange(0, N, L, dtype=np.int64), np.int64(N))
            nseg = len(offs) - 1
            d_offs = torch.from_numpy(offs).cuda()
            op = d_offs.data_ptr()
            masks = np.full(nseg, 0xFFFFFFFF, dtype=np.uint32)
            d_masks = torch.from_numpy(masks.view(np.int32).copy()).cuda()
            ga = d_masks.data_ptr()
            st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
            ps = [torch.zeros(nseg, dtype=torch.int64, device="cuda") for _ in range(2)]
            # every flow begins here: the root state and byte count 0 in (a state carried in from an
            # earlier packet would need that packet's length as the count)
            s0, s1, p0, p1 = st[0].data_ptr(), st[1].data_ptr(), ps[0].data_ptr(), ps[1].data_ptr()
            calls = {
                "batch": {
                    "groups": lambda ml: auto.scan_batch_groups_device(tp, op, nseg, N, ga, ml, True, ep, EVENTS_CAP,
                                                                       np_, sp),
                    "windows": lambda ml: auto.scan_batch_windows_device(tp, op, nseg, N, ga, ml, True, ep, EVENTS_CAP,
                                                                         np_, sp),
                    "ids": lambda ml: auto.scan_batch_device(tp, op, nseg, N, op_, cnt.data_ptr(), sp),
                },
                "flows": {
                    "groups": lambda ml: ac.scan_flows_groups_device(tp, op, nseg, N, s0, s1, ga, ml, True, ep,
                                                                     EVENTS_CAP, np_, sp),
                    "windows": lambda ml: ac.scan_flows_windows_device(tp, op, nseg, N, s0, s1, ga, ml, True, ep,
                                                                       EVENTS_CAP, np_, sp, p0, p1),
                    "ids": lambda ml: ac.scan_flows_device(tp, op, nseg, N, s0, s1, op_, cnt.data_ptr(), sp),
                },
            }
            cell = {"stream_bytes": L, "streams": nseg}
            for family, c in calls.items():
                m = auto if family == "batch" else ac
                r = {}

                def leg(name, call, ml):
                    r[name] = stat(timed(torch, s, lambda: c[call](ml), pre=lambda: nev.zero_()))
                    if call != "ids":
                        total = int(nev.item())
                        assert total <= EVENTS_CAP, (name, total)
                        r[name]["events"] = total
                        r[name]["events_per_byte"] = round(total / N, 6)

                leg("groups_a", "groups", 3)
                c["ids"](3)  # the dense ids the window lists are checked against
                for name in ("unbounded", "first256", "anchored"):
                    m.set_windows(*tables[name])
                    leg(name, "windows", min_len[name])
                    nev.zero_()
                    c["windows"](min_len[name])
                    torch.cuda.synchronize()
                    assert check(f"{stream} {cut} {family} {name}", offs, masks, name) == r[name]["events"]
                leg("ids", "ids", 3)
                leg("groups_b", "groups", 3)
                assert r["unbounded"]["events"] == r["groups_a"]["events"]
                gt = min(r["groups_a"]["median_us"], r["groups_b"]["median_us"])
                r["unbounded_over_groups"] = round(r["unbounded"]["median_us"] / gt, 3)
                r["first256_over_groups"] = round(r["first256"]["median_us"] / gt, 3)
                r["anchored_over_ids"] = round(r["anchored"]["median_us"] / r["ids"]["median_us"], 3)
                r["groups_spread"] = round(max(r["groups_a"]["median_us"], r["groups_b"]["median_us"]) / gt, 3)
                r["first256_list_ratio"] = round(r["first256"]["events"] / max(r["groups_a"]["events"], 1), 4)
                cell[family] = r
            res[f"{stream}_{cut}"] = cell
    lib.pm_flat_free(flat)
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "windows", "bench_windows.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "window call (all form, every stream on all groups: every window unbounded; a third of the patterns "
                   "limited to the first 256 bytes; min_len 1 with the patterns of at most 2 bytes anchored at (0, "
                   "len)) vs the group call (timed twice: its spread) and the dense-id call; batched scan (auto kind) "
                   "and flow scan (ac kind, state and byte count in and out per stream, every flow at its first byte); 64 MiB, "
                   "gen_stream mode 0 seed 3 and the lines stream seed 3", "reps": REPS, "warmup": WARM,
           "library": os.environ.get("PM_LIBPM") or "in-tree"}
    for step, limit in [("box", 120)] + [(k, STEP_SECONDS) for k in DICTS]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True,
                               text=True, timeout=limit)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{step}: exit {p.returncode}; stopping\n{p.stderr[-3000:]}", file=sys.stderr)
            return 1
        doc[step] = json.loads(line[-1][7:])
        print(step, json.dumps(doc[step]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
