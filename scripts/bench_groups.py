#!/usr/bin/env python3
"""The group calls (pm_hip_scan_batch_groups_device,
pm_hip_scan_flows_groups_device, all form) beside the all-matches calls they
were built on.

scripts/bench_matches.py's cells, inputs and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream (dense deep matches), cut into 1,500-byte and 100 KiB streams;
hipEvent times of REPS repetitions after warm-up, min and median, all of one
cell in one process; min_len 3.  The group table is 8 disjoint groups, pattern
p in group crc32(p) & 7.  Per dictionary, text, cut and family (batch: an auto
object's reverse-trie walk; flows: an ac object's dense-row walk with a state
in and out per stream), in this order:
  matches_a    the all-matches call;
  groups_all   the group call, every stream on all groups (0xFFFFFFFF, as an
               array of masks): the sibling's list, plus the reach[] load per
               surviving position;
  groups_own   the group call, stream j on group j & 7: about an eighth of
               the list;
  matches_b    the all-matches call once more: matches_b / matches_a is the
               run-to-run spread of one binary's one call, the yardstick for
               groups_all_over_matches.
The cursor is zeroed before every repetition (outside the timed region) and the
lists have room for every event.  Each group list is checked on the host
against the dense ids of the same call expanded through pm_flat_expand_groups.

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
MIN_LEN = 3
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
    res = {"bytes": N, "patterns": P, "events_cap": EVENTS_CAP, "group_table_bytes": 2 * 4 * (P + 1)}
    tp, ep, np_, op_ = text.data_ptr(), events.data_ptr(), nev.data_ptr(), out.data_ptr()

    def check(what, offs, masks):
        """The group list just written == the dense ids just written, expanded
        by pm_flat_expand_groups on the host."""
        total = int(nev.item())
        assert total <= EVENTS_CAP, (what, total)
        ids = out.cpu().numpy().view(np.uint32)
        want = np.empty(total + 1, dtype=np.uint64)
        n_want = ctypes.c_size_t(0)
        rc = lib.pm_flat_expand_groups(flat, ids.ctypes.data_as(U32P), N, offs.ctypes.data_as(I64P), len(offs) - 1,
                                       masks.ctypes.data_as(U32P), groups.ctypes.data_as(U32P), MIN_LEN, 1,
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
            masks = {"all": np.full(nseg, 0xFFFFFFFF, dtype=np.uint32),
                     "own": (np.uint32(1) << (np.arange(nseg, dtype=np.uint32) & np.uint32(7))).astype(np.uint32)}
            d_masks = {k: torch.from_numpy(v.view(np.int32).copy()).cuda() for k, v in masks.items()}
            ga, go = d_masks["all"].data_ptr(), d_masks["own"].data_ptr()
            st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
            # the states the timed flow calls start from: an earlier call over the same buffer
            ac.scan_flows_device(tp, op, nseg, N, None, st[0].data_ptr(), None, None, sp)
            torch.cuda.synchronize()
            s0, s1 = st[0].data_ptr(), st[1].data_ptr()
            ml = MIN_LEN
            calls = {
                "batch": {
                    "matches": lambda: auto.scan_batch_matches_device(tp, op, nseg, N, ml, ep, EVENTS_CAP, np_, sp),
                    "groups_all": lambda: auto.scan_batch_groups_device(tp, op, nseg, N, ga, ml, True, ep, EVENTS_CAP,
                                                                        np_, sp),
                    "groups_own": lambda: auto.scan_batch_groups_device(tp, op, nseg, N, go, ml, True, ep, EVENTS_CAP,
                                                                        np_, sp),
                    "ids": lambda: auto.scan_batch_device(tp, op, nseg, N, op_, cnt.data_ptr(), sp),
                },
                "flows": {
                    "matches": lambda: ac.scan_flows_matches_device(tp, op, nseg, N, s0, s1, ml, ep, EVENTS_CAP, np_,
                                                                    sp),
                    "groups_all": lambda: ac.scan_flows_groups_device(tp, op, nseg, N, s0, s1, ga, ml, True, ep,
                                                                      EVENTS_CAP, np_, sp),
                    "groups_own": lambda: ac.scan_flows_groups_device(tp, op, nseg, N, s0, s1, go, ml, True, ep,
                                                                      EVENTS_CAP, np_, sp),
                    "ids": lambda: ac.scan_flows_device(tp, op, nseg, N, s0, s1, op_, cnt.data_ptr(), sp),
                },
            }
            cell = {"stream_bytes": L, "streams": nseg}
            for family, c in calls.items():
                r = {}
                for name, call in (("matches_a", "matches"), ("groups_all", "groups_all"),
                                   ("groups_own", "groups_own"), ("matches_b", "matches")):
                    r[name] = stat(timed(torch, s, c[call], pre=lambda: nev.zero_()))
                    total = int(nev.item())
                    assert total <= EVENTS_CAP
                    r[name]["events"] = total
                    r[name]["events_per_byte"] = round(total / N, 6)
                # each group list against the dense ids of the same call
                c["ids"]()
                for name in ("groups_all", "groups_own"):
                    nev.zero_()
                    c[name]()
                    torch.cuda.synchronize()
                    assert check(f"{stream} {cut} {family} {name}", offs, masks[name[7:]]) == r[name]["events"]
                assert r["groups_all"]["events"] == r["matches_a"]["events"]
                mt = min(r["matches_a"]["median_us"], r["matches_b"]["median_us"])
                r["groups_all_over_matches"] = round(r["groups_all"]["median_us"] / mt, 3)
                r["groups_own_over_matches"] = round(r["groups_own"]["median_us"] / mt, 3)
                r["matches_spread"] = round(max(r["matches_a"]["median_us"], r["matches_b"]["median_us"]) / mt, 3)
                r["own_list_ratio"] = round(r["groups_own"]["events"] / max(r["matches_a"]["events"], 1), 4)
                cell[family] = r
            res[f"{stream}_{cut}"] = cell
    lib.pm_flat_free(flat)
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "host": platform.node(), "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "groups", "bench_groups.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "group call (all form; every stream on all groups, and stream j on group j & 7) vs the all-matches "
                   "call (timed twice: its spread), min_len 3, 8 disjoint groups by crc32(pattern) & 7; batched scan "
                   "(auto kind) and flow scan (ac kind, state in and out per stream); 64 MiB, gen_stream mode 0 seed 3 "
                   "and the lines stream seed 3", "reps": REPS, "warmup": WARM, "min_len": MIN_LEN,
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
