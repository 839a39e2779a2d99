#!/usr/bin/env python3
"""The all-matches list (pm_hip_scan_batch_matches_device,
pm_hip_scan_flows_matches_device) beside the two calls it was built on: the
longest-only events call and the dense u32 ids.

scripts/bench_events.py's cells, inputs and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream (dense deep matches), cut into 1,500-byte and 100 KiB streams;
hipEvent times of REPS repetitions after warm-up, min and median, all of one
cell in one process; min_len 3.  Per dictionary, text, cut and family (batch:
an auto object's reverse-trie walk; flows: an ac object's dense-row walk with
a state in and out per stream), in this order:
  events_a   the longest-only events call;
  matches    the all-matches call;
  ids        the dense u32 call;
  events_b   the longest-only events call once more: events_b / events_a is
             the run-to-run spread of one binary's one call, the yardstick for
             matches_over_events.
The cursor is zeroed before every repetition (outside the timed region) and the
lists have room for every event.  The all-matches list is checked on the
device against the dense ids expanded through pm_hip_parent_gid and filtered
by pm_hip_pattern_len.

Every step runs in a child process under its own time limit; the first one
that fails ends the run.  Writes one JSON file (--out).
"""
import argparse
import json
import os
import platform
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_DEVICE = 64 << 20
EVENTS_CAP = N_DEVICE // 2  # the lines stream holds an all-matches event per 3 to 5 bytes
CUTS = {"1500B": 1500, "100KiB": 100 << 10}
DICTS = {"snort": ["snort.dict"], "merged": ["snort.dict", "et.dict"]}
REPS, WARM = 20, 3
MIN_LEN = 3
STEP_SECONDS = 420


def stat(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2)}


def matcher(pm, kind, key):
    m = pm.HipMatcher(kind)
    m.add_dictionary(pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", f) for f in DICTS[key]]))
    m.compile()
    return m


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
    ac, auto = matcher(pm, "ac", key), matcher(pm, "auto", key)
    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(N, dtype=torch.int32, device="cuda")
    events = torch.zeros(EVENTS_CAP, dtype=torch.int64, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    P = int(lib.pm_hip_n_patterns(ac.obj))
    lens = torch.tensor([ac.pattern_len(g) for g in range(P + 1)], dtype=torch.int64, device="cuda")
    parent = torch.tensor([lib.pm_hip_parent_gid(ac.obj, g) for g in range(P + 1)], dtype=torch.int64, device="cuda")
    assert [auto.pattern_len(g) for g in (1, P // 2, P)] == [ac.pattern_len(g) for g in (1, P // 2, P)]
    assert int(parent[0]) == 0
    res = {"bytes": N, "patterns": P, "events_cap": EVENTS_CAP}
    tp, ep, np_, op_ = text.data_ptr(), events.data_ptr(), nev.data_ptr(), out.data_ptr()

    def check(what):
        """The all-matches list just written == the dense ids just written,
        expanded along parent[] while the length is at least MIN_LEN."""
        total = int(nev.item())
        assert total <= EVENTS_CAP, (what, total)
        ids = out.to(torch.int64) & 0xFFFFFFFF
        pos = torch.nonzero(lens[ids] >= MIN_LEN).flatten()
        cur = ids[pos]
        want = []
        while pos.numel():
            want.append((pos << 24) | cur)
            cur = parent[cur]
            keep = lens[cur] >= MIN_LEN
            pos, cur = pos[keep], cur[keep]
        want = torch.sort(torch.cat(want)).values if want else torch.zeros(0, dtype=torch.int64, device="cuda")
        got = torch.sort(events[:total]).values
        assert total == want.numel() and bool(torch.equal(got, want)), what
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
            st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
            # the states the timed flow calls start from: an earlier call over the same buffer
            ac.scan_flows_device(tp, op, nseg, N, None, st[0].data_ptr(), None, None, sp)
            torch.cuda.synchronize()
            s0, s1 = st[0].data_ptr(), st[1].data_ptr()
            ml = MIN_LEN
            calls = {
                "batch": {
                    "events": lambda: auto.scan_batch_events_device(tp, op, nseg, N, ml, ep, EVENTS_CAP, np_, sp),
                    "matches": lambda: auto.scan_batch_matches_device(tp, op, nseg, N, ml, ep, EVENTS_CAP, np_, sp),
                    "ids": lambda: auto.scan_batch_device(tp, op, nseg, N, op_, cnt.data_ptr(), sp),
                },
                "flows": {
                    "events": lambda: ac.scan_flows_events_device(tp, op, nseg, N, s0, s1, ml, ep, EVENTS_CAP, np_, sp),
                    "matches": lambda: ac.scan_flows_matches_device(tp, op, nseg, N, s0, s1, ml, ep, EVENTS_CAP, np_,
                                                                    sp),
                    "ids": lambda: ac.scan_flows_device(tp, op, nseg, N, s0, s1, op_, cnt.data_ptr(), sp),
                },
            }
            cell = {"stream_bytes": L, "streams": nseg}
            for family, c in calls.items():
                r = {}
                for name, call in (("events_a", "events"), ("matches", "matches"), ("ids", "ids"),
                                   ("events_b", "events")):
                    r[name] = stat(timed(torch, s, c[call], pre=None if call == "ids" else lambda: nev.zero_()))
                    if call != "ids":
                        total = int(nev.item())
                        assert total <= EVENTS_CAP
                        r[name]["events"] = total
                        r[name]["events_per_byte"] = round(total / N, 6)
                # the all-matches list against the dense ids of the same call
                c["ids"]()
                nev.zero_()
                c["matches"]()
                torch.cuda.synchronize()
                assert check(f"{stream} {cut} {family}") == r["matches"]["events"]
                ev = min(r["events_a"]["median_us"], r["events_b"]["median_us"])
                r["matches_over_ids"] = round(r["matches"]["median_us"] / r["ids"]["median_us"], 3)
                r["matches_over_events"] = round(r["matches"]["median_us"] / ev, 3)
                r["events_over_ids"] = round(ev / r["ids"]["median_us"], 3)
                r["events_spread"] = round(max(r["events_a"]["median_us"], r["events_b"]["median_us"]) / ev, 3)
                r["list_growth"] = round(r["matches"]["events"] / max(r["events_a"]["events"], 1), 3)
                cell[family] = r
            res[f"{stream}_{cut}"] = cell
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "host": platform.node(), "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "matches", "bench_matches.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "all-matches call vs longest-only events call (timed twice: its spread) vs dense u32 ids, min_len 3, "
                   "batched scan (auto kind) and flow scan (ac kind, state in and out per stream); 64 MiB, gen_stream "
                   "mode 0 seed 3 and the lines stream seed 3", "reps": REPS, "warmup": WARM, "min_len": MIN_LEN,
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
