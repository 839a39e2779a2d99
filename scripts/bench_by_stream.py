#!/usr/bin/env python3
"""The per-stream sets call (pm_hip_events_by_stream_device, plain and UNIQUE)
beside the all-matches scans whose list it groups, and beside what a caller
does with that list today on the host.

scripts/bench_groups.py's cells, inputs and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream (dense deep matches), cut into 1,500-byte and 100 KiB streams;
hipEvent times of REPS repetitions after warm-up, min and median, all of one
cell in one process; min_len 3, all-matches lists.  Per dictionary, text, cut
and family (batch: an auto object's reverse-trie walk; flows: an ac object's
dense-row walk with a state in and out per stream), in this order:
  scan_a        (a) the all-matches scan alone;
  by_stream     (b) the by-stream call alone on the list that scan left, flags 0;
  by_stream_unique  (b) the same with PM_BY_STREAM_UNIQUE;
  chained / chained_unique  (c) the scan and the by-stream call enqueued back to
                back, nothing between them, one pair of events around both;
  host          (d) the host alternative on the same list, timed on the host:
                the device-to-host copy of the events, np.sort, np.searchsorted
                of the offsets (its parts are reported too);
  scan_b        (a) once more: scan_b / scan_a is the run's spread.
The list and the by-stream output have room for 1.25x the cell's events (from
a count-only call, as pm_hip.h advises): the UNIQUE table is sized by the
list's capacity, not by its cursor.  The cursor is zeroed before every scan
(outside the timed region).  Both by-stream results of every cell are checked
against pm_flat_events_by_stream on the same list.

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
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_DEVICE = 64 << 20
CUTS = {"1500B": 1500, "100KiB": 100 << 10}
DICTS = {"snort": ["snort.dict"], "merged": ["snort.dict", "et.dict"]}
REPS, WARM = 20, 3
MIN_LEN = 3
STEP_SECONDS = 560


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


def step_dict(key, only=None, reps=REPS):
    import numpy as np
    import torch
    import patternmatching_amd as pm
    lib = pm.load()
    d = pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", f) for f in DICTS[key]])
    objs = {}
    for kind in ("ac", "auto"):
        m = pm.HipMatcher(kind)
        m.add_dictionary(d)
        m.compile()
        objs[kind] = m
    ac, auto = objs["ac"], objs["auto"]
    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = {"bytes": N, "patterns": int(lib.pm_hip_n_patterns(ac.obj))}
    tp, np_ = text.data_ptr(), nev.data_ptr()

    for stream in ("ascii", "lines"):
        if stream == "ascii":
            lib.pm_hip_gen_stream_device(tp, 0, N + 64, 3, 0, sp)
        else:
            ac.gen_lines_device(tp, N + 64, 3, sp)
        torch.cuda.synchronize()
        for cut, L in CUTS.items():
            if only and f"{stream}_{cut}" != only:
                continue
            offs = np.append(np.arange(0, N, L, dtype=np.int64), np.int64(N))
            nseg = len(offs) - 1
            d_offs = torch.from_numpy(offs).cuda()
            op = d_offs.data_ptr()
            st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
            # the states the timed flow calls start from: an earlier call over the same buffer
            ac.scan_flows_device(tp, op, nseg, N, None, st[0].data_ptr(), None, None, sp)
            torch.cuda.synchronize()
            s0, s1 = st[0].data_ptr(), st[1].data_ptr()
            cell = {"stream_bytes": L, "streams": nseg}
            for family in ("batch", "flows"):
                def scan(ep, cap, family=family):
                    if family == "batch":
                        auto.scan_batch_matches_device(tp, op, nseg, N, MIN_LEN, ep, cap, np_, sp)
                    else:
                        ac.scan_flows_matches_device(tp, op, nseg, N, s0, s1, MIN_LEN, ep, cap, np_, sp)
                nev.zero_()
                scan(None, 0)  # count only
                torch.cuda.synchronize()
                total = int(nev.item())
                cap = max(1024, total * 5 // 4)
                events = torch.zeros(cap, dtype=torch.int64, device="cuda")
                out = torch.zeros(cap, dtype=torch.int64, device="cuda")
                ptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
                sbytes = {f: auto.by_stream_scratch_bytes(cap, nseg, unique=bool(f)) for f in (0, 1)}
                scratch = torch.empty(max(sbytes.values()), dtype=torch.uint8, device="cuda")
                ep = events.data_ptr()

                def by_stream(flags):
                    auto.events_by_stream_device(ep, cap, np_, op, nseg, flags, out.data_ptr(), cap, ptr.data_ptr(),
                                                 scratch.data_ptr(), sbytes[flags], sp)
                r = {"events": total, "events_per_byte": round(total / N, 6), "list_cap": cap,
                     "scratch_bytes": sbytes[0], "scratch_bytes_unique": sbytes[1]}
                zero = lambda: nev.zero_()  # noqa: E731
                r["scan_a"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=zero, reps=reps))
                assert int(nev.item()) == total
                lst = events[:total].cpu().numpy().view(np.uint64)
                for name, flags in (("by_stream", 0), ("by_stream_unique", 1)):
                    r[name] = stat(timed(torch, s, lambda: by_stream(flags), reps=reps))
                    # against the twin on the same list
                    exp_ptr, exp_ev = pm.events_by_stream_host(lst, offs, unique=bool(flags))
                    got_ptr = ptr.cpu().numpy()
                    assert np.array_equal(got_ptr, exp_ptr), (stream, cut, family, name)
                    kept = int(got_ptr[-1])
                    body = out[:kept].cpu().numpy().view(np.uint64)
                    seg = np.repeat(np.arange(nseg), np.diff(got_ptr))
                    assert np.array_equal(body[np.lexsort((body, seg))], exp_ev), (stream, cut, family, name)
                    r[name]["kept"] = kept
                    if not flags:
                        plain_ptr = exp_ptr
                for name, flags in (("chained", 0), ("chained_unique", 1)):
                    def both(flags=flags):
                        scan(ep, cap)
                        by_stream(flags)
                    r[name] = stat(timed(torch, s, both, pre=zero, reps=reps))
                # (d) what callers do today: the list to the host, a sort, a cut per stream
                copy_s, sort_s, cut_s = [], [], []
                for _ in range(reps):
                    t0 = time.perf_counter()
                    h = events[:total].cpu().numpy().view(np.uint64)
                    t1 = time.perf_counter()
                    h = np.sort(h)
                    t2 = time.perf_counter()
                    cuts = np.searchsorted(h >> np.uint64(24), offs.astype(np.uint64))
                    t3 = time.perf_counter()
                    copy_s.append(t1 - t0), sort_s.append(t2 - t1), cut_s.append(t3 - t2)
                assert np.array_equal(cuts, plain_ptr)  # the host alternative's cut is the plain stream_ptr
                whole = [a + b + c for a, b, c in zip(copy_s, sort_s, cut_s)]
                r["host"] = stat([x * 1e6 for x in whole])
                r["host"]["copy_median_us"] = round(statistics.median(copy_s) * 1e6, 2)
                r["host"]["sort_median_us"] = round(statistics.median(sort_s) * 1e6, 2)
                r["host"]["searchsorted_median_us"] = round(statistics.median(cut_s) * 1e6, 2)
                r["scan_b"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=zero, reps=reps))
                a = min(r["scan_a"]["median_us"], r["scan_b"]["median_us"])
                r["scan_spread"] = round(max(r["scan_a"]["median_us"], r["scan_b"]["median_us"]) / a, 3)
                for name in ("by_stream", "by_stream_unique"):
                    r[f"{name}_over_scan"] = round(r[name]["median_us"] / a, 3)
                    r[f"{name}_over_host"] = round(r[name]["median_us"] / r["host"]["median_us"], 5)
                r["chained_over_sum"] = round(r["chained"]["median_us"] / (a + r["by_stream"]["median_us"]), 3)
                r["chained_unique_over_sum"] = round(
                    r["chained_unique"]["median_us"] / (a + r["by_stream_unique"]["median_us"]), 3)
                r["unique_list_ratio"] = round(r["by_stream_unique"]["kept"] / max(total, 1), 4)
                cell[family] = r
                print(f"{key} {stream}_{cut} {family}: {json.dumps(r)}", file=sys.stderr, flush=True)
                del events, out, ptr, scratch
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "bystream", "bench_by_stream.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    ap.add_argument("--cell", help="with --step: one cell only, e.g. lines_100KiB (a profiler's run)")
    ap.add_argument("--reps", type=int, default=REPS, help="with --step: timed repetitions")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step, a.cell, a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "per-stream sets call (plain and UNIQUE) on the all-matches list of the batched scan (auto kind) and "
                   "the flow scan (ac kind, state in and out per stream), alone, chained behind the scan, and beside "
                   "the host alternative (device-to-host copy + np.sort + np.searchsorted); the scan timed before and "
                   "after (its spread); min_len 3; 64 MiB, gen_stream mode 0 seed 3 and the lines stream seed 3",
           "reps": REPS, "warmup": WARM, "min_len": MIN_LEN, "library": os.environ.get("PM_LIBPM") or "in-tree"}
    for step, limit in [("box", 120)] + [(k, STEP_SECONDS) for k in DICTS]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], stdout=subprocess.PIPE,
                               text=True, timeout=limit)  # (the step's progress lines go to stderr as they come)
        except subprocess.TimeoutExpired:
            print(f"{step}: no result within {limit} s; stopping", file=sys.stderr)
            return 1
        line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
        if p.returncode != 0 or not line:
            print(f"{step}: exit {p.returncode}; stopping", file=sys.stderr)
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
