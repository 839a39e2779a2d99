#!/usr/bin/env python3
"""The flow ordered-rules call (pm_hip_flow_seq_rules_device) beside the flow
scan whose list it reads, beside its two siblings on a like list in the same
process, and beside what a caller did without it: the list copied to the host
and the twin pm_flat_flow_seq_rules run on it, on one thread, over rows kept on
the host.

scripts/bench_flow_rules.py's cells and timing: device-resident, the snort
dictionary, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the lines
stream, cut into 1,500-byte packets, one packet per flow and call; hipEvent
times of REPS repetitions after warm-up, min, median and max; min_len 3,
all-matches lists from the flow scan of an ac object with a state in and out
per flow.  Two calls: packet 1 of every flow (seed 3), then packet 2 (seed 4)
continuing it.  The rules are --rules seeded synthetic ordered ones: 2 to 4
positive terms, the second following the first at distance 0 (one chain word
per rule), the others free, every fifth with one negated term more.  A row
has --rules chain words and the bits behind them; the default keeps the rows
of 44,740 flows below 400 MB.
Per call, in this order:
  scan     the flow scan alone;
  keep     the call alone under PM_FLOW_RULES_KEEP (the same work every
           repetition: the rows are not changed);
  commit   one committing call (timed once: it changes the rows);
  seq      the ordered-rules call (pm_hip_seq_rules_by_stream_device) with the
           same rules on the same list: no flows, the packet alone;
  flow     the flow-rules call (pm_hip_flow_rules_device, KEEP) with the same
           rules' terms, unordered, on the same list and the sets as the first
           call's commit left them;
  host     the list copied to the host, then pm_flat_flow_seq_rules on it;
           its hits and rows are the expected values of the device's.
--kernel-stats CSV adds the per-pass times of a rocprofv3 kernel trace, taken
in a run of its own, to --out.  Writes one JSON file (--out).
"""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rules import MIN_LEN, N_DEVICE, REPS, box, timed  # noqa: E402

PACKET = 1500


def stat(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2), "max_us": round(max(us), 2),
            "spread": round(max(us) / min(us), 3)}


def synthetic_seq_rules(np, long_gids, seed, nrules):
    rng = np.random.default_rng(seed)
    rules = []
    for r in range(nrules):
        k = int(rng.integers(2, 5))
        while True:
            pick = long_gids[rng.integers(0, len(long_gids), size=k + 1)].tolist()
            if len(set(pick)) == k + 1:
                break
        rule = [(pick[0], None), (pick[1], 0)] + [(g, None) for g in pick[2:k]]
        rules.append(rule + ([(-pick[k], None)] if r % 5 == 0 else []))
    return rules


def run(reps, nrules, only=None):
    import numpy as np
    import torch
    import patternmatching_amd as pm
    lib = pm.load()
    u32p, u64p, i64p = (ctypes.POINTER(t) for t in (ctypes.c_uint32, ctypes.c_uint64, ctypes.c_int64))
    d = pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", "snort.dict")])
    ac = pm.HipMatcher("ac")
    ac.add_dictionary(d)
    ac.compile()
    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    plen = [0]
    while ac.pattern_len(len(plen)) > 0:
        plen.append(ac.pattern_len(len(plen)))
    plen = np.array(plen, dtype=np.uint32)
    rules = synthetic_seq_rules(np, np.nonzero(plen >= 3)[0], 7, nrules)
    ac.set_flow_seq_rules(rules)
    ac.set_seq_rules(rules)
    ac.set_flow_rules([[g for g, _ in r] for r in rules])
    assert ac.flow_seq_rules_min_len() >= MIN_LEN
    S, W = ac.flow_seq_rule_words, ac.flow_rule_words
    tptr, terms, gaps = pm.pack_seq_rules(rules)
    offs = np.append(np.arange(0, N, PACKET, dtype=np.int64), np.int64(N))
    nseg = len(offs) - 1
    lens = np.diff(offs).astype(np.uint64)
    d_offs = torch.from_numpy(offs).cuda()
    op = d_offs.data_ptr()
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    tp, np_ = text.data_ptr(), nev.data_ptr()
    res = {"bytes": N, "flows": nseg, "packet_bytes": PACKET, "rules": len(rules), "row_words": S,
           "chain_words": ac.flow_seq_chain_count(), "row_bytes": 8 * S, "rows_bytes": 8 * S * nseg,
           "flow_rules_set_words": W}
    for stream in ("ascii", "lines"):
        if only and stream != only:
            continue
        d_prog = torch.zeros(nseg * S, dtype=torch.int64, device="cuda")
        d_sets = torch.zeros(nseg * W, dtype=torch.int64, device="cuda")
        h_prog = np.zeros((nseg, S), dtype=np.uint64)
        st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
        cell = {}
        for call, seed in enumerate((3, 4)):
            if stream == "ascii":
                lib.pm_hip_gen_stream_device(tp, 0, N + 64, seed, 0, sp)
            else:
                ac.gen_lines_device(tp, N + 64, seed, sp)
            torch.cuda.synchronize()
            s_in = None if call == 0 else st[0].data_ptr()
            s_out = st[call].data_ptr()
            pos_in = np.zeros(nseg, dtype=np.uint64) if call == 0 else lens
            d_pos = torch.from_numpy(pos_in.view(np.int64).copy()).cuda()

            def scan(ep, cap):
                ac.scan_flows_matches_device(tp, op, nseg, N, s_in, s_out, MIN_LEN, ep, cap, np_, sp)
            nev.zero_()
            scan(None, 0)  # count only
            torch.cuda.synchronize()
            total = int(nev.item())
            cap = max(1024, total * 5 // 4)
            events = torch.zeros(cap, dtype=torch.int64, device="cuda")
            rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
            sbytes = ac.flow_seq_rules_scratch_bytes(cap, nseg)
            scratch = torch.empty(max(sbytes, ac.flow_rules_scratch_bytes(cap, nseg)), dtype=torch.uint8, device="cuda")
            ep = events.data_ptr()
            r = {"events": total, "list_cap": cap, "scratch_bytes": sbytes}
            r["scan"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=lambda: nev.zero_(), reps=reps))
            assert int(nev.item()) == total

            def call_fs(flags, hp, hcap):
                ac.flow_seq_rules_device(ep, cap, np_, op, nseg, d_prog.data_ptr(), nseg, None, d_pos.data_ptr(), flags,
                                         hp, hcap, rptr.data_ptr(), scratch.data_ptr(), sbytes, sp)

            def call_seq(hp, hcap):
                ac.seq_rules_by_stream_device(ep, cap, np_, op, nseg, hp, hcap, rptr.data_ptr(), scratch.data_ptr(),
                                              sbytes, sp)

            def call_flow(flags, hp, hcap):
                ac.flow_rules_device(ep, cap, np_, op, nseg, d_sets.data_ptr(), nseg, None, flags, hp, hcap,
                                     rptr.data_ptr(), scratch.data_ptr(), len(scratch), sp)
            # the siblings first, on the same list: each sized by a count-only call of its own
            call_seq(None, 0)
            torch.cuda.synchronize()
            n_seq = int(rptr[-1].item())
            hits = torch.zeros(max(n_seq, 1), dtype=torch.int64, device="cuda")
            r["seq"] = stat(timed(torch, s, lambda: call_seq(hits.data_ptr(), n_seq), reps=reps))
            call_flow(pm.FLOW_RULES_KEEP, None, 0)
            torch.cuda.synchronize()
            n_flow = int(rptr[-1].item())
            hits = torch.zeros(max(n_flow, 1), dtype=torch.int64, device="cuda")
            r["flow"] = stat(timed(torch, s, lambda: call_flow(pm.FLOW_RULES_KEEP, hits.data_ptr(), n_flow), reps=reps))
            call_flow(0, hits.data_ptr(), n_flow)  # its sets go on to the next call
            call_fs(pm.FLOW_RULES_KEEP, None, 0)  # count only
            torch.cuda.synchronize()
            nhits = int(rptr[-1].item())
            hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device="cuda")
            r["keep"] = stat(timed(torch, s, lambda: call_fs(pm.FLOW_RULES_KEEP, hits.data_ptr(), nhits), reps=reps))
            r["commit"] = stat(timed(torch, s, lambda: call_fs(0, hits.data_ptr(), nhits), reps=1, warm=0))
            got_ptr = rptr.cpu().numpy()
            body = hits[:nhits].cpu().numpy().view(np.uint64)
            # the host alternative: the list to the host, the twin over host rows
            t0 = time.perf_counter()
            h = events[:total].cpu().numpy().view(np.uint64)
            t1 = time.perf_counter()
            exp_ptr, exp_hits = np.zeros(nseg + 1, np.int64), np.zeros(max(nhits, 1), np.uint64)
            rc = lib.pm_flat_flow_seq_rules(h.ctypes.data_as(u64p), len(h), offs.ctypes.data_as(i64p), nseg,
                                            tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p),
                                            gaps.ctypes.data_as(u32p), len(rules), plen.ctypes.data_as(u32p),
                                            len(plen) - 1, h_prog.ctypes.data_as(u64p), nseg, S, None,
                                            pos_in.ctypes.data_as(u64p), 0, exp_hits.ctypes.data_as(u64p), nhits,
                                            exp_ptr.ctypes.data_as(i64p))  # one call: the device gave the hits' number
            t2 = time.perf_counter()
            assert rc == 0
            exp_hits = exp_hits[:nhits]
            assert np.array_equal(got_ptr, exp_ptr), (stream, call)
            seg = np.repeat(np.arange(nseg), np.diff(got_ptr))
            assert np.array_equal(body[np.lexsort((body, seg))], exp_hits), (stream, call)
            assert np.array_equal(d_prog.cpu().numpy().view(np.uint64).reshape(nseg, S), h_prog), (stream, call)
            keep = r["keep"]["median_us"]
            r.update({"hits": nhits, "seq_hits": n_seq, "flow_hits": n_flow,
                      "host_copy_us": round((t1 - t0) * 1e6, 1), "host_twin_us": round((t2 - t1) * 1e6, 1),
                      "keep_over_scan": round(keep / r["scan"]["median_us"], 3),
                      "keep_over_seq": round(keep / r["seq"]["median_us"], 3),
                      "keep_over_flow": round(keep / r["flow"]["median_us"], 3),
                      "keep_over_host": round(keep / ((t2 - t0) * 1e6), 5),
                      "nonzero_row_words": int(np.count_nonzero(h_prog))})
            cell[f"call{call + 1}"] = r
            print(f"{stream} call {call + 1}: {json.dumps(r)}", file=sys.stderr, flush=True)
            del events, rptr, scratch, hits
        res[stream] = cell
    return res


def kernel_stats(path):
    """The rows of a rocprofv3 kernel statistics file that belong to the
    calls: name, calls, average and share of the traced kernel time."""
    import csv
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if not any(k in name for k in ("fs_", "sq_", "fr_", "bs_scan")):
                continue
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.append({"kernel": short, "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                         "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1), "percent": float(row["Percentage"])})
    return sorted(rows, key=lambda r: -r["total_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flowseqrules", "bench_flow_seq_rules.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rules", type=int, default=1000)
    ap.add_argument("--only", choices=["ascii", "lines"], help="one stream only (a profiler's run)")
    ap.add_argument("--no-out", action="store_true", help="print only (a profiler's run)")
    ap.add_argument("--kernel-stats", metavar="CSV", help="add a kernel trace's statistics to --out as \"passes\"")
    ap.add_argument("--kernel-stats-what", default="", help="the traced run, in words")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            doc = json.load(f)
        doc["passes"] = {"run": a.kernel_stats_what, "kernels": kernel_stats(a.kernel_stats)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return 0
    res = run(a.reps, a.rules, a.only)
    if a.no_out:
        print(json.dumps(res))
        return 0
    doc = {"what": "flow ordered-rules call behind the flow scan (ac kind), two calls of one 1,500-byte packet per flow, "
                   "beside the scan, the ordered-rules call and the flow-rules call on the same list, and the host "
                   "alternative (the list copied to the host + pm_flat_flow_seq_rules on one thread); seeded synthetic "
                   "ordered rules of 2-4 positive terms, the second following the first at distance 0, a fifth with "
                   "one negated term; min_len 3; 64 MiB",
           "reps": a.reps, "default_reps": REPS, "box": box(), "snort": res}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["snort"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
