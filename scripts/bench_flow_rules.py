#!/usr/bin/env python3
"""The flow-rules call (pm_hip_flow_rules_device) beside the flow scan whose
list it reads, and beside what a caller did without it: the list's
PM_BY_STREAM_UNIQUE sets copied to the host and the twin pm_flat_flow_rules run
on them, on one thread, over sets kept on the host.

scripts/bench_rules.py's inputs and timing: device-resident, the snort
dictionary, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the lines
stream, cut into 1,500-byte packets, one packet per flow and call; hipEvent
times of REPS repetitions after warm-up, min and median; min_len 3,
all-matches lists from the flow scan of an ac object with a state in and out
per flow.  Two calls: packet 1 of every flow (seed 3), then packet 2 (seed 4)
continuing it.  The rules are bench_rules.py's 10,000 seeded synthetic ones.
Per call, in this order:
  scan     the flow scan alone;
  keep     the flow-rules call alone under PM_FLOW_RULES_KEEP (the same work
           every repetition: the sets are not changed);
  commit   one committing call (timed once: it changes the sets);
  host     the UNIQUE sets of the list copied to the host, then
           pm_flat_flow_rules on them; its hits and sets are the expected
           values of the device's.
Writes one JSON file (--out).
"""
import argparse
import ctypes
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_rules import MIN_LEN, N_DEVICE, REPS, box, stat, synthetic_rules, timed  # noqa: E402

PACKET = 1500


def run(reps):
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
    rules = synthetic_rules(np, np.nonzero(plen >= 3)[0], 7)
    ac.set_flow_rules(rules)
    assert ac.flow_rules_min_len() >= MIN_LEN
    W = ac.flow_rule_words
    tptr, terms = pm.pack_rules(rules)
    offs = np.append(np.arange(0, N, PACKET, dtype=np.int64), np.int64(N))
    nseg = len(offs) - 1
    d_offs = torch.from_numpy(offs).cuda()
    op = d_offs.data_ptr()
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    tp, np_ = text.data_ptr(), nev.data_ptr()
    res = {"bytes": N, "flows": nseg, "packet_bytes": PACKET, "rules": len(rules), "set_words": W,
           "term_gids": int(np.count_nonzero(pm.flow_rule_bits_host((tptr, terms), len(plen) - 1)[0] != 0xFFFFFFFF))}
    for stream in ("ascii", "lines"):
        d_sets = torch.zeros(nseg * W, dtype=torch.int64, device="cuda")
        h_sets = np.zeros((nseg, W), dtype=np.uint64)
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

            def scan(ep, cap):
                ac.scan_flows_matches_device(tp, op, nseg, N, s_in, s_out, MIN_LEN, ep, cap, np_, sp)
            nev.zero_()
            scan(None, 0)  # count only
            torch.cuda.synchronize()
            total = int(nev.item())
            cap = max(1024, total * 5 // 4)
            events = torch.zeros(cap, dtype=torch.int64, device="cuda")
            out = torch.zeros(cap, dtype=torch.int64, device="cuda")
            ptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
            rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
            ubytes = ac.by_stream_scratch_bytes(cap, nseg, unique=True)
            rbytes = ac.flow_rules_scratch_bytes(cap, nseg)
            scratch = torch.empty(max(ubytes, rbytes), dtype=torch.uint8, device="cuda")
            ep = events.data_ptr()
            r = {"events": total, "list_cap": cap, "scratch_bytes": rbytes}
            r["scan"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=lambda: nev.zero_(), reps=reps))
            assert int(nev.item()) == total

            def rules_call(flags, hp, hcap):
                ac.flow_rules_device(ep, cap, np_, op, nseg, d_sets.data_ptr(), nseg, None, flags, hp, hcap,
                                     rptr.data_ptr(), scratch.data_ptr(), rbytes, sp)
            rules_call(pm.FLOW_RULES_KEEP, None, 0)  # count only
            torch.cuda.synchronize()
            nhits = int(rptr[-1].item())
            hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device="cuda")
            r["keep"] = stat(timed(torch, s, lambda: rules_call(pm.FLOW_RULES_KEEP, hits.data_ptr(), nhits), reps=reps))
            r["commit"] = stat(timed(torch, s, lambda: rules_call(0, hits.data_ptr(), nhits), reps=1, warm=0))
            got_ptr = rptr.cpu().numpy()
            body = hits[:nhits].cpu().numpy().view(np.uint64)
            # the host alternative: the UNIQUE sets to the host, the twin over host sets
            ac.events_by_stream_device(ep, cap, np_, op, nseg, 1, out.data_ptr(), cap, ptr.data_ptr(), scratch.data_ptr(),
                                       ubytes, sp)
            torch.cuda.synchronize()
            kept = int(ptr[-1].item())
            t0 = time.perf_counter()
            h = out[:kept].cpu().numpy().view(np.uint64)
            t1 = time.perf_counter()
            exp_ptr, exp_hits = np.zeros(nseg + 1, np.int64), np.zeros(max(nhits, 1), np.uint64)
            rc = lib.pm_flat_flow_rules(h.ctypes.data_as(u64p), len(h), offs.ctypes.data_as(i64p), nseg,
                                        tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(rules),
                                        h_sets.ctypes.data_as(u64p), nseg, W, None, 0, exp_hits.ctypes.data_as(u64p), nhits,
                                        exp_ptr.ctypes.data_as(i64p))  # one call: the device gave the hits' number
            t2 = time.perf_counter()
            assert rc == 0
            exp_hits = exp_hits[:nhits]
            assert np.array_equal(got_ptr, exp_ptr), (stream, call)
            seg = np.repeat(np.arange(nseg), np.diff(got_ptr))
            assert np.array_equal(body[np.lexsort((body, seg))], exp_hits), (stream, call)
            assert np.array_equal(d_sets.cpu().numpy().view(np.uint64).reshape(nseg, W), h_sets), (stream, call)
            r.update({"hits": nhits, "unique_kept": kept, "host_copy_us": round((t1 - t0) * 1e6, 1),
                      "host_twin_us": round((t2 - t1) * 1e6, 1),
                      "keep_over_scan": round(r["keep"]["median_us"] / r["scan"]["median_us"], 3),
                      "keep_over_host": round(r["keep"]["median_us"] / ((t2 - t0) * 1e6), 5),
                      "nonzero_set_words": int(np.count_nonzero(h_sets))})
            cell[f"call{call + 1}"] = r
            print(f"{stream} call {call + 1}: {json.dumps(r)}", file=sys.stderr, flush=True)
            del events, out, ptr, rptr, scratch, hits
        res[stream] = cell
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flowrules", "bench_flow_rules.json"))
    ap.add_argument("--reps", type=int, default=REPS)
    a = ap.parse_args()
    doc = {"what": "flow-rules call behind the flow scan (ac kind), two calls of one 1,500-byte packet per flow, beside "
                   "the scan and the host alternative (UNIQUE sets copied to the host + pm_flat_flow_rules); 10,000 "
                   "seeded synthetic rules of 2-4 positive terms, a fifth with one negated term; min_len 3; 64 MiB",
           "reps": a.reps, "box": box(), "snort": run(a.reps)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc["snort"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
