#!/usr/bin/env python3
"""The rules call (pm_hip_rules_by_stream_device) beside the all-matches scan
whose list it reads, beside the PM_BY_STREAM_UNIQUE call on the same list
(which pays the same hash insert), and beside what a caller does without it:
the UNIQUE sets copied to the host and the twin pm_flat_rules_by_stream run
on them on one thread.

scripts/bench_by_stream.py's cells, inputs and timing: device-resident, snort
and merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2)
the lines stream (dense deep matches), cut into 1,500-byte and 100 KiB
streams; hipEvent times of REPS repetitions after warm-up, min and median, all
of one cell in one process; min_len 3, all-matches lists from the batched scan
(an auto object's reverse-trie walk) and the flow scan (an ac object's
dense-row walk with a state in and out per stream).

The dictionaries carry no rules, so the rules are synthetic and seeded:
  rules    10,000 rules of 2-4 positive terms drawn from the patterns of at
           least 3 bytes, a fifth of them with one negated term more;
  stress   the same, and 5,000 rules more that all carry the cell's most
           frequent pattern as their PM_RULE_FAST anchor beside one other term.
Per cell, in this order:
  scan_a   (a) the all-matches scan alone;
  unique   (b) the PM_BY_STREAM_UNIQUE call alone on the list that scan left;
  rules / stress   the rules call alone on that list, per rule set;
  host     (c) per rule set, timed on the host: the UNIQUE sets and stream_ptr
           copied to the host, then pm_flat_rules_by_stream on them (its parts
           are reported too); its hits are the expected value of the device's;
  scan_b   (a) once more: scan_b / scan_a is the run's spread.
The hits array has exactly the rule set's hits (from a first call with
hits_cap 0, as pm_hip.h advises).  Every step runs in a child process under
its own time limit; the first one that fails ends the run.  Writes one JSON
file (--out).
"""
import argparse
import ctypes
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
REPS, WARM, HOST_REPS = 20, 3, 2
MIN_LEN = 3
NRULES, NSTRESS = 10000, 5000
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


def synthetic_rules(np, long_gids, seed):
    """NRULES seeded rules: 2-4 distinct positive terms, every fifth one negated term more."""
    rng = np.random.default_rng(seed)
    rules = []
    for r in range(NRULES):
        k = int(rng.integers(2, 5))
        while True:
            pick = long_gids[rng.integers(0, len(long_gids), size=k + 1)].tolist()
            if len(set(pick)) == k + 1:
                break
        rules.append(pick[:k] + ([-pick[k]] if r % 5 == 0 else []))
    return rules


def step_dict(key, only=None, reps=REPS):
    import numpy as np
    import torch
    import patternmatching_amd as pm
    lib = pm.load()
    u32p = ctypes.POINTER(ctypes.c_uint32)
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
    plen = [0]
    while auto.pattern_len(len(plen)) > 0:
        plen.append(auto.pattern_len(len(plen)))
    plen = np.array(plen, dtype=np.uint32)
    long_gids = np.nonzero(plen >= 3)[0]
    base_rules = synthetic_rules(np, long_gids, 7)
    res = {"bytes": N, "patterns": int(lib.pm_hip_n_patterns(ac.obj)), "gids": len(plen) - 1,
           "gids_of_3_bytes_or_more": len(long_gids)}
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
                rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
                ubytes = auto.by_stream_scratch_bytes(cap, nseg, unique=True)
                rbytes = auto.rules_scratch_bytes(cap, nseg)
                scratch = torch.empty(max(ubytes, rbytes), dtype=torch.uint8, device="cuda")
                ep = events.data_ptr()
                r = {"events": total, "events_per_byte": round(total / N, 6), "list_cap": cap,
                     "scratch_bytes": rbytes, "scratch_bytes_unique": ubytes}
                zero = lambda: nev.zero_()  # noqa: E731
                r["scan_a"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=zero, reps=reps))
                assert int(nev.item()) == total

                def unique():
                    auto.events_by_stream_device(ep, cap, np_, op, nseg, 1, out.data_ptr(), cap, ptr.data_ptr(),
                                                 scratch.data_ptr(), ubytes, sp)
                r["unique"] = stat(timed(torch, s, unique, reps=reps))
                kept = int(ptr[-1].item())
                r["unique"]["kept"] = kept
                sets = out[:kept].cpu().numpy().view(np.uint64)
                gid_count = np.bincount((sets & np.uint64(0xFFFFFF)).astype(np.int64), minlength=len(plen))
                top = int(np.argmax(np.where(plen >= 3, gid_count[:len(plen)], -1)))
                rng = np.random.default_rng(11)
                others = rng.choice(long_gids[long_gids != top], size=NSTRESS, replace=True).tolist()
                sets_of = {"rules": (base_rules, None),
                           "stress": (base_rules + [[top, int(g)] for g in others], [None] * NRULES + [top] * NSTRESS)}
                for name, (rules, fast) in sets_of.items():
                    auto.set_rules(rules, fast)
                    assert auto.rules_min_len() >= MIN_LEN
                    tptr, terms = pm.pack_rules(rules, fast)

                    def call(hp, hcap):
                        auto.rules_by_stream_device(ep, cap, np_, op, nseg, hp, hcap, rptr.data_ptr(), scratch.data_ptr(),
                                                    rbytes, sp)
                    call(None, 0)  # count only: rule_ptr is exact whatever hits_cap is
                    torch.cuda.synchronize()
                    nhits = int(rptr[-1].item())
                    hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device="cuda")
                    q = stat(timed(torch, s, lambda: call(hits.data_ptr(), nhits), reps=reps))
                    # (c) what a caller does without the call: the sets to the host, the twin on one thread
                    copy_s, twin_s = [], []
                    for _ in range(HOST_REPS):
                        t0 = time.perf_counter()
                        h = out[:kept].cpu().numpy().view(np.uint64)
                        hp = ptr.cpu().numpy()
                        t1 = time.perf_counter()
                        exp_ptr, exp_hits = pm.rules_by_stream_host(h, offs, (tptr, terms), hits_cap=nhits)
                        t2 = time.perf_counter()
                        copy_s.append(t1 - t0), twin_s.append(t2 - t1)
                    assert hp[-1] == kept
                    # the device's hits against the twin's (the sets give what the whole list gives)
                    got_ptr = rptr.cpu().numpy()
                    assert np.array_equal(got_ptr, exp_ptr), (stream, cut, family, name)
                    body = hits[:nhits].cpu().numpy().view(np.uint64)
                    seg = np.repeat(np.arange(nseg), np.diff(got_ptr))
                    assert np.array_equal(body[np.lexsort((body, seg))], exp_hits), (stream, cut, family, name)
                    # the slots that anchor something: the (stream, gid) pairs whose gid anchors a rule
                    aptr = np.zeros(len(plen) + 1, np.uint32)
                    arules, aterm = np.zeros(len(rules), np.uint32), np.zeros(len(rules), np.uint32)
                    assert lib.pm_flat_rule_tables(tptr.ctypes.data_as(u32p), terms.ctypes.data_as(u32p), len(rules),
                                                   plen.ctypes.data_as(u32p), len(plen) - 1, aptr.ctypes.data_as(u32p),
                                                   arules.ctypes.data_as(u32p), aterm.ctypes.data_as(u32p)) == 0
                    per_gid = np.diff(aptr)[:len(plen)].astype(np.int64)
                    q.update({"rules": len(rules), "hits": nhits, "hits_per_stream": round(nhits / nseg, 4),
                              "anchoring_slots": int(np.sum(gid_count[:len(plen)][per_gid > 0])),
                              "rules_verified": int(np.sum(gid_count[:len(plen)] * per_gid)),
                              "table_slots": 1 << (2 * cap - 1).bit_length()})
                    whole = [a + b for a, b in zip(copy_s, twin_s)]
                    q["host"] = stat([x * 1e6 for x in whole])
                    q["host"]["copy_median_us"] = round(statistics.median(copy_s) * 1e6, 2)
                    q["host"]["twin_median_us"] = round(statistics.median(twin_s) * 1e6, 2)
                    r[name] = q
                    del hits
                r["scan_b"] = stat(timed(torch, s, lambda: scan(ep, cap), pre=zero, reps=reps))
                a = min(r["scan_a"]["median_us"], r["scan_b"]["median_us"])
                r["scan_spread"] = round(max(r["scan_a"]["median_us"], r["scan_b"]["median_us"]) / a, 3)
                for name in sets_of:
                    r[f"{name}_over_scan"] = round(r[name]["median_us"] / a, 3)
                    r[f"{name}_over_unique"] = round(r[name]["median_us"] / r["unique"]["median_us"], 3)
                    r[f"{name}_over_host"] = round(r[name]["median_us"] / r[name]["host"]["median_us"], 5)
                cell[family] = r
                print(f"{key} {stream}_{cut} {family}: {json.dumps(r)}", file=sys.stderr, flush=True)
                del events, out, ptr, rptr, scratch
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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "rules", "bench_rules.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    ap.add_argument("--cell", help="with --step: one cell only, e.g. lines_100KiB (a profiler's run)")
    ap.add_argument("--reps", type=int, default=REPS, help="with --step: timed repetitions")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step, a.cell, a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "rules call on the all-matches list of the batched scan (auto kind) and the flow scan (ac kind, state "
                   "in and out per stream), alone, beside the scan, the PM_BY_STREAM_UNIQUE call on the same list and "
                   "the host alternative (UNIQUE sets copied to the host + pm_flat_rules_by_stream on one thread); the "
                   "scan timed before and after (its spread); 10,000 seeded synthetic rules of 2-4 positive terms from "
                   "the patterns of >= 3 bytes, a fifth with one negated term; stress: 5,000 rules more anchored "
                   "(PM_RULE_FAST) at the list's most frequent pattern; min_len 3; 64 MiB, gen_stream mode 0 seed 3 and "
                   "the lines stream seed 3",
           "reps": REPS, "warmup": WARM, "host_reps": HOST_REPS, "min_len": MIN_LEN,
           "library": os.environ.get("PM_LIBPM") or "in-tree"}
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
