#!/usr/bin/env python3
"""The ordered-rules call (pm_hip_seq_rules_by_stream_device) beside the rules
call (pm_hip_rules_by_stream_device) on the same list in the same process.

scripts/bench_rules.py's cells, lists and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream, cut into 1,500-byte and 100 KiB streams; hipEvent times of REPS
repetitions after warm-up, min and median; min_len 3, all-matches lists from
the batched scan (auto kind) and the flow scan (ac kind); its 10,000 seeded
synthetic rules of 2-4 positive terms, a fifth with one negated term more.
Per cell and list, in this order:
  rules_a  the rules call alone;
  free     (a) the ordered-rules call on the same rules with every gap free;
           its hits are asserted to be the rules call's;
  dist0    (b) the same rules with each positive term after the first made a
           following term at distance 0; on lists of at most TWIN_MAX events
           the hits are asserted to be the twin's (pm_flat_seq_rules_by_stream);
  rules_b  the rules call once more: rules_b / rules_a is the run's spread,
           beside which free_over_rules and dist0_over_rules are to be read.
No bar is fixed in advance.
(c) The per-pass times are a profiler's: one cell under a kernel trace,
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
          python scripts/bench_seq_rules.py --step snort --cell lines_1500B --reps 5
    and then --kernel-stats DIR/.../*kernel_stats.csv puts the statistics of
    the call's kernels (sq_*, the scan's three, the rules call's rl_*) into
    the JSON file as "passes".
(d) --step worst: the sort's worst case, one (stream, gid) with 2^20 distinct
    positions in shuffled order (one workgroup sorts all of them), under the
    rule gid ... gid at distance 0, beside the same events cut into ranges of
    4,096 (the LDS tier's largest), of 17 (its smallest) and of 16 (the lane
    tier's largest: no work-list entry at all).
Every step runs in a child process under its own time limit; the first one
that fails ends the run.  Writes one JSON file (--out).
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from bench_rules import CUTS, DICTS, MIN_LEN, N_DEVICE, REPS, WARM, box, stat, synthetic_rules, timed  # noqa: E402

STEP_SECONDS = 560
TWIN_MAX = 2 << 20
WORST = 1 << 20


def sorted_ranges(np, ptr, hits, nseg):
    seg = np.repeat(np.arange(nseg), np.diff(ptr))
    return hits[np.lexsort((hits, seg))]


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
    plen = [0]
    while auto.pattern_len(len(plen)) > 0:
        plen.append(auto.pattern_len(len(plen)))
    plen = np.array(plen, dtype=np.uint32)
    long_gids = np.nonzero(plen >= 3)[0]
    base = synthetic_rules(np, long_gids, 7)
    free = [[(g, None) for g in r] for r in base]
    dist0 = []
    for r in base:
        seen = False
        rule = []
        for g in r:
            rule.append((g, 0 if g > 0 and seen else None))
            seen = seen or g > 0
        dist0.append(rule)
    auto.set_rules(base)
    res = {"bytes": N, "patterns": int(lib.pm_hip_n_patterns(ac.obj)), "gids": len(plen) - 1, "rules": len(base)}
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
                rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
                rbytes, qbytes = auto.rules_scratch_bytes(cap, nseg), auto.seq_rules_scratch_bytes(cap, nseg)
                scratch = torch.empty(qbytes, dtype=torch.uint8, device="cuda")
                ep = events.data_ptr()
                nev.zero_()
                scan(ep, cap)
                torch.cuda.synchronize()
                assert int(nev.item()) == total
                r = {"events": total, "list_cap": cap, "scratch_bytes_rules": rbytes, "scratch_bytes": qbytes}

                def rules_call(hp, hcap):
                    auto.rules_by_stream_device(ep, cap, np_, op, nseg, hp, hcap, rptr.data_ptr(), scratch.data_ptr(),
                                                rbytes, sp)

                def seq_call(hp, hcap):
                    auto.seq_rules_by_stream_device(ep, cap, np_, op, nseg, hp, hcap, rptr.data_ptr(),
                                                    scratch.data_ptr(), qbytes, sp)

                def measure(call):
                    call(None, 0)  # count only: rule_ptr is exact whatever hits_cap is
                    torch.cuda.synchronize()
                    nhits = int(rptr[-1].item())
                    hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device="cuda")
                    q = stat(timed(torch, s, lambda: call(hits.data_ptr(), nhits), reps=reps))
                    ptr = rptr.cpu().numpy().copy()
                    q["hits"] = nhits
                    return q, ptr, sorted_ranges(np, ptr, hits[:nhits].cpu().numpy().view(np.uint64), nseg)
                r["rules_a"], want_ptr, want = measure(rules_call)
                auto.set_seq_rules(free)
                r["free"], ptr, hits = measure(seq_call)
                assert np.array_equal(ptr, want_ptr) and np.array_equal(hits, want), (stream, cut, family, "free")
                auto.set_seq_rules(dist0)
                r["dist0"], ptr, hits = measure(seq_call)
                if total <= TWIN_MAX:
                    lst = events[:total].cpu().numpy().view(np.uint64)
                    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, dist0, plen)
                    assert np.array_equal(ptr, exp_ptr) and np.array_equal(hits, exp_hits), (stream, cut, family, "dist0")
                    r["dist0"]["checked_against_the_twin"] = True
                r["rules_b"], _, _ = measure(rules_call)
                a, b = r["rules_a"]["median_us"], r["rules_b"]["median_us"]
                r["rules_spread"] = round(max(a, b) / min(a, b), 3)
                r["free_over_rules"] = round(r["free"]["median_us"] / min(a, b), 3)
                r["dist0_over_rules"] = round(r["dist0"]["median_us"] / min(a, b), 3)
                cell[family] = r
                print(f"{key} {stream}_{cut} {family}: {json.dumps(r)}", file=sys.stderr, flush=True)
                del events, rptr, scratch
            res[f"{stream}_{cut}"] = cell
    return res


def step_worst(reps=REPS):
    """(d): WORST events of gid 1 in one stream at distinct positions, and the
    same number spread over keys of 16 positions each."""
    import numpy as np
    import torch
    import patternmatching_amd as pm
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", "snort.dict")]))
    m.compile()
    plen = np.array([0, m.pattern_len(1)], dtype=np.uint32)
    rules = [[(1, None), (1, 0)]]
    m.set_seq_rules(rules)
    s = torch.cuda.current_stream()
    rng = np.random.default_rng(5)
    res = {"events": WORST}
    span = 4 * WORST
    cut = lambda r: np.unique(np.append(np.arange(0, span, 4 * r, dtype=np.int64), np.int64(span)))  # noqa: E731
    shapes = {"one_range": cut(WORST), "ranges_of_4096": cut(4096), "ranges_of_17": cut(17), "ranges_of_16": cut(16)}
    for name, offs in shapes.items():
        pos = rng.permutation(4 * np.arange(WORST, dtype=np.uint64))  # a position in every 4 bytes
        lst = (pos << np.uint64(24)) | np.uint64(1)
        nseg = len(offs) - 1
        events = torch.from_numpy(lst.view(np.int64)).cuda()
        nev = torch.full((1,), WORST, dtype=torch.int64, device="cuda")
        d_offs = torch.from_numpy(offs).cuda()
        rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
        nbytes = m.seq_rules_scratch_bytes(WORST, nseg)
        scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        hits = torch.zeros(nseg, dtype=torch.int64, device="cuda")

        def call():
            m.seq_rules_by_stream_device(events.data_ptr(), WORST, nev.data_ptr(), d_offs.data_ptr(), nseg,
                                         hits.data_ptr(), nseg, rptr.data_ptr(), scratch.data_ptr(), nbytes,
                                         s.cuda_stream)
        q = stat(timed(torch, s, call, reps=reps, warm=1))
        exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, rules, plen)
        ptr = rptr.cpu().numpy()
        assert np.array_equal(ptr, exp_ptr)
        assert np.array_equal(sorted_ranges(np, ptr, hits[:ptr[-1]].cpu().numpy().view(np.uint64), nseg), exp_hits)
        q.update({"streams": nseg, "hits": int(ptr[-1]), "scratch_bytes": nbytes})
        res[name] = q
        print(f"worst {name}: {json.dumps(q)}", file=sys.stderr, flush=True)
    for name in ("one_range", "ranges_of_4096", "ranges_of_17"):
        res[f"{name}_over_ranges_of_16"] = round(res[name]["median_us"] / res["ranges_of_16"]["median_us"], 2)
    return res


def kernel_stats(path):
    """The rows of a rocprofv3 kernel statistics file that belong to the two
    calls: name, calls, average and share of the traced kernel time."""
    import csv
    rows = []
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if not any(k in name for k in ("sq_", "rl_", "bs_scan")):
                continue
            short = name.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            rows.append({"kernel": short, "calls": int(row["Calls"]), "average_us": round(float(row["AverageNs"]) / 1e3, 2),
                         "total_us": round(float(row["TotalDurationNs"]) / 1e3, 1), "percent": float(row["Percentage"])})
    return sorted(rows, key=lambda r: -r["total_us"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "seqrules", "bench_seq_rules.json"))
    ap.add_argument("--dicts", default=",".join(sorted(DICTS)), help="the dictionaries to run, e.g. snort")
    ap.add_argument("--step", choices=sorted(DICTS) + ["box", "worst"], help="(internal) run one step, print its JSON")
    ap.add_argument("--cell", help="with --step: one cell only, e.g. lines_1500B (a profiler's run)")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions")
    ap.add_argument("--kernel-stats", metavar="CSV", help="add a kernel trace's statistics to --out as \"passes\"")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            doc = json.load(f)
        doc["passes"] = {"cell": "snort lines_1500B, both lists, --reps 5 (each pass once per call: the count-only "
                                 "call, 3 warm-ups and 5 repetitions of every measured set)",
                         "kernels": kernel_stats(a.kernel_stats)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return 0
    if a.step:
        r = box() if a.step == "box" else step_worst(min(a.reps, 5)) if a.step == "worst" else step_dict(a.step, a.cell,
                                                                                                       a.reps)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "ordered-rules call beside the rules call on the same all-matches list (batched scan, auto kind; flow "
                   "scan, ac kind) in the same process: the rules benchmark's 10,000 seeded rules with every gap free "
                   "(the same hits asserted) and with every positive term after the first following at distance 0; the "
                   "rules call timed before and after (its spread); worst: 2^20 events of one (stream, gid) at distinct "
                   "positions against the same events in ranges of 16; min_len 3; 64 MiB, gen_stream mode 0 seed 3 and "
                   "the lines stream seed 3",
           "reps": a.reps, "warmup": WARM, "min_len": MIN_LEN, "twin_checked_up_to_events": TWIN_MAX}
    for step, limit in [("box", 120), ("worst", 300)] + [(k, STEP_SECONDS) for k in a.dicts.split(",")]:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(a.reps)],
                               stdout=subprocess.PIPE, text=True, timeout=limit)
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
