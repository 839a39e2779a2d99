#!/usr/bin/env python3
"""Within (an upper bound on an ordered rule's link) beside distance-only
ordered rules, on scripts/bench_seq_rules.py's cells, lists and 10,000 rules.

  unbounded  a set without any bound runs sq_eval_kernel as before.  With
             --parent-lib PATH (a libpm.so built from the parent commit) the
             dist0 set is timed in child processes that load this tree's
             library and the parent's in turn, PARENT_RUNS times each: the
             parent's own run-to-run spread, and this tree's median over the
             parent's.  A ratio outside the spread is a regression.
  bounded    per cell and list, in one process: dist0 (every positive term
             after the first following at distance 0), then the same with
             every such term bounded at d + L + 64 (sq_eval_within_kernel);
             the whole call's time, and on lists of at most TWIN_MAX events the
             hits asserted to be the twin's.  The eval pass alone is a
             profiler's figure: one cell under a kernel trace,
               rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- \
                   python scripts/bench_within_rules.py --step bounded --cell lines_1500B --reps 5
             and then --kernel-stats DIR/.../*kernel_stats.csv puts the
             statistics of the call's kernels into the JSON file as "passes".
  worst      one lane, two ranges: in one stream of 100 KiB, N A's and N B's
             interleaved so that every candidate fails by one byte but the
             last; the rule A, then B within L + 1 has one anchoring slot, so
             one lane walks both ranges serially, one gallop step of one
             position per turn.
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
from bench_seq_rules import TWIN_MAX, kernel_stats, sorted_ranges  # noqa: E402

STEP_SECONDS = 560
PARENT_RUNS = 3
SLACK = 64
WORST_BYTES = 100 << 10


def rule_sets(np, plen):
    base = synthetic_rules(np, np.nonzero(plen >= 3)[0], 7)
    dist0, bounded = [], []
    for r in base:
        seen = False
        a, b = [], []
        for g in r:
            follows = g > 0 and seen
            a.append((g, 0 if follows else None))
            b.append((g, 0, int(plen[g]) + SLACK) if follows else (g, None))
            seen = seen or g > 0
        dist0.append(a)
        bounded.append(b)
    return dist0, bounded


def step_cells(key, only=None, reps=REPS, unbounded_only=False):
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
    dist0, bounded = rule_sets(np, plen)
    res = {"bytes": N, "gids": len(plen) - 1, "rules": len(dist0), "library": os.path.relpath(pm.LIB_PATH, REPO)}
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
            nev.zero_()
            auto.scan_batch_matches_device(tp, op, nseg, N, MIN_LEN, None, 0, np_, sp)  # count only
            torch.cuda.synchronize()
            total = int(nev.item())
            cap = max(1024, total * 5 // 4)
            events = torch.zeros(cap, dtype=torch.int64, device="cuda")
            rptr = torch.zeros(nseg + 1, dtype=torch.int64, device="cuda")
            qbytes = auto.seq_rules_scratch_bytes(cap, nseg)
            scratch = torch.empty(qbytes, dtype=torch.uint8, device="cuda")
            ep = events.data_ptr()
            nev.zero_()
            auto.scan_batch_matches_device(tp, op, nseg, N, MIN_LEN, ep, cap, np_, sp)
            torch.cuda.synchronize()
            r = {"stream_bytes": L, "streams": nseg, "events": total}

            def call(hp, hcap):
                auto.seq_rules_by_stream_device(ep, cap, np_, op, nseg, hp, hcap, rptr.data_ptr(), scratch.data_ptr(),
                                                qbytes, sp)

            def measure(rules):
                auto.set_seq_rules(rules)
                call(None, 0)  # count only: rule_ptr is exact whatever hits_cap is
                torch.cuda.synchronize()
                nhits = int(rptr[-1].item())
                hits = torch.zeros(max(nhits, 1), dtype=torch.int64, device="cuda")
                q = stat(timed(torch, s, lambda: call(hits.data_ptr(), nhits), reps=reps))
                ptr = rptr.cpu().numpy().copy()
                q["hits"] = nhits
                if total <= TWIN_MAX and not unbounded_only:
                    lst = events[:total].cpu().numpy().view(np.uint64)
                    exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, rules, plen)
                    got = sorted_ranges(np, ptr, hits[:nhits].cpu().numpy().view(np.uint64), nseg)
                    assert np.array_equal(ptr, exp_ptr) and np.array_equal(got, exp_hits), (stream, cut)
                    q["checked_against_the_twin"] = True
                return q
            r["dist0"] = measure(dist0)
            if not unbounded_only:
                r["bounded"] = measure(bounded)
                r["within_run"] = auto.seq_rules_within_run()
                r["dist0_again"] = measure(dist0)
                a, b = r["dist0"]["median_us"], r["dist0_again"]["median_us"]
                r["dist0_spread"] = round(max(a, b) / min(a, b), 3)
                r["bounded_over_dist0"] = round(r["bounded"]["median_us"] / min(a, b), 3)
            res[f"{stream}_{cut}"] = r
            print(f"{key} {stream}_{cut}: {json.dumps(r)}", file=sys.stderr, flush=True)
            del events, rptr, scratch
    return res


def step_worst(reps=REPS):
    import numpy as np
    import torch
    import patternmatching_amd as pm
    m = pm.HipMatcher("auto")
    m.add_dictionary(pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", "snort.dict")]))
    m.compile()
    plen = np.array([0, m.pattern_len(1), m.pattern_len(2)], dtype=np.uint32)
    L = int(plen[2])
    n = WORST_BYTES // 4 - 8
    a = 8 + 4 * np.arange(n, dtype=np.uint64)
    b = a + np.uint64(L - 1)
    b[-1] = a[-1] + np.uint64(L)
    rng = np.random.default_rng(5)
    lst = rng.permutation(np.concatenate([(a << np.uint64(24)) | np.uint64(1), (b << np.uint64(24)) | np.uint64(2)]))
    offs = np.array([0, WORST_BYTES], dtype=np.int64)
    s = torch.cuda.current_stream()
    events = torch.from_numpy(lst.view(np.int64)).cuda()
    nev = torch.full((1,), len(lst), dtype=torch.int64, device="cuda")
    d_offs = torch.from_numpy(offs).cuda()
    rptr = torch.zeros(2, dtype=torch.int64, device="cuda")
    nbytes = m.seq_rules_scratch_bytes(len(lst), 1)
    scratch = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hits = torch.zeros(4, dtype=torch.int64, device="cuda")
    res = {"stream_bytes": WORST_BYTES, "positions_per_range": n}

    def call():
        m.seq_rules_by_stream_device(events.data_ptr(), len(lst), nev.data_ptr(), d_offs.data_ptr(), 1, hits.data_ptr(),
                                     4, rptr.data_ptr(), scratch.data_ptr(), nbytes, s.cuda_stream)
    for name, rules in (("distance_only", [[(1, None), (2, 0)]]), ("within", [[(1, None), (2, 0, L + 1)]])):
        m.set_seq_rules(rules)
        q = stat(timed(torch, s, call, reps=reps, warm=1))
        exp_ptr, exp_hits = pm.seq_rules_by_stream_host(lst, offs, rules, plen)
        assert np.array_equal(rptr.cpu().numpy(), exp_ptr) and exp_ptr[-1] == 1
        assert np.array_equal(hits[:1].cpu().numpy().view(np.uint64), exp_hits)
        q["hit_position"] = int(exp_hits[0] >> np.uint64(24))
        res[name] = q
        print(f"worst {name}: {json.dumps(q)}", file=sys.stderr, flush=True)
    assert res["within"]["hit_position"] == int(b[-1])
    res["within_minus_distance_only_us"] = round(res["within"]["median_us"] - res["distance_only"]["median_us"], 1)
    return res


def child(step, reps, limit, env=None, cell=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--step", step, "--reps", str(reps)]
    p = subprocess.run(cmd + (["--cell", cell] if cell else []), stdout=subprocess.PIPE, text=True, timeout=limit,
                       env=env)
    line = [x for x in p.stdout.splitlines() if x.startswith("RESULT ")]
    if p.returncode != 0 or not line:
        raise RuntimeError(f"{step}: exit {p.returncode}")
    return json.loads(line[-1][7:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "within", "bench_within_rules.json"))
    ap.add_argument("--step", choices=["box", "worst", "bounded", "unbounded"], help="(internal) run one step")
    ap.add_argument("--cell", help="with --step: one cell only, e.g. lines_1500B")
    ap.add_argument("--reps", type=int, default=REPS, help="timed repetitions")
    ap.add_argument("--parent-lib", help="a libpm.so built from the parent commit: the unbounded comparison")
    ap.add_argument("--kernel-stats", metavar="CSV", help="add a kernel trace's statistics to --out as \"passes\"")
    a = ap.parse_args()
    if a.kernel_stats:
        with open(a.out) as f:
            doc = json.load(f)
        doc["passes"] = {"cell": "snort lines_1500B, --step bounded --reps 5 (each pass once per call: the count-only "
                                 "call, 3 warm-ups and 5 repetitions of dist0, bounded and dist0 again; "
                                 "sq_eval_kernel runs in the dist0 calls, sq_eval_within_kernel in the bounded ones)",
                         "kernels": kernel_stats(a.kernel_stats)}
        with open(a.out, "w") as f:
            json.dump(doc, f, indent=1)
            f.write("\n")
        return 0
    if a.step:
        r = (box() if a.step == "box" else step_worst(min(a.reps, 5)) if a.step == "worst" else
             step_cells("snort", a.cell, a.reps, unbounded_only=a.step == "unbounded"))
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "ordered rules with an upper bound (within) beside distance-only ordered rules on the same "
                   "all-matches list (batched scan, auto kind, snort, min_len 3, 64 MiB) in the same process; worst: one "
                   "lane walking two interleaved ranges of one 100 KiB stream, every candidate but the last failing by "
                   "one byte; unbounded: the dist0 set with this tree's library and the parent commit's",
           "reps": a.reps, "warmup": WARM, "min_len": MIN_LEN, "slack": SLACK}
    try:
        doc["box"] = child("box", a.reps, 120)
        doc["worst"] = child("worst", a.reps, 300)
        doc["bounded"] = child("bounded", a.reps, STEP_SECONDS)
        if a.parent_lib:
            runs = {"tree": [], "parent": []}
            for _ in range(PARENT_RUNS):
                for who, env in (("parent", dict(os.environ, PM_LIBPM=os.path.abspath(a.parent_lib))), ("tree", None)):
                    runs[who].append(child("unbounded", a.reps, STEP_SECONDS, env=env))
            cells = [k for k in runs["tree"][0] if isinstance(runs["tree"][0][k], dict)]
            out = {}
            for c in cells:
                t = sorted(r[c]["dist0"]["median_us"] for r in runs["tree"])
                p = sorted(r[c]["dist0"]["median_us"] for r in runs["parent"])
                out[c] = {"tree_median_us": t, "parent_median_us": p, "parent_spread": round(p[-1] / p[0], 3),
                          "tree_over_parent": round(t[len(t) // 2] / p[len(p) // 2], 3)}
            doc["unbounded"] = out
    except (RuntimeError, subprocess.TimeoutExpired) as e:
        print(f"{e}; stopping", file=sys.stderr)
        return 1
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
