#!/usr/bin/env python3
"""The nocase calls (pm_hip_scan_batch_nocase_device,
pm_hip_scan_flows_nocase_device, all form, min_len 3) beside the window call
of the same process with every window unbounded.

scripts/bench_windows.py's cells, inputs and timing: device-resident, snort and
merged dictionaries, 64 MiB in HBM of (1) gen_stream mode 0 ASCII and (2) the
lines stream, cut into 1,500-byte and 100 KiB streams; hipEvent times of REPS
repetitions after warm-up, min and median, all of one cell in one process.  No
group tables; the window table is unbounded for every pattern, so the window
call's list is the all-matches list.  Per dictionary, text, cut and family
(batch: an auto object's reverse-trie walk; flows: an ac object's dense-row
walk, state, byte count and case history in and out, every flow fresh):
  windows_a    the window call: the baseline;
  all          every pattern nocase: the folded walk, no confirmation;
  none         no pattern nocase: every candidate that holds a letter is
               confirmed against the text; the list is the baseline's (checked);
  crc          nocase where crc32(pattern) & 1;
  windows_b    the window call once more: windows_b / windows_a is its spread.
Beside the times: the events of each list and its growth over the baseline's,
the confirmations per byte (counted on the host from the `all` list, which
holds every candidate: those whose pattern is case-sensitive under the leg's
flags and holds a letter), pm_hip_set_nocase's build and upload time and the
table bytes it added.

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
import zlib

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

N_DEVICE = 64 << 20
EVENTS_CAP = N_DEVICE
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
    P = len(pats)
    flagsets = {"all": np.ones(P, np.uint8), "none": np.zeros(P, np.uint8),
                "crc": np.array([zlib.crc32(p) & 1 for p in pats], np.uint8)}
    letter = np.array([any(65 <= c <= 90 or 97 <= c <= 122 for c in p) for p in pats])
    objs = {}
    for kind in ("ac", "auto"):
        m = pm.HipMatcher(kind)
        m.add_dictionary(d)
        m.compile()
        m.set_windows(np.zeros(P, np.uint32), np.full(P, INF, np.uint32))
        objs[kind] = m
    ac, auto = objs["ac"], objs["auto"]
    G = int(lib.pm_hip_n_patterns(ac.obj))
    index_of_gid = np.array([0] + [lib.pm_hip_gid_index(ac.obj, g) for g in range(1, G + 1)])
    # per gid: a confirmation under these flags
    confirms = {name: np.concatenate([[False], (letter & (f == 0))[index_of_gid[1:]]]) for name, f in flagsets.items()}

    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    events = torch.zeros(EVENTS_CAP, dtype=torch.int64, device="cuda")
    nev = torch.zeros(1, dtype=torch.int64, device="cuda")
    tp, ep, np_ = text.data_ptr(), events.data_ptr(), nev.data_ptr()
    res = {"bytes": N, "patterns": G, "events_cap": EVENTS_CAP, "set_nocase": {}}

    def sorted_list():
        total = int(nev.item())
        assert total <= EVENTS_CAP, total
        return torch.sort(events[:total]).values

    # One pass over every cell per leg, so that pm_hip_set_nocase (which rebuilds the folded images)
    # runs once per flag set and object; the texts are generated again per pass (same seeds).
    base = {}  # (cell, family) -> the window list's (count, sum, xor)
    for pass_name in ("windows_a", "all", "none", "crc", "windows_b"):
        if pass_name in flagsets:
            for kind, m in objs.items():
                m.set_nocase(flagsets[pass_name])
                b, u, t = m.nocase_stats()
                res["set_nocase"][f"{pass_name}_{kind}"] = {
                    "build_ms": round(b, 1), "upload_ms": round(u, 1), "table_bytes": t, "case_words": m.case_words,
                    "folded_flow_states": m.nocase_flow_states}
                assert m.case_words <= 8
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
                ps = [torch.zeros(nseg, dtype=torch.int64, device="cuda") for _ in range(2)]
                cs = [torch.zeros(nseg * 8, dtype=torch.int64, device="cuda") for _ in range(2)]
                s0, s1, p0, p1 = st[0].data_ptr(), st[1].data_ptr(), ps[0].data_ptr(), ps[1].data_ptr()
                c0, c1 = cs[0].data_ptr(), cs[1].data_ptr()
                calls = {
                    "batch": {
                        "windows": lambda: auto.scan_batch_windows_device(tp, op, nseg, N, None, 3, True, ep,
                                                                          EVENTS_CAP, np_, sp),
                        "nocase": lambda: auto.scan_batch_nocase_device(tp, op, nseg, N, None, 3, True, ep,
                                                                        EVENTS_CAP, np_, sp),
                    },
                    "flows": {
                        "windows": lambda: ac.scan_flows_windows_device(tp, op, nseg, N, s0, s1, None, 3, True, ep,
                                                                        EVENTS_CAP, np_, sp, p0, p1),
                        "nocase": lambda: ac.scan_flows_nocase_device(tp, op, nseg, N, s0, s1, None, 3, True, ep,
                                                                      EVENTS_CAP, np_, sp, p0, p1, c0, c1),
                    },
                }
                cell = res.setdefault(f"{stream}_{cut}", {"stream_bytes": L, "streams": nseg})
                for family, c in calls.items():
                    r = cell.setdefault(family, {})
                    call = c["nocase" if pass_name in flagsets else "windows"]
                    r[pass_name] = stat(timed(torch, s, call, pre=lambda: nev.zero_()))
                    r[pass_name]["events"] = int(nev.item())
                    got = sorted_list()
                    sig = (int(got.numel()), int(got.sum().item()), int(np.bitwise_xor.reduce(got.cpu().numpy())))
                    if pass_name == "windows_a":
                        base[(stream, cut, family)] = sig
                    if pass_name in ("none", "windows_b"):
                        assert sig == base[(stream, cut, family)], f"{stream} {cut} {family} {pass_name}: another list"
                    if pass_name == "all":  # the list of every candidate: the confirmations of each flag set
                        every = (got & 0xFFFFFF).cpu().numpy()
                        r["confirmations_per_byte"] = {
                            name: round(int(np.count_nonzero(confirms[name][every])) / N, 6) for name in flagsets}
    for cell in res.values():
        if not isinstance(cell, dict) or "batch" not in cell:
            continue
        for family in ("batch", "flows"):
            r = cell[family]
            wt = min(r["windows_a"]["median_us"], r["windows_b"]["median_us"])
            for name in flagsets:
                r[f"{name}_over_windows"] = round(r[name]["median_us"] / wt, 3)
                r[name]["list_growth"] = round(r[name]["events"] / max(r["windows_a"]["events"], 1), 4)
            r["windows_spread"] = round(max(r["windows_a"]["median_us"], r["windows_b"]["median_us"]) / wt, 3)
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "nocase", "bench_nocase.json"))
    ap.add_argument("--dicts", default=",".join(DICTS), help="comma-separated subset of: " + ", ".join(DICTS))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "nocase call (all form, min_len 3, no group tables, every window unbounded; flags: every pattern, "
                   "none, crc32 & 1) vs the window call (timed twice: its spread); batched scan (auto kind) and flow "
                   "scan (ac kind; state, byte count and case history in and out per stream, every flow fresh); 64 "
                   "MiB, gen_stream mode 0 seed 3 and the lines stream seed 3", "reps": REPS, "warmup": WARM}
    for step, limit in [("box", 120)] + [(k, STEP_SECONDS) for k in a.dicts.split(",")]:
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
