#!/usr/bin/env python3
"""The flow scan (pm_hip_scan_flows_device) beside the two calls that bracket
it: the batched scan it extends and the unsegmented DFA walk it is cut from.

Device-resident, snort and merged dictionaries, 64 MiB in HBM of (1) gen_stream
mode 0 ASCII and (2) the lines stream (dense deep matches), cut into 1,500-byte
and 100 KiB streams, u32 ids.  Per dictionary, text and cut, hipEvent times of
REPS repetitions after warm-up, min and median:
  flows    one pm_hip_scan_flows_device call of an ac object, every stream
           carrying a state in (the states an earlier call over the same
           buffer left) and a state out;
  batch    (a) one pm_hip_scan_batch_device call of an auto object over the
           same bytes and offsets: the batched path without carried state
           (the reverse-trie walk, rt_batch_kernel);
  dense    (b) one unsegmented pm_hip_scan_device of the ac object with
           "dfa_form" 1 over the same bytes: the same table walk
           (dfa_coded_kernel) without streams or states.
With no state in, the flow call's ids are checked against the batch call's.

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
CUTS = {"1500B": 1500, "100KiB": 100 << 10}
DICTS = {"snort": ["snort.dict"], "merged": ["snort.dict", "et.dict"]}
REPS, WARM = 20, 3
STEP_SECONDS = 420


def stat(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2)}


def matcher(pm, kind, key):
    m = pm.HipMatcher(kind)
    m.add_dictionary(pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", f) for f in DICTS[key]]))
    m.compile()
    return m


def timed(torch, s, fn, reps=REPS, warm=WARM):
    us = []
    for r in range(warm + reps):
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
    assert ac.set_option("dfa_form", 1) == 0
    s = torch.cuda.current_stream()
    N, sp = N_DEVICE, s.cuda_stream
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    out = torch.zeros(N, dtype=torch.int32, device="cuda")
    out2 = torch.zeros(N, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    res = {"bytes": N, "patterns": int(lib.pm_hip_n_patterns(ac.obj)), "flow_states": int(ac.flow_states),
           "table_bytes_ac": int(ac.table_bytes)}

    def gbps(us):
        return round(N / (statistics.median(us) * 1e-6) / 1e9, 1)

    for stream in ("ascii", "lines"):
        if stream == "ascii":
            lib.pm_hip_gen_stream_device(text.data_ptr(), 0, N + 64, 3, 0, sp)
        else:
            ac.gen_lines_device(text.data_ptr(), N + 64, 3, sp)
        torch.cuda.synchronize()
        tp = text.data_ptr()
        us = timed(torch, s, lambda: ac.scan_device(tp, 0, 0, N, out.data_ptr(), cnt.data_ptr(), sp))
        assert ac.kernel_last == pm.KIND_AC and ac.dfa_form_last == 1
        dense = dict(stat(us), gbps_median=gbps(us))
        for cut, L in CUTS.items():
            offs = np.append(np.arange(0, N, L, dtype=np.int64), np.int64(N))
            nseg = len(offs) - 1
            d_offs = torch.from_numpy(offs).cuda()
            op = d_offs.data_ptr()
            st = [torch.zeros(nseg, dtype=torch.int32, device="cuda") for _ in range(2)]
            r = {"stream_bytes": L, "streams": nseg, "dense": dense}
            us = timed(torch, s, lambda: auto.scan_batch_device(tp, op, nseg, N, out2.data_ptr(), cnt.data_ptr(), sp))
            assert auto.kernel_last == pm.KIND_RT
            r["batch"] = dict(stat(us), gbps_median=gbps(us))
            # fresh flows: the batch call's ids; and the states the timed calls start from
            ac.scan_flows_device(tp, op, nseg, N, None, st[0].data_ptr(), out.data_ptr(), None, sp)
            torch.cuda.synchronize()
            r["ids_equal_batch"] = bool(torch.equal(out, out2))
            assert r["ids_equal_batch"]
            r["streams_ending_off_the_root"] = int(torch.count_nonzero(st[0]).item())
            us = timed(torch, s, lambda: ac.scan_flows_device(tp, op, nseg, N, st[0].data_ptr(), st[1].data_ptr(),
                                                              out.data_ptr(), cnt.data_ptr(), sp))
            assert ac.kernel_last == pm.KIND_AC and ac.dfa_form_last == 1
            r["flows"] = dict(stat(us), gbps_median=gbps(us))
            us = timed(torch, s, lambda: ac.scan_flows_device(tp, op, nseg, N, st[0].data_ptr(), st[1].data_ptr(),
                                                              None, cnt.data_ptr(), sp))
            r["flows_count_only"] = dict(stat(us), gbps_median=gbps(us))
            r["flows_over_dense"] = round(r["flows"]["median_us"] / dense["median_us"], 3)
            r["flows_over_batch"] = round(r["flows"]["median_us"] / r["batch"]["median_us"], 3)
            res[f"{stream}_{cut}"] = r
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "host": platform.node(), "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "flows", "bench_flows.json"))
    ap.add_argument("--step", choices=sorted(DICTS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_dict(a.step)
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "flow scan (ac kind, state in and out per stream) vs the batched scan (auto kind, no carry) vs one "
                   "unsegmented dense-row scan_device (ac kind, dfa_form 1); 64 MiB, gen_stream mode 0 seed 3 and the "
                   "lines stream seed 3, u32 ids", "reps": REPS, "warmup": WARM}
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
