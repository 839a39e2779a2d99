#!/usr/bin/env python3
"""The batched scan (pm_hip_scan_batch_device, pm_hip_read_batch_gid) against
what the library offered before it for the same work, and against its ceiling.

Device-resident, snort dictionary, 64 MiB of gen_stream mode 0 ASCII, cut into
(a) 100 KiB streams (the reference's chunk, measure.c:77) and (b) 1,500-byte
streams.  Per cut, hipEvent times of REPS repetitions after warm-up, min and
median, for u32 ids and for count only:
  batch    one pm_hip_scan_batch_device call;
  loop     one pm_hip_scan_device launch per stream, stream_start = pos0 =
           the stream's first byte rounded down to 16 as that call requires
           (its answers at the cuts are then those of a stream beginning
           there).  At 1,500 B the first LOOP_STREAMS streams are timed and
           the time scaled to all of them ("scaled": true);
  ceiling  one unsegmented pm_hip_scan_device over the same 64 MiB (wrong
           answers at the cuts, the same traffic).
Host path: pm_hip_read_batch_gid over 16 MiB in 100 KiB streams against the
loop of reset() + read_block_gid (the resident server), host wall clock,
both into result arrays made once.

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
N_HOST = 16 << 20
CUTS = {"100KiB": 100 << 10, "1500B": 1500}
LOOP_STREAMS = 4096
REPS, WARM = 20, 3
STEPS = {"device_100KiB": 300, "device_1500B": 300, "host_100KiB": 300}  # seconds each


def stat(us):
    return {"min_us": round(min(us), 2), "median_us": round(statistics.median(us), 2)}


def matcher():
    import patternmatching_amd as pm
    m = pm.HipMatcher("rt")
    m.add_dictionary(pm.Dictionary([os.path.join(REPO, "tests", "golden", "data", "snort.dict")]))
    m.compile()
    return pm, m


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


def step_device(cut):
    import numpy as np
    import torch
    pm, m = matcher()
    lib = pm.load()
    s = torch.cuda.current_stream()
    L, N = CUTS[cut], N_DEVICE
    text = torch.empty(N + 64, dtype=torch.uint8, device="cuda")
    lib.pm_hip_gen_stream_device(text.data_ptr(), 0, N + 64, 3, 0, s.cuda_stream)
    offs = np.append(np.arange(0, N, L, dtype=np.int64), np.int64(N))
    nseg = len(offs) - 1
    d_offs = torch.from_numpy(offs).cuda()
    out = torch.zeros(N, dtype=torch.int32, device="cuda")
    out2 = torch.zeros(N, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(1, dtype=torch.int64, device="cuda")
    tp, op, sp = text.data_ptr(), d_offs.data_ptr(), s.cuda_stream
    res = {"stream_bytes": L, "streams": nseg, "bytes": N}

    def gbps(us):
        return round(N / (statistics.median(us) * 1e-6) / 1e9, 1)

    for mode, o in (("ids_u32", out), ("count", None)):
        optr = o.data_ptr() if o is not None else None
        us = timed(torch, s, lambda: m.scan_batch_device(tp, op, nseg, N, optr, cnt.data_ptr(), sp))
        res[f"batch_{mode}"] = dict(stat(us), gbps_median=gbps(us))
        us = timed(torch, s, lambda: m.scan_device(tp, 0, 0, N, optr, cnt.data_ptr(), sp))
        res[f"ceiling_{mode}"] = dict(stat(us), gbps_median=gbps(us))
        k = min(nseg, LOOP_STREAMS)
        starts = [int(a) & ~15 for a in offs[:k]]
        lens = [int(b - a) for a, b in zip(offs[:k], offs[1:k + 1])]
        o2 = out2.data_ptr() if o is not None else None

        def loop():
            for a, ln in zip(starts, lens):
                m.scan_device(tp, a, a, ln, o2 + 4 * a if o2 else None, cnt.data_ptr(), sp)

        us = [t * nseg / k for t in timed(torch, s, loop)]
        res[f"loop_{mode}"] = dict(stat(us), gbps_median=gbps(us), streams_timed=k, scaled=k != nseg)
        res[f"batch_over_ceiling_{mode}"] = round(res[f"ceiling_{mode}"]["median_us"] /
                                                  res[f"batch_{mode}"]["median_us"], 3)
        res[f"batch_over_loop_{mode}"] = round(res[f"loop_{mode}"]["median_us"] / res[f"batch_{mode}"]["median_us"], 1)
    # where every stream starts on a multiple of 16 the loop scans exactly the
    # batch's streams: the ids agree
    if all(int(a) % 16 == 0 for a in offs[:-1]):
        m.scan_batch_device(tp, op, nseg, N, out.data_ptr(), None, sp)
        torch.cuda.synchronize()
        res["ids_equal_loop"] = bool(torch.equal(out, out2))
        assert res["ids_equal_loop"]
    return res


def step_host():
    import numpy as np
    pm, m = matcher()
    L, N = CUTS["100KiB"], N_HOST
    text = pm.gen_stream(N, 3, 0)
    offs = np.append(np.arange(0, N, L, dtype=np.int64), np.int64(N))
    import ctypes
    lib = pm.load()
    u8p, u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)
    res = {"stream_bytes": L, "streams": len(offs) - 1, "bytes": N}
    # both paths fill arrays made once (a fresh 64 MiB array per call would
    # time its page faults)
    got = {"batch": np.zeros(N, np.uint32), "loop": np.zeros(N, np.uint32)}
    pieces = [(ctypes.cast(text.ctypes.data + int(a), u8p), int(b - a),
               ctypes.cast(got["loop"].ctypes.data + 4 * int(a), u32p)) for a, b in zip(offs[:-1], offs[1:])]

    def batch():
        m.read_batch_gids(text, offs, out=got["batch"])

    def loop():
        for src, ln, dst in pieces:
            lib.pm_hip_reset(m.obj)
            lib.pm_hip_read_block_gid(m.obj, src, ln, dst)

    for name, fn in (("read_batch_gid", batch), ("reset_read_block_gid_loop", loop)):
        us = []
        for r in range(WARM + REPS):
            t0 = time.perf_counter()
            fn()
            if r >= WARM:
                us.append((time.perf_counter() - t0) * 1e6)
        res[name] = dict(stat(us), gbps_median=round(N / (statistics.median(us) * 1e-6) / 1e9, 2))
    res["serve_calls"] = m.serve_stats()["calls"]
    res["ids_equal_loop"] = bool(np.array_equal(got["batch"], got["loop"]))
    assert res["ids_equal_loop"]
    res["batch_over_loop"] = round(res["reset_read_block_gid_loop"]["median_us"] / res["read_batch_gid"]["median_us"], 1)
    return res


def box():
    import torch
    p = torch.cuda.get_device_properties(0)
    return {"device": p.name, "arch": getattr(p, "gcnArchName", ""), "compute_units": p.multi_processor_count,
            "hbm_bytes": p.total_memory, "hip": torch.version.hip, "torch": torch.__version__,
            "host": platform.node(), "python": platform.python_version()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "batch", "bench_batch.json"))
    ap.add_argument("--step", choices=sorted(STEPS) + ["box"], help="(internal) run one step, print its JSON")
    a = ap.parse_args()
    if a.step:
        r = box() if a.step == "box" else step_host() if a.step.startswith("host") else \
            step_device(a.step.split("_", 1)[1])
        print("RESULT " + json.dumps(r))
        return 0
    doc = {"what": "batched scan vs a scan_device launch per stream vs one unsegmented scan; snort, rt kind, "
                   "gen_stream mode 0 seed 3", "reps": REPS, "warmup": WARM}
    for step, limit in [("box", 120)] + list(STEPS.items()):
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
