#!/usr/bin/env python3
"""K6 several-subsets launch against one launch per subset: for every metric and both dtypes, the HIP-event kernel time
of ONE vf_degeneracy_scores_batch launch over {all, trans, rot} and the sum of the three vf_degeneracy_batch launches
(all, trans, rot) on the same seeded batch, 2^22 matrices by default (the size bench.py times K6 at).  Writes JSON
(profiles/k6_scores_timing.json by default).  Run from the repo root on a GPU box:

    timeout -k 10 600 python tools/k6_scores_timing.py

--pmc: one launch of each form for d_opt float64 and nothing else, for a counter pass of its own:

    rocprofv3 --pmc FETCH_SIZE -d <dir> -o k6 -f csv -- python tools/k6_scores_timing.py --pmc
    python tools/k6_scores_timing.py --fetch-summary <dir>/.../k6_counter_collection.csv
"""
import argparse
import csv
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def batch(count, dtype, seed=22):
    rng = np.random.default_rng(seed)
    A = rng.standard_normal(size=(count, 6, 6), dtype=np.float64)
    m = np.matmul(A, A.transpose(0, 2, 1))
    m += 0.5 * np.eye(6)
    return np.ascontiguousarray(m, dtype=dtype), np.ascontiguousarray(rng.normal(size=(count, 6)), dtype=dtype)


def run(lib, metric, m, p, subsets, reps):
    """kernel ms of the fused launch over `subsets` (reps > 0), its output rows"""
    from vil_sensor_fusion_amd._lib import check
    n = m.shape[0]
    mask = sum(1 << s for s in subsets)
    out = np.zeros((len(subsets), n), dtype=m.dtype)
    ms = C.c_float(0)
    check(lib.vf_degeneracy_scores_batch(m.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), n,
                                         0 if m.dtype == np.float64 else 1, metric, C.c_uint(mask),
                                         out.ctypes.data_as(C.c_void_p), reps, C.byref(ms)))
    return ms.value, out


def run_single(lib, metric, m, p, subset, reps):
    from vil_sensor_fusion_amd._lib import check
    n = m.shape[0]
    out = np.zeros(n, dtype=m.dtype)
    ms = C.c_float(0)
    check(lib.vf_degeneracy_batch(m.ctypes.data_as(C.c_void_p), p.ctypes.data_as(C.c_void_p), n,
                                  0 if m.dtype == np.float64 else 1, subset, metric, out.ctypes.data_as(C.c_void_p),
                                  reps, C.byref(ms)))
    return ms.value, out


def fetch_summary(path):
    """FETCH_SIZE (KB, summed over the dispatch's instances) per dispatch of a rocprofv3 counter CSV"""
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if r.get("Counter_Name") != "FETCH_SIZE":
                continue
            key = (int(r["Dispatch_Id"]), r["Kernel_Name"])
            rows.append((key, float(r["Counter_Value"])))
    per = {}
    for key, v in rows:
        per[key] = per.get(key, 0.0) + v
    return [{"dispatch": k[0], "kernel": k[1], "fetch_kb": v} for k, v in sorted(per.items())]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "k6_scores_timing.json"))
    ap.add_argument("--pmc", action="store_true", help="one launch of each form, d_opt float64 (for rocprofv3 --pmc)")
    ap.add_argument("--fetch-summary", metavar="CSV", help="print FETCH_SIZE per dispatch of a rocprofv3 counter CSV")
    a = ap.parse_args()
    if a.fetch_summary:
        print(json.dumps(fetch_summary(a.fetch_summary), indent=1))
        return
    from vil_sensor_fusion_amd import _lib
    from vil_sensor_fusion_amd import degeneracy as dg
    lib = _lib.lib()
    names = dg.METRICS + dg.EXTRA_METRICS
    if a.pmc:
        m, p = batch(a.count, np.float64)
        run(lib, 0, m, p, (0, 1, 2), 0)
        for s in (0, 1, 2):
            run_single(lib, 0, m, p, s, 0)
        print(f"d_opt float64, {a.count} matrices: one fused launch (all, trans, rot), then all, trans, rot alone; "
              f"one pass reads {a.count * 288 / 1024:.0f} KB of matrices")
        return
    res = {"count": a.count, "reps": a.reps, "subsets": ["all", "trans", "rot"], "unit": "ms per launch (HIP events)",
           "metrics": {}}
    t0 = time.time()
    for dt in (np.float64, np.float32):
        m, p = batch(a.count, dt)
        for k, name in enumerate(names):
            fused, rows = run(lib, k, m, p, (0, 1, 2), a.reps)
            single = []
            for s in (0, 1, 2):
                ms, y = run_single(lib, k, m, p, s, a.reps)
                single.append(ms)
                assert np.array_equal(y, rows[s], equal_nan=True), (name, s)
            r = {"fused_ms": round(fused, 4), "single_ms": [round(x, 4) for x in single], "sum_single_ms": round(sum(single), 4),
                 "fused_over_sum": round(fused / sum(single), 3) if sum(single) > 0 else None}
            res["metrics"].setdefault(name, {})[dt.__name__] = r
            print(f"{dt.__name__:8s} {name:28s} fused {fused:8.3f} ms  single {single[0]:7.3f} + {single[1]:7.3f} + {single[2]:7.3f}"
                  f" = {sum(single):8.3f} ms  ratio {r['fused_over_sum']}", flush=True)
        del m, p
    res["wall_s"] = round(time.time() - t0, 1)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
