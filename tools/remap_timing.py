#!/usr/bin/env python3
"""k_remap_covariance against the eigenvalue-only solve K6 already had: the HIP-event kernel time of
vf_degeneracy_remap_batch (all four outputs) and of vf_degeneracy_batch(condition_number, all) on the same float64 Hessians
in the same process, 2^20 of them by default, a fifth of them tunnel scans (one eigenvalue at 1e-6 of the nominal).  Writes
JSON (profiles/remap_timing.json by default) with the bytes moved per message and the achieved share of the HBM peak.  Run
from the repo root on a GPU box:

    timeout -k 10 300 python tools/remap_timing.py
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12        # bytes / s, MI355X data sheet


def hessians(count, seed=7):
    rng = np.random.default_rng(seed)
    q = np.linalg.qr(rng.normal(size=(count, 6, 6)) * 0.05 + np.eye(6))[0]
    ev = 4.0e4 * 10 ** rng.uniform(-0.15, 0.15, size=(count, 6))
    ev[rng.random(count) < 0.2, 0] *= 1e-6
    h = np.einsum("nik,nk,njk->nij", q, ev, q)
    return np.ascontiguousarray(0.5 * (h + h.transpose(0, 2, 1)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--count", type=int, default=1 << 20)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "remap_timing.json"))
    a = ap.parse_args()
    from vil_sensor_fusion_amd import _lib, degeneracy as dg
    H = hessians(a.count)
    nom = [0.2] * 6
    dg.remap_covariance(H[:4096], nom)                                   # warm-up: module load, first launch
    cov, sq, eig, dw, remap_ms = dg.remap_covariance(H, nom, reps=a.reps)
    out = np.zeros(a.count)
    ms = C.c_float(0)
    _lib.check(_lib.lib().vf_degeneracy_batch(H.ctypes.data_as(C.c_void_p), None, a.count, 0, 0, dg._metric_id("condition_number"),
                                              out.ctypes.data_as(C.c_void_p), a.reps, C.byref(ms)))
    # the two solves see the same spectra: -cond from the values-only solve against max / min of eig6
    np.testing.assert_allclose(-out[1:], eig[1:, 5] / eig[1:, 0], rtol=1e-6)
    moved = {"remap": 36 * 8 + 36 * 8 + 21 * 8 + 6 * 8 + 4, "condition_number": 36 * 8 + 8}
    res = {"count": a.count, "reps": a.reps, "dtype": "float64", "unit": "ms per launch (HIP events, after a warm-up launch)",
           "deweighted_share": round(float(np.mean(dw > 0)), 4), "hbm_peak_bytes_per_s": HBM_PEAK,
           "remap": {"kernel_ms": round(remap_ms, 4), "bytes_per_message": moved["remap"]},
           "condition_number_all": {"kernel_ms": round(ms.value, 4), "bytes_per_message": moved["condition_number"]}}
    for k, key in (("remap", "remap"), ("condition_number_all", "condition_number")):
        r = res[k]
        r["ns_per_message"] = round(r["kernel_ms"] * 1e6 / a.count, 3)
        r["gbytes_per_s"] = round(moved[key] * a.count / (r["kernel_ms"] * 1e-3) / 1e9, 1)
        r["share_of_hbm_peak"] = round(moved[key] * a.count / (r["kernel_ms"] * 1e-3) / HBM_PEAK, 4)
    res["remap_over_condition_number"] = round(remap_ms / ms.value, 2)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))
    print("wrote", a.out)


if __name__ == "__main__":
    main()
