"""Time of the score ranking metrics at the configs[1] size.

  python tools/metrics_time.py [--rows 17762295] [--calls 20] [--out profiles/metrics_time.json]

fdx_ranking_metrics on `rows` scores rounded to 1e-4 (tie-heavy, as a forest's probabilities are)
and fdx_threshold_counts with 100 thresholds: HIP events around each call, `calls` calls after
warm-up, median and spread.  Then the per-kernel split from a rocprofv3 kernel trace of the same
calls (a run of its own: tracing slows the host), and scikit-learn's roc_auc_score +
average_precision_score on the same arrays and host as a CPU baseline (one run).

The steps are fresh child processes, each under its own `timeout -k 10`; the first one that fails
ends the run (the parent never opens the GPU).  One JSON line goes to stdout and to --out.
"""
import argparse
import collections
import csv
import glob
import json
import os
import re
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time_fraud_detection_system_amd"))

N_THR = 100
WARMUP = 3


def inputs(rows):
    import numpy as np

    rng = np.random.default_rng(0)
    p = np.round(rng.beta(0.3, 3, rows) * 1e4) / 1e4
    y = (rng.random(rows) < p * 0.5 + 0.002).astype(np.uint8)
    return p, y


def spread(ms):
    s = sorted(ms)
    return {"median_ms": round(s[len(s) // 2], 4), "min_ms": round(s[0], 4), "max_ms": round(s[-1], 4), "calls": len(s)}


def device_calls(rows, calls, timed):
    """Warm-up, then `calls` calls of each entry point; timed: HIP events around each call."""
    import numpy as np
    import torch

    from fdx import ops

    dev = ops.require_gpu()
    p, y = inputs(rows)
    s_d, y_d = torch.from_numpy(p).to(dev), torch.from_numpy(y).to(dev)
    thr_d = torch.linspace(0.0, 0.99, N_THR, dtype=torch.float64, device=dev)
    out = {}
    for name, call in (("ranking_metrics", lambda: ops.ranking_metrics(s_d, y_d)),
                       ("threshold_counts", lambda: ops.threshold_counts(s_d, y_d, thr_d))):
        for _ in range(WARMUP):
            last = call()
        torch.cuda.synchronize()
        ms = []
        for _ in range(calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            last = call()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        out[name] = spread(ms)
        if name == "ranking_metrics":
            out["result"] = last.host()
    if not timed:
        return {}
    # how many of the sort's 8 digit passes see one digit value only (host restatement of the key;
    # the scores are >= +0.0)
    b = p.view(np.uint64)
    key = ~np.where(b >> np.uint64(63), ~b, b | np.uint64(1 << 63))
    both, either = np.bitwise_and.reduce(key), np.bitwise_or.reduce(key)
    out["constant_digit_passes"] = sum(1 for d in range(8) if (int(both) >> 8 * d) & 255 == (int(either) >> 8 * d) & 255)
    out["device"] = torch.cuda.get_device_name(0)
    return out


def sklearn_baseline(rows):
    from sklearn.metrics import average_precision_score, roc_auc_score

    p, y = inputs(rows)
    t = time.perf_counter()
    auc, ap = roc_auc_score(y, p), average_precision_score(y, p)
    return {"sklearn_cpu_s": round(time.perf_counter() - t, 3), "sklearn_auc": float(auc), "sklearn_ap": float(ap),
            "cpus": len(os.sched_getaffinity(0))}


def kernel_split(trace_dir, calls):
    """us per call and kernel from the rocprofv3 kernel trace (warm-up calls included in the mean)."""
    per = collections.defaultdict(float)
    for f in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            m = re.search(r"k_[a-z0-9_]+", r["Kernel_Name"])  # (mangled or not)
            if m and "fdx" in r["Kernel_Name"]:
                per[m.group(0)] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    return {k: round(v / (calls + WARMUP), 2) for k, v in sorted(per.items(), key=lambda kv: -kv[1])}


def algorithmic_bytes_per_row():
    """Key pass 8 + 8; per radix pass the histogram reads the key (8) and the scatter reads and
    writes key + value (12 + 12; the first reads key + label, 9); the scan reads key + value twice."""
    return {"keys": 16, "sort": 8 * 8 + (9 + 12) + 7 * 24, "scan": 24}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=17_762_295)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "metrics_time.json"))
    ap.add_argument("--step", choices=["time", "calls", "sklearn"], help="(internal) one step, as a child process")
    a = ap.parse_args()
    if a.step:
        r = {"time": lambda: device_calls(a.rows, a.calls, True), "calls": lambda: device_calls(a.rows, a.calls, False),
             "sklearn": lambda: sklearn_baseline(a.rows)}[a.step]()
        print("STEP " + json.dumps(r), flush=True)
        return

    def step(name, limit, prefix=()):
        cmd = ["timeout", "-k", "10", str(limit), *prefix, sys.executable, os.path.abspath(__file__), "--step", name,
               "--rows", str(a.rows), "--calls", str(a.calls)]
        p = subprocess.run(cmd, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if p.returncode != 0:
            sys.exit(f"step {name} failed ({p.returncode}):\n{p.stdout[-3000:]}")
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("STEP ")]
        return json.loads(lines[-1][5:])

    res = {"rows": a.rows, "n_thresholds": N_THR}
    res.update(step("time", 240))
    with tempfile.TemporaryDirectory() as d:
        step("calls", 300, ("rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--"))
        res["kernel_us_per_call"] = kernel_split(d, a.calls)
    res.update(step("sklearn", 300))
    r = res["result"]
    res["auc_rel_diff_vs_sklearn"] = abs(r["auc"] - res["sklearn_auc"]) / res["sklearn_auc"]
    res["ap_rel_diff_vs_sklearn"] = abs(r["ap"] - res["sklearn_ap"]) / res["sklearn_ap"]
    res["algorithmic_bytes_per_row"] = algorithmic_bytes_per_row()
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
