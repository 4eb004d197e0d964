#!/usr/bin/env python3
"""What a convergence check costs on a whole-domain context (sfl_residual, sfl_poisson_solve_until).

  overhead   sfl_poisson_solve_until(cap, every, tol = 0: every check is made, none stops the solve) against
             sfl_poisson_solve(cap), warmed, in one process, the calls alternating, host clock around synchronous calls:
             microseconds per call (median and minimum over --reps) and the overhead per check.
  trace      the launches a kernel trace wants to see: --reps solves of `cap` iterations, then --reps residuals (run it under
             rocprofv3 --kernel-trace --stats in a run of its own: tools/recipes/context_until.sh reads the trace).

usage: python3 tools/context_until_probe.py overhead|trace [--size N ...] [--cap K] [--every E ...] [--reps R]"""
import argparse
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")


def context(size):
    s = sfl.Solver(size, size)
    rng = np.random.default_rng(size)
    d = rng.standard_normal((size, size), dtype=np.float32)
    s.upload(sfl.capi.FIELD_DIVERGENCE, d - d.mean(dtype=np.float64).astype(np.float32))
    return s


def timed(call, s):
    s.synchronize()
    t = time.perf_counter()
    call()
    s.synchronize()
    return (time.perf_counter() - t) * 1e6


def overhead(a):
    for size in a.size:
        with context(size) as s:
            calls = {"solve": lambda: s.poisson_solve(1.0, a.cap, 1.9)}
            for e in a.every:
                calls[f"until every {e}"] = (lambda e=e: s.poisson_solve_until(1.0, a.cap, 1.9, tol=0.0, every=e))
            calls["residual"] = lambda: s.residual(1.0)
            for _ in range(a.warmup):
                for c in calls.values():
                    timed(c, s)
            us = {n: [] for n in calls}
            for _ in range(a.reps):          # alternating: every round runs each call once
                for n, c in calls.items():
                    us[n].append(timed(c, s))
            k, u = s.poisson_solve_until(1.0, a.cap, 1.9, tol=0.0, every=a.every[0])
            base = statistics.median(us["solve"])
            print(f"{size} x {size}, cap {a.cap}, omega 1.9, {a.reps} rounds (until ran {k} iterations, norm {u:.4g}):")
            for n, v in us.items():
                line = f"  {n:<16} median {statistics.median(v):9.1f} us   min {min(v):9.1f} us"
                if n.startswith("until"):
                    checks = -(-a.cap // int(n.split()[-1])) + 1      # k = 0, every, ... < cap, and the final norm
                    extra = statistics.median(v) - base
                    line += f"   {checks:3d} checks: +{extra:8.1f} us = {100 * extra / base:5.1f} % of the solve, {extra / checks:6.1f} us per check"
                print(line)
            sys.stdout.flush()


def trace(a):
    for size in a.size:
        with context(size) as s:
            for _ in range(a.reps):
                s.poisson_solve(1.0, a.cap, 1.9)
            s.synchronize()
            for _ in range(a.reps):
                s.residual(1.0)
            print(f"{size} x {size}: {a.reps} solves of {a.cap} iterations (launches {s.last_solve_info()}), {a.reps} residuals")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["overhead", "trace"])
    ap.add_argument("--size", type=int, nargs="+", default=[8192, 2048])
    ap.add_argument("--cap", type=int, default=80)
    ap.add_argument("--every", type=int, nargs="+", default=[8, 16, 40])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    {"overhead": overhead, "trace": trace}[a.mode](a)
