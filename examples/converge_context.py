#!/usr/bin/env python3
"""How many SOR iterations does each omega need at ONE grid size, on a whole-domain context of any size?

    python examples/converge_context.py [--size 512] [--tol 1e-2] [--cap 5000] [--every 16] [--omega 1.8 1.9 1.96 1.98 1.99]

One context, a zero-mean random right-hand side (under the all-Neumann stencil anything else plateaus), and for every omega
one sfl_poisson_solve_until: the solve stops at the first check -- one in front of every `every`-th iteration -- that finds
the update norm max |p_gs - p| <= tol, at the cap at the latest.  Printed: the iterations used, the norm they left and the
time of the call.  A check is one pass over p and d: with a small --every the time is the checks' as much as the solve's.

Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--tol", type=float, default=1e-2)
    ap.add_argument("--cap", type=int, default=5000)
    ap.add_argument("--every", type=int, default=16)
    ap.add_argument("--omega", type=float, nargs="+", default=[1.8, 1.9, 1.96, 1.98, 1.99])
    args = ap.parse_args()
    n = args.size
    d = np.random.default_rng(n).standard_normal((n, n), dtype=np.float32)
    d -= d.mean(dtype=np.float64).astype(np.float32)
    with sfl.Solver(n, n) as s:
        s.upload(sfl.capi.FIELD_DIVERGENCE, d)
        s.poisson_solve_until(1.0, args.every, args.omega[0], tol=args.tol, every=args.every)     # warm-up: code objects
        print(f"SOR iterations to an update norm max |p_gs - p| <= {args.tol:g} (checked every {args.every}, at most {args.cap}), "
              f"{n} x {n}")
        print("omega   iterations   final norm        ms")
        for w in args.omega:
            t = time.perf_counter()
            used, norm = s.poisson_solve_until(1.0, args.cap, w, tol=args.tol, every=args.every)
            ms = (time.perf_counter() - t) * 1e3
            print(f"{w:<7.2f}{used:>10d}{'*' if used == args.cap else ' '}  {norm:>10.3e}{ms:>10.2f}")
        print("(* = the cap)")
