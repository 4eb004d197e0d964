#!/usr/bin/env python3
"""Which omega and how many SOR iterations does the sketch's 61 x 81 grid need?  One batch, one member per (omega, iters)
point, the sketch's start with one drag, a few steps -- and the update norm of every member's last solve as a table.

    python examples/omega_study.py [--steps 5] [--tol T [--cap K]]

With --tol the question is asked directly: one member per omega, every solve stopped at the first check (one in front of
every 4th iteration) that finds the update norm <= T, at K iterations (default 400) at the latest -- and the table is the
iterations each omega used.

Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

OMEGAS = (1.0, 1.5, 1.8, 1.9, 1.96, 1.99)
ITERS = (5, 10, 20, 40, 80)

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--tol", type=float, default=None, help="stop every solve at this update norm: one member per omega")
    ap.add_argument("--cap", type=int, default=400, help="with --tol: iterations at the most")
    args = ap.parse_args()
    steps = args.steps
    if args.tol is not None:
        with sfl.BatchSolver(61, 81, len(OMEGAS)) as b:
            b.setup_sketch_fields()
            b.queue_forces(np.arange(len(OMEGAS)), [(30, 40)] * len(OMEGAS), [(40.0, -25.0)] * len(OMEGAS))
            b.step_n_until(steps, dt=1 / 30, dx=1.0, max_iters=args.cap, omega=OMEGAS, tol=args.tol, every=4)
            used, norm = b.iterations(), b.residual()
        print(f"SOR iterations to an update norm max |p_gs - p| <= {args.tol:g} (checked every 4, at most {args.cap}), "
              f"61 x 81, {steps} steps")
        print("omega   last step   all steps   final norm")
        for w, (last, total), r in zip(OMEGAS, used, norm):
            print(f"{w:<7.2f}{last:>10d}{'*' if last == args.cap else ' '}{total:>11d}   {r:>10.3e}")
        print("(* = the cap)")
        sys.exit(0)
    omega, iters = (a.reshape(-1) for a in np.meshgrid(OMEGAS, ITERS, indexing="ij"))   # member = omega-major
    batch = len(omega)
    with sfl.BatchSolver(61, 81, batch) as b:
        b.setup_sketch_fields()
        b.queue_forces(np.arange(batch), [(30, 40)] * batch, [(40.0, -25.0)] * batch)     # the same drag for every member
        b.step_n_each(steps, dt=1 / 30, dx=1.0, iters=iters, omega=omega)
        norm = b.residual().reshape(len(OMEGAS), len(ITERS))
    print(f"update norm max |p_gs - p| after {steps} steps, 61 x 81 (rows: omega, columns: SOR iterations)")
    print("omega  " + "".join(f"{n:>11d}" for n in ITERS))
    for w, row in zip(OMEGAS, norm):
        print(f"{w:<7.2f}" + "".join(f"{r:>11.3e}" for r in row))
