#!/usr/bin/env python3
"""An omega study as CURVES: how the remaining divergence, the update norm and the iterations each solve took develop
over the steps, for one member per omega -- recorded by a history while the batch steps, without a host wait per step.

    python examples/history_curves.py [--steps 120] [--every 1] [--tol 1e-3 [--cap 400]] [--out history_curves.csv]

One batch of the sketch's 61 x 81 grid, the sketch's start with one drag in its first step.  Without --tol every member
runs 20 iterations per solve (iterations is then constant); with --tol every solve is stopped at the first check (one in
front of every 4th iteration) that finds the update norm <= T, at --cap iterations at the latest, and the iterations column
shows what each omega needed, step by step -- which sfl_batch_step_n_until alone reports only for the last step.  The CSV
has one line per sample and member: step, omega, max_abs_div, update_norm, iterations, max_abs_vx, max_abs_vy.

Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

OMEGAS = (1.0, 1.5, 1.8, 1.9, 1.96, 1.99)

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=1, help="a sample after every this-many-th step")
    ap.add_argument("--tol", type=float, default=None, help="stop every solve at this update norm")
    ap.add_argument("--cap", type=int, default=400, help="with --tol: iterations at the most")
    ap.add_argument("--out", default="history_curves.csv")
    args = ap.parse_args()
    batch = len(OMEGAS)
    with sfl.BatchSolver(61, 81, batch) as b:
        b.setup_sketch_fields()
        b.queue_forces(np.arange(batch), [(30, 40)] * batch, [(40.0, -25.0)] * batch)     # the same drag for every member
        b.history_start(args.every, max(args.steps // args.every, 1))
        if args.tol is None:   # ONE asynchronous call: the samples are taken on the stream between its step launches
            b.step_n_each(args.steps, dt=1 / 30, dx=1.0, iters=20, omega=OMEGAS)
        else:
            b.step_n_until(args.steps, dt=1 / 30, dx=1.0, max_iters=args.cap, omega=OMEGAS, tol=args.tol, every=4)
        curves = b.history()   # (samples, members): the one wait
    with open(args.out, "w") as f:
        f.write("step,omega,max_abs_div,update_norm,iterations,max_abs_vx,max_abs_vy\n")
        for sample in curves:
            for w, r in zip(OMEGAS, sample):
                f.write(f"{r['step']},{w:g},{r['max_abs_div']:.9g},{r['update_norm']:.9g},{r['iterations']},{r['max_abs_vx']:.9g},{r['max_abs_vy']:.9g}\n")
    print(f"{len(curves)} samples of {batch} members -> {args.out}")
    if len(curves):
        print("the last sample:   omega   max |div v|   update norm   iterations")
        for w, r in zip(OMEGAS, curves[-1]):
            print(f"                   {w:<7.2f}{r['max_abs_div']:>12.3e}{r['update_norm']:>14.3e}{r['iterations']:>13d}")
