#!/usr/bin/env python3
"""Drag against viscosity: one batch, one peg, nu per member over a few decades, ONE step_n_each call.

    python examples/reynolds_study.py --members 16 --steps 300 --out reynolds.csv

Every member is the same 96 x 64 channel with the same peg (a shared mask) and the same inflow; the members differ in nu
alone (sfl_batch_set_viscosity, per member), from --nu-min to --nu-max on a logarithmic scale, member 0 at nu = 0: the
inviscid flow the solver had before.  A loads recorder samples the pressure force on the peg after every step on the stream;
the host waits once, at the end, and writes nu, the Reynolds number speed * diameter / nu, and the mean drag and the lift's
swing over the second half of the run as CSV.  It is the PRESSURE drag: the loads have no viscous part.  Needs a GPU: there is
no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--speed", type=float, default=20.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--nu-min", type=float, default=1e-2)
    ap.add_argument("--nu-max", type=float, default=1e2)
    ap.add_argument("--out", default="reynolds.csv")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y, B = 96, 64, args.members
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    radius = dim_y // 8
    peg = (i - dim_x // 4) ** 2 + (j - dim_y // 2 - 1) ** 2 <= radius ** 2   # (one cell off the axis: the wake sheds sooner)
    solid = peg.copy()
    solid[0:2, :] = solid[-2:, :] = True                 # the channel's walls
    labels = np.where(peg, 1, 0).astype(np.uint8)        # ... which are in no body
    nu = np.concatenate([[0.0], np.geomspace(args.nu_min, args.nu_max, B - 1)]).astype(np.float32)
    with sfl.BatchSolver(dim_x, dim_y, B) as b:
        v = np.zeros((B, dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the channel starts in motion
        b.upload(cap.FIELD_VELOCITY, v)
        b.set_solids(solid)
        b.set_bodies(labels, 1)
        b.set_viscosity(nu, args.sweeps)
        column = [(i_at, row) for i_at in (2, dim_x - 3) for row in range(2, dim_y - 2)]
        members = [m for m in range(B) for _ in column]
        for step in range(args.steps):   # the inflow and the outflow column of every member, on the timeline
            b.queue_forces(members, column * B, [(args.speed, 0.0)] * len(members), step=step)
        b.loads_start(1, args.steps)
        b.step_n_each(args.steps, dt, dx, args.iters, omega)   # asynchronous: one launch and one sample per step
        xy = b.loads_history_xy()[:, :, 0] * dx                # the one wait: [steps, B, 2]
    half = args.steps // 2
    with open(args.out, "w") as f:
        f.write("member,nu,reynolds,mean_drag,lift_min,lift_max\n")
        for m in range(B):
            re = args.speed * 2 * radius * dx / nu[m] if nu[m] > 0 else float("inf")
            f.write(f"{m},{nu[m]:.6g},{re:.6g},{xy[half:, m, 0].mean():.9g},{xy[half:, m, 1].min():.9g},{xy[half:, m, 1].max():.9g}\n")
    print(f"{B} members of {dim_x} x {dim_y}, a peg of radius {radius}, nu from {nu[1]:.3g} to {nu[-1]:.3g} and member 0 inviscid; "
          f"mean drag from {xy[half:, :, 0].mean(axis=0).min():.6g} to {xy[half:, :, 0].mean(axis=0).max():.6g}; wrote {B} rows to {args.out}")


if __name__ == "__main__":
    main()
