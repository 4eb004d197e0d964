#!/usr/bin/env python3
"""The lid-driven cavity: one batch, nu per member, the lid a row of solid cells that moves (include/sfl.h "WALL VELOCITIES").

    python examples/lid_cavity.py --members 8 --steps 2000 --out lid_cavity

Every member is the same square cavity of --size cells whose top row is solid and is body 1; a wall table gives that row the
velocity (--speed, 0).  The members differ in nu alone (per member, from --nu-min to --nu-max on a logarithmic scale), so one
batch sweeps the Reynolds number Re = speed * size * dx / nu.  From rest the lid moves nothing by itself: the implicit diffusion
of the velocity (item 3a) reads the lid's cells as they are and drags the row beside them, and the next step's advection
interpolates the stored field, lid included.  The pressure sees a wall at rest.

Writes <out>_u.csv (u on the vertical centreline against y, one column per member), <out>_v.csv (v on the horizontal
centreline against x) and <out>_vorticity.npy (the vorticity sheet of every member, float32 [members, size, size], central
differences of the downloaded velocity).  Setting the profiles beside published cavity profiles (Ghia, Ghia and Shin 1982) is
a picture to look at, not a test: this solver is first order in time and its walls are cells, not faces.
Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=8)
    ap.add_argument("--size", type=int, default=64, help="cells per side, lid row included (at most 78: a member is at most 6144 cells)")
    ap.add_argument("--steps", type=int, default=2000)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--sweeps", type=int, default=6)
    ap.add_argument("--speed", type=float, default=10.0, help="the lid's velocity, cells per time unit")
    ap.add_argument("--nu-min", type=float, default=0.64)
    ap.add_argument("--nu-max", type=float, default=6.4)
    ap.add_argument("--out", default="lid_cavity")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    n, B = args.size, args.members
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    labels = np.zeros((n, n), np.uint8)
    labels[-1, :] = 1                                       # the lid: the top row, body 1
    nu = np.geomspace(args.nu_min, args.nu_max, B).astype(np.float32)
    with sfl.BatchSolver(n, n, B) as b:
        b.set_solids(labels > 0)
        b.set_bodies(labels, 1)
        b.set_viscosity(nu, args.sweeps)
        b.set_wall_velocity(*sfl.rigid_wall_velocity(labels, 1, u=args.speed))   # one table for all members
        b.step_n(args.steps, dt, dx, args.iters, omega)     # asynchronous: one launch per step
        v = b.download(cap.FIELD_VELOCITY)                  # the one wait: [B, n, n, 2]
        drag = b.friction_xy(relative=True)[:, 0, 0]        # what the fluid drags the lid with: relative to the moving wall
    y = (np.arange(n) + 0.5) / n
    header = "position," + ",".join(f"nu={x:.4g} (Re={args.speed * n * dx / x:.4g})" for x in nu)
    np.savetxt(f"{args.out}_u.csv", np.column_stack([y, (v[:, :, n // 2, 0] / args.speed).T]), delimiter=",", header=header, comments="")
    np.savetxt(f"{args.out}_v.csv", np.column_stack([y, (v[:, n // 2, :, 1] / args.speed).T]), delimiter=",", header=header, comments="")
    vorticity = np.zeros((B, n, n), np.float32)
    vorticity[:, 1:-1, 1:-1] = ((v[:, 1:-1, 2:, 1] - v[:, 1:-1, :-2, 1]) - (v[:, 2:, 1:-1, 0] - v[:, :-2, 1:-1, 0])) / (2 * dx)
    np.save(f"{args.out}_vorticity.npy", vorticity)
    print(f"{B} cavities of {n} x {n}, lid speed {args.speed}, Re from {args.speed * n * dx / nu[-1]:.3g} to {args.speed * n * dx / nu[0]:.3g}; "
          f"the lowest u on the centreline runs from {(v[:, :, n // 2, 0] / args.speed).min(axis=1).max():.3g} to "
          f"{(v[:, :, n // 2, 0] / args.speed).min(axis=1).min():.3g} of the lid's; drag on the lid {drag.min():.4g} .. {drag.max():.4g}; "
          f"wrote {args.out}_u.csv, {args.out}_v.csv, {args.out}_vorticity.npy")


if __name__ == "__main__":
    main()
