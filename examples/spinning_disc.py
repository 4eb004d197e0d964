#!/usr/bin/env python3
"""A spinning disc in the wind tunnel: lift, torque and relative friction against the spin, one batch, omega per member.

    python examples/spinning_disc.py --members 9 --steps 600 --out spinning_disc.csv

Every member is the same 96 x 64 tunnel -- the west column an inflow, the east column an outflow (include/sfl.h "OPENINGS") --
with the same disc (a shared mask, body 1, its pivot at its centre).  The members differ in the disc's angular velocity alone:
a wall table per member (include/sfl.h "WALL VELOCITIES"; rigid_wall_velocity), from -omega-max to +omega-max, the middle
member at rest.  With openings set there is no viscosity, so the spin acts through the next step's advection alone, which
interpolates the stored field across the disc's rim: a thin layer is carried round, and the disc lifts (the Magnus effect).
The loads and the torque recorders run behind every step, and the friction is queried once, behind the last step; the CSV
holds, per member, the means over the second half of the recorded figures and that one query:

    drag, lift          fx, fy of the loads * dx
    torque              the pressure torque about the disc's centre * dx^2
    slip_x, slip_y      the friction sums of the fluid's velocity RELATIVE to the moving wall (friction_xy(nu=1, relative=True)
                        behind the last step, no mean): what a viscosity would multiply

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
    ap.add_argument("--members", type=int, default=9)
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--speed", type=float, default=20.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--omega-max", type=float, default=4.0, help="largest angular velocity, radians per time unit")
    ap.add_argument("--out", default="spinning_disc.csv")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y, B = 96, 64, args.members
    dt, dx, omega_sor = 1 / 30.0, 1.0, 1.9
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    cx, cy, radius = dim_x // 4, dim_y // 2, dim_y // 8
    disc = (i - cx) ** 2 + (j - cy) ** 2 <= radius ** 2
    labels = disc.astype(np.uint8)
    tunnel = np.zeros((dim_y, dim_x), np.uint8)
    tunnel[1:-1, 0], tunnel[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW
    spin = np.linspace(-args.omega_max, args.omega_max, B)
    who, cells, vel = [], [], []
    for m in range(B):   # one table, a row per member: the same cells, another spin
        c, w = sfl.rigid_wall_velocity(labels, 1, omega=spin[m], pivot2=(2 * cx, 2 * cy))
        who.append(np.full(len(c), m)), cells.append(c), vel.append(w)
    with sfl.BatchSolver(dim_x, dim_y, B) as b:
        v = np.zeros((B, dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the tunnel starts in motion
        b.upload(cap.FIELD_VELOCITY, v)
        b.set_solids(disc)
        b.set_bodies(labels, 1)
        b.set_body_pivots([(cx, cy)])
        b.set_openings(tunnel, (args.speed, 0.0))
        b.set_wall_velocity(np.concatenate(cells), np.concatenate(vel), np.concatenate(who))
        b.loads_start(1, args.steps)
        b.torque_start(1, args.steps)
        b.step_n(args.steps, dt, dx, args.iters, omega_sor)   # asynchronous: one launch and two samples per step
        loads = b.loads_history_xy() * dx                     # the one wait: [steps, B, 1, 2]
        torque = b.torque_history_xy(dx)[..., 0]              # the pressure torque: [steps, B, 1]
        slip = b.friction_xy(nu=1.0, relative=True)[:, 0]     # [B, 2]
    half = args.steps // 2
    drag, lift, moment = loads[half:, :, 0, 0].mean(axis=0), loads[half:, :, 0, 1].mean(axis=0), torque[half:, :, 0].mean(axis=0)
    with open(args.out, "w") as f:
        f.write("member,omega,rim_speed_over_inflow,drag,lift,torque,slip_x,slip_y\n")
        for m in range(B):
            f.write(f"{m},{spin[m]:.6g},{spin[m] * radius / args.speed:.6g},{drag[m]:.9g},{lift[m]:.9g},{moment[m]:.9g},{slip[m, 0]:.9g},{slip[m, 1]:.9g}\n")
    print(f"{B} members of {dim_x} x {dim_y}, a disc of radius {radius} spinning at {spin[0]:.3g} .. {spin[-1]:.3g}; lift from {lift.min():.4g} to "
          f"{lift.max():.4g}; wrote {B} rows to {args.out}")


if __name__ == "__main__":
    main()
