#!/usr/bin/env python3
"""Drag, lift, pitching moment and centre of pressure of a flat plate against its angle of attack: one batch, a mask per member,
ONE step_n call.

    python examples/plate_moment.py --members 16 --steps 300 --out plate_moment.csv

Every member is the same 96 x 64 channel with the same inflow; the members differ in the angle of their plate alone (masks per
member), from --angle-min to --angle-max degrees, nose down positive (the flow comes from the west).  A plate is a rasterised
line of --chord cells, one cell thick, turned about its middle; its pivot is the QUARTER CHORD point, rounded to half a cell
(sfl_batch_set_body_pivots, per member).  The loads, the friction and the torque recorders are on: after every step each
samples the plate on the stream; the host waits once, at the end.  The CSV holds, per member, the means over the second half of
the run of

    drag, lift          pressure force * dx + nu * friction force           (include/sfl.h "LOADS", "FRICTION")
    moment              pressure torque * dx^2 + nu * friction torque * dx, about the quarter chord, counter-clockwise ("TORQUE")
    centre_of_pressure  the point ON THE CHORD LINE about which the moment vanishes, as a fraction of the chord from the leading
                        edge: x_cp = 1/4 + moment / (normal force * chord), by the header's identity -- moving the pivot by r
                        changes the moment by -(r x F) -- and so from the three records without a second sample

all per unit depth and density.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def plate(dim_x, dim_y, cx, cy, chord, degrees):
    """(mask, leading edge, unit vector along the chord): cells within half a cell of the segment."""
    a = np.radians(degrees)
    along = np.array([np.cos(a), -np.sin(a)])   # nose down positive: the trailing edge lies lower
    lead = np.array([cx, cy], float) - 0.5 * chord * along
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    rel = np.stack([i - lead[0], j - lead[1]], axis=-1)
    s = rel @ along
    d = np.abs(rel @ np.array([-along[1], along[0]]))
    return (s >= 0) & (s <= chord) & (d <= 0.5), lead, along


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--members", type=int, default=16)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--nu", type=float, default=0.5)
    ap.add_argument("--speed", type=float, default=20.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--chord", type=int, default=24)
    ap.add_argument("--angle-min", type=float, default=0.0)
    ap.add_argument("--angle-max", type=float, default=30.0)
    ap.add_argument("--out", default="plate_moment.csv")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y, B = 96, 64, args.members
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    angles = np.linspace(args.angle_min, args.angle_max, B)
    solid = np.zeros((B, dim_y, dim_x), bool)
    labels = np.zeros((B, dim_y, dim_x), np.uint8)
    pivots = np.zeros((B, 1, 2))
    alongs = np.zeros((B, 2))
    for m, angle in enumerate(angles):
        mask, lead, along = plate(dim_x, dim_y, dim_x // 3, dim_y // 2, args.chord, angle)
        labels[m][mask] = 1                      # the channel's walls are in no body
        solid[m] = mask
        pivots[m, 0] = np.round((lead + 0.25 * args.chord * along) * 2) / 2   # the quarter chord, in half cells
        alongs[m] = along
    solid[:, 0:2, :] = solid[:, -2:, :] = True
    with sfl.BatchSolver(dim_x, dim_y, B) as b:
        v = np.zeros((B, dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the channel starts in motion
        b.upload(cap.FIELD_VELOCITY, v)
        b.set_solids(solid)
        b.set_bodies(labels, 1)
        b.set_body_pivots(pivots)
        b.set_viscosity(args.nu, args.sweeps)
        column = [(i_at, row) for i_at in (2, dim_x - 3) for row in range(2, dim_y - 2)]
        members = [m for m in range(B) for _ in column]
        for step in range(args.steps):   # the inflow and the outflow column of every member, on the timeline
            b.queue_forces(members, column * B, [(args.speed, 0.0)] * len(members), step=step)
        b.loads_start(1, args.steps)
        b.friction_start(1, args.steps)
        b.torque_start(1, args.steps)
        b.step_n(args.steps, dt, dx, args.iters, omega)        # asynchronous: one launch and three samples per step
        force = b.loads_history_xy()[:, :, 0] * dx + b.friction_history_xy()[:, :, 0]   # the one wait: [steps, B, 2]
        moment = b.torque_history_xy(dx=dx).sum(axis=-1)[:, :, 0]                       # pressure + friction: [steps, B]
        held = b.body_pivots()[:, 0]
    half = args.steps // 2
    f_mean, m_mean = force[half:].mean(axis=0), moment[half:].mean(axis=0)
    normal = f_mean[:, 1] * alongs[:, 0] - f_mean[:, 0] * alongs[:, 1]   # the force across the chord: along x F
    with np.errstate(divide="ignore", invalid="ignore"):
        x_cp = 0.25 + m_mean / (normal * args.chord * dx)   # (moving the pivot by r along the chord changes the moment by -r * normal)
    with open(args.out, "w") as f:
        f.write("member,angle_deg,pivot_x,pivot_y,drag,lift,moment,centre_of_pressure\n")
        for m in range(B):
            f.write(f"{m},{angles[m]:.6g},{held[m, 0]:.6g},{held[m, 1]:.6g},{f_mean[m, 0]:.9g},{f_mean[m, 1]:.9g},{m_mean[m]:.9g},{x_cp[m]:.6g}\n")
    print(f"{B} members of {dim_x} x {dim_y}, a plate of {args.chord} cells at {angles[0]:.3g} to {angles[-1]:.3g} degrees, nu = {args.nu:g}; "
          f"lift from {f_mean[:, 1].min():.4g} to {f_mean[:, 1].max():.4g}, moment about the quarter chord from {m_mean.min():.4g} to "
          f"{m_mean.max():.4g}; wrote {B} rows to {args.out}")


if __name__ == "__main__":
    main()
