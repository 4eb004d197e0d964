#!/usr/bin/env python3
"""Drag and lift of the wind tunnel's disc, per step, from ONE step_n call: the loads recorder (sfl_loads_start).

    python examples/drag_curve.py --steps 400 --out drag.csv

The channel of examples/wind_tunnel.py: 512 x 256 along i, a disc of radius dim_y / 8 a quarter of the way down it, an inflow
and an outflow column of point forces queued once on the timeline.  Channel walls two cells thick line the long sides; they
are labelled 0 -- in no body -- and the disc is body 1, so the walls stay out of the drag.  The recorder samples the pressure
load after every step on the stream; the host waits once, at the end, and writes step, drag (fx), lift (fy) -- in pressure
times cell widths times dx -- and the face counts as CSV.  The oscillation of the lift is the vortex shedding.  Needs a GPU:
there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 256], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--speed", type=float, default=40.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--out", default="drag.csv")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y = args.size
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    disc = (i - dim_x // 4) ** 2 + (j - dim_y // 2 - 1) ** 2 <= (dim_y // 8) ** 2   # (one cell off the axis: the wake sheds sooner)
    solid = disc.copy()
    solid[0:2, :] = solid[-2:, :] = True                 # the channel's walls
    labels = np.where(disc, 1, 0).astype(np.uint8)       # ... which are in no body
    with sfl.Solver(dim_x, dim_y) as s:
        v = np.zeros((dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the channel starts in motion
        s.upload(cap.FIELD_VELOCITY, v)
        s.set_solids(solid)
        s.set_bodies(labels, 1)
        column = [(i_at, row) for i_at in (2, dim_x - 3) for row in range(2, dim_y - 2)]
        for step in range(args.steps):   # the inflow and the outflow column, on the timeline
            s.queue_forces(column, [(args.speed, 0.0)] * len(column), step=step)
        s.loads_start(1, args.steps)
        s.step_n(args.steps, dt, dx, args.iters, omega)   # asynchronous: a sample behind every step, on the stream
        rec = s.loads_history()[:, 0, 0]                  # the one wait
        xy = s.loads_history_xy()[:, 0, 0] * dx
    with open(args.out, "w") as f:
        f.write("step,drag,lift,max_abs_p,faces_w,faces_e,faces_s,faces_n,nonfinite\n")
        for k, (r, (fx, fy)) in enumerate(zip(rec, xy)):
            f.write(f"{k + 1},{fx:.9g},{fy:.9g},{r['max_abs_p']:.6g},{','.join(str(n) for n in r['faces'])},{r['nonfinite']}\n")
    half = len(xy) // 2
    print(f"{dim_x} x {dim_y}, frontal area {rec[0]['faces'][0]} faces; mean drag over the second half {xy[half:, 0].mean():.6g}, "
          f"lift between {xy[half:, 1].min():.6g} and {xy[half:, 1].max():.6g}; wrote {len(xy)} rows to {args.out}")


if __name__ == "__main__":
    main()
