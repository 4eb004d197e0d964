#!/usr/bin/env python3
"""A disc in a channel: solid cells on a whole-domain context (sfl_set_solids), at a size no batch member has.

    python examples/wind_tunnel.py --steps 400 --every 20 --out tunnel

A 512 x 256 channel along i with a disc of radius dim_y / 8 a quarter of the way down it.  The grid is a closed box, so the
tunnel is driven from both ends: an inflow column of point forces at i = 2 and an outflow column at i = dim_x - 3 set the
velocity there to (speed, 0) on every step -- what enters leaves.  Both are queued ONCE, on the force timeline, for all
the steps to come, so the run is a handful of asynchronous step_n calls.  The disc is painted into the dye, which a solid cell
keeps, and three dye stripes enter with the flow.  Written: one vorticity frame (sfl_view_render: blue, white, red) per
`every` steps as PPM, and flow_stats.csv -- max |v.x|, max |v.y| and the remaining divergence by the solids' rule per
frame.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from demo_frames import rgb565_to_rgb888   # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 256], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--speed", type=float, default=40.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--scaling", type=int, default=2)
    ap.add_argument("--out", default="tunnel")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y = args.size
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    disc = (i - dim_x // 4) ** 2 + (j - dim_y // 2 - 1) ** 2 <= (dim_y // 8) ** 2   # (one cell off the axis: the wake sheds sooner)
    view = sfl.View(cap.VIEW_VORTICITY, -15.0, 15.0, sfl.PALETTE_BLUE_WHITE_RED, dx=dx)
    os.makedirs(args.out, exist_ok=True)
    rows = ["frame,step,max_abs_vx,max_abs_vy,max_abs_div"]
    with sfl.Solver(dim_x, dim_y) as s:
        v = np.zeros((dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the channel starts in motion
        colour = np.zeros((dim_y, dim_x, 3), np.uint32)
        colour[(j // (dim_y // 6)) % 2 == 0, 2] = cap.VIEW_MAX_COLOUR   # stripes, carried along
        colour[disc] = (cap.VIEW_MAX_COLOUR, cap.VIEW_MAX_COLOUR, 0)    # the obstacle, painted
        s.upload(cap.FIELD_VELOCITY, v)
        s.upload(cap.FIELD_COLOR, colour)
        s.set_solids(disc)
        print(f"{dim_x} x {dim_y}, {s.solids_info()[1]} solid cells")
        column = [(i_at, row) for i_at in (2, dim_x - 3) for row in range(1, dim_y - 1)]
        for step in range(args.steps):   # the inflow and the outflow column, on the timeline
            s.queue_forces(column, [(args.speed, 0.0)] * len(column), step=step)
        for f in range(args.steps // args.every):
            s.step_n(args.every, dt, dx, args.iters, omega)
            img = rgb565_to_rgb888(s.view_render(view, args.scaling, byteswap=False))
            img = np.ascontiguousarray(img.transpose(1, 0, 2)[::-1])   # rows of the image run along i: the channel lies flat
            with open(os.path.join(args.out, f"vorticity_{f:04d}.ppm"), "wb") as out:
                out.write(b"P6 %d %d 255\n" % (img.shape[1], img.shape[0]))
                out.write(img.tobytes())
            st = s.flow_stats(dx, dye=False)
            rows.append(f"{f},{(f + 1) * args.every},{st['max_abs_vx']:.6g},{st['max_abs_vy']:.6g},{st['max_abs_div']:.6g}")
    with open(os.path.join(args.out, "flow_stats.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"wrote {args.steps // args.every} vorticity frames and flow_stats.csv to {args.out}")


if __name__ == "__main__":
    main()
