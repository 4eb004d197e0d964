#!/usr/bin/env python3
"""The time-averaged wake of a disc: the averages of a whole-domain context (sfl_mean_start), from ONE step_n call.

    python examples/mean_wake.py --steps 600 --skip 200 --out mean_wake

The set-up is the closed tunnel of examples/wind_tunnel.py -- a 512 x 256 box driven by an inflow and an outflow column of
point forces queued on the timeline, a disc of radius dim_y / 8 a quarter of the way down -- with a viscosity (--nu): an open
rim (sfl_set_openings) would be the better tunnel, but the library refuses openings and viscosity together, and the wake of a
study is read at a Reynolds number.  The first --skip steps run without averages, so that the start-up does not weigh on the
means; then the averages are started with every = 1 and the rest of the run is ONE asynchronous step_n call: a sample of the
mean velocity and of the second moments behind every step, on the stream, no download in between.

Written to --out: mean_speed.pgm and tke.pgm (8-bit, the channel lying flat, scaled to their maxima), mean_u_centreline.csv
(i, mean u on the row through the disc's centre) and, printed, the recirculation length: the distance from the disc's rear to
the cell on the centreline behind it where the mean u turns positive again.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_pgm(path, a):
    """A float field as an 8-bit PGM scaled to its maximum, rows along i."""
    top = float(np.nanmax(a)) if a.size and np.isfinite(np.nanmax(a)) and np.nanmax(a) > 0 else 1.0
    img = np.clip(np.nan_to_num(a) / top * 255.0, 0, 255).astype(np.uint8)[::-1]
    with open(path, "wb") as out:
        out.write(b"P5 %d %d 255\n" % (img.shape[1], img.shape[0]))
        out.write(img.tobytes())
    return top


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[512, 256], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--steps", type=int, default=600)
    ap.add_argument("--skip", type=int, default=200, help="steps in front of the averages")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--speed", type=float, default=40.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--nu", type=float, default=0.5, help="viscosity; 0: none")
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--out", default="mean_wake")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y = args.size
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    cx, cy, radius = dim_x // 4, dim_y // 2 + 1, dim_y // 8   # (one cell off the axis: the wake sheds sooner)
    disc = (i - cx) ** 2 + (j - cy) ** 2 <= radius ** 2
    os.makedirs(args.out, exist_ok=True)
    with sfl.Solver(dim_x, dim_y) as s:
        v = np.zeros((dim_y, dim_x, 2), np.float32)
        v[..., 0] = args.speed   # the channel starts in motion
        s.upload(cap.FIELD_VELOCITY, v)
        s.set_solids(disc)
        if args.nu > 0:
            s.set_viscosity(args.nu, args.sweeps)
        column = [(i_at, row) for i_at in (2, dim_x - 3) for row in range(1, dim_y - 1)]
        for step in range(args.steps):   # the inflow and the outflow column, on the timeline
            s.queue_forces(column, [(args.speed, 0.0)] * len(column), step=step)
        s.step_n(args.skip, dt, dx, args.iters, omega)
        s.mean_start(sfl.MEAN_VELOCITY | sfl.MEAN_STRESS, 1)
        s.step_n(args.steps - args.skip, dt, dx, args.iters, omega)   # ONE call: a sample behind every step, on the stream
        what, every, samples, steps = s.mean_info()
        m, rs = s.means(), s.reynolds_stress()
        s.mean_stop()
    u, w = m["U"][0], m["V"][0]
    speed, tke = np.hypot(u, w), rs["tke"][0]
    speed[disc], tke[disc] = 0.0, 0.0
    top_speed, top_tke = write_pgm(os.path.join(args.out, "mean_speed.pgm"), speed), write_pgm(os.path.join(args.out, "tke.pgm"), tke)
    line = u[cy]
    with open(os.path.join(args.out, "mean_u_centreline.csv"), "w") as f:
        f.write("i,mean_u\n" + "".join(f"{k},{line[k]:.9g}\n" for k in range(dim_x)))
    rear = cx + radius + 1   # the first fluid cell behind the disc on its centre row
    behind = line[rear:dim_x - 3]
    back = np.nonzero(behind < 0)[0]
    if len(back) and back[0] < 4:
        ahead = np.nonzero(behind[back[0]:] >= 0)[0]
        length = f"{back[0] + ahead[0]} cells ({(back[0] + ahead[0]) / (2.0 * radius):.2f} diameters)" if len(ahead) else "reaches the outflow column"
    else:
        length = "none: the mean u behind the disc is nowhere negative"
    print(f"{dim_x} x {dim_y}, nu {args.nu}, Re = U D / nu = {args.speed * 2 * radius / args.nu if args.nu > 0 else float('inf'):.0f}; "
          f"{samples} samples behind {steps} steps (mask {what}, every {every})")
    print(f"mean speed up to {top_speed:.4g}, turbulent kinetic energy up to {top_tke:.4g}; recirculation length: {length}")
    print(f"wrote mean_speed.pgm, tke.pgm and mean_u_centreline.csv to {args.out}")


if __name__ == "__main__":
    main()
