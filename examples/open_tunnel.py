#!/usr/bin/env python3
"""A wind tunnel with a real inlet and outlet: openings on the rim of a context's grid (sfl_set_openings).

    python examples/open_tunnel.py --steps 400 --out open_tunnel

examples/wind_tunnel.py drives a closed box from both ends with a column of point forces per step.  Here the west column of a
512 x 256 channel is an INFLOW and the east column an OUTFLOW (include/sfl.h "OPENINGS"): nothing is queued, the flow enters and
leaves through the rim, and a uniform stream is a fixed point of the step.  Channel walls two cells thick line the long sides;
they are labelled 0 -- in no body -- and a disc of radius dim_y / 8 a quarter of the way down the channel is body 1.

The loads recorder samples the pressure force on the disc after every step, on the stream; with --every 0 the whole run is ONE
step_n call and the host waits once, at the end.  With --every N a vorticity frame is rendered after every N steps (one step_n
call per frame; the recorder counts across calls).  Written: drag.csv (step, drag, lift, in pressure times cell widths times
dx) and the frames as PPM files.  Needs a GPU: there is no CPU fallback.
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
    ap.add_argument("--speed", type=float, default=40.0, help="inflow velocity, cells per time unit")
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--every", type=int, default=20, help="a vorticity frame after every so many steps; 0: none, one step_n call")
    ap.add_argument("--iters", type=int, default=40)
    ap.add_argument("--scaling", type=int, default=2)
    ap.add_argument("--out", default="open_tunnel")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y = args.size
    dt, dx, omega = 1 / 30.0, 1.0, 1.9
    os.makedirs(args.out, exist_ok=True)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    disc = (i - dim_x // 4) ** 2 + (j - dim_y // 2 - 1) ** 2 <= (dim_y // 8) ** 2   # (one cell off the axis: the wake sheds sooner)
    solid = disc.copy()
    solid[0:2, :] = solid[-2:, :] = True                 # the channel's walls
    labels = np.where(disc, 1, 0).astype(np.uint8)       # ... which are in no body
    tunnel = np.zeros((dim_y, dim_x), np.uint8)
    tunnel[1:-1, 0], tunnel[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW   # (on the walls' cells the openings do not count)
    view = sfl.View(cap.VIEW_VORTICITY, -15.0, 15.0, sfl.PALETTE_BLUE_WHITE_RED, dx=dx)
    frames = 0
    with sfl.Solver(dim_x, dim_y) as s:
        v = np.zeros((dim_y, dim_x, 2), np.float32)
        v[~solid, 0] = args.speed                        # the channel starts in motion
        s.upload(cap.FIELD_VELOCITY, v)
        s.set_solids(solid)
        s.set_bodies(labels, 1)
        s.set_openings(tunnel, (args.speed, 0.0))
        _, live_in, live_out = s.openings_info()
        s.loads_start(1, args.steps)
        if args.every <= 0:
            s.step_n(args.steps, dt, dx, args.iters, omega)   # asynchronous: a sample behind every step, on the stream
        else:
            for done in range(0, args.steps, args.every):
                s.step_n(min(args.every, args.steps - done), dt, dx, args.iters, omega)
                img = rgb565_to_rgb888(s.view_render(view, args.scaling, byteswap=False))
                with open(os.path.join(args.out, f"vorticity_{frames:04d}.ppm"), "wb") as out:
                    out.write(b"P6 %d %d 255\n" % (img.shape[1], img.shape[0]))
                    out.write(img.tobytes())
                frames += 1
        rec = s.loads_history()[:, 0, 0]
        xy = s.loads_history_xy()[:, 0, 0] * dx
        left = s.flow_stats(dx, dye=False)["max_abs_div"]
    with open(os.path.join(args.out, "drag.csv"), "w") as f:
        f.write("step,drag,lift,max_abs_p,faces_w,faces_e,faces_s,faces_n,nonfinite\n")
        for k, (r, (fx, fy)) in enumerate(zip(rec, xy)):
            f.write(f"{k + 1},{fx:.9g},{fy:.9g},{r['max_abs_p']:.6g},{','.join(str(n) for n in r['faces'])},{r['nonfinite']}\n")
    half = len(xy) // 2
    print(f"{dim_x} x {dim_y}, {live_in} live inflow and {live_out} live outflow cells, frontal area {rec[0]['faces'][0]} faces")
    print(f"mean drag over the second half {xy[half:, 0].mean():.6g}, lift between {xy[half:, 1].min():.6g} and {xy[half:, 1].max():.6g}, "
          f"max |div| left {left:.3g}")
    print(f"wrote {len(xy)} rows to {args.out}/drag.csv and {frames} vorticity frames")


if __name__ == "__main__":
    main()
