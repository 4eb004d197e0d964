#!/usr/bin/env python3
"""What do more SOR iterations buy?  The sketch's start plus a few drags on a whole-domain context, stepped twice -- once
per value of --iters -- with the flow reported after every step WITHOUT downloading a field:

    python examples/flow_report.py [--size 61 81] [--steps 8] [--iters 10 80] [--omega 1.9] [--dt 0.05]

Per step, from one sfl_flow_stats call (two streaming passes over the velocity and the dye):
  max |div|     the largest |calculate_divergence(v)| of the velocity the projection left: what the iterations are spent for;
  max |v.x|, max |v.y|   times dt the longest back-trace of the next advection, in cells;
  dye sums      the exact total of every dye channel: semi-Lagrangian advection does not conserve it.

Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--iters", type=int, nargs="+", default=[10, 80])
    ap.add_argument("--omega", type=float, default=1.9)
    ap.add_argument("--dt", type=float, default=0.05)
    args = ap.parse_args()
    dim_x, dim_y = args.size
    # drags in the sketch's graphics coordinates (struct drag, ino:45-48): across the middle of the screen
    drags = [(dim_y // 2 + k, dim_x // 2, 40.0, 15.0 * (k - 1)) for k in range(3)]
    for iters in args.iters:
        with sfl.Solver(dim_x, dim_y) as s:
            s.setup_sketch_fields()
            start = s.flow_stats(velocity=False)["dye_sum"]
            print(f"{dim_x} x {dim_y}, {iters} iterations per step, omega {args.omega}, dt {args.dt}")
            print("step     max |div|     max |v.x|     max |v.y|   back-trace (cells)   dye kept (r, g, b)")
            for step in range(1, args.steps + 1):
                if step <= 3:
                    s.queue_drags(drags)
                s.step(args.dt, 1.0, iters, args.omega)
                r = s.flow_stats(1.0)
                reach = max(abs(r["max_abs_vx"] * args.dt), abs(r["max_abs_vy"] * args.dt))
                kept = "  ".join(f"{int(now) / max(int(was), 1):.6f}" for now, was in zip(r["dye_sum"], start))
                print(f"{step:4d}  {r['max_abs_div']:12.5e}  {r['max_abs_vx']:12.5e}  {r['max_abs_vy']:12.5e}  {reach:12.4f}          {kept}")
            print()
