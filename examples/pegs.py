#!/usr/bin/env python3
"""Something in the way of the fluid: one batch whose members differ in their obstacle only.

    python examples/pegs.py --steps 120 --every 20 --out pegs

Every member is the sketch's 61 x 81 grid and gets the same drag: one finger drawn upwards through the middle of the lower
half, queued on the timeline before the first step.  What differs is the mask of solid cells (sfl_batch_set_solids, one mask
per member): no obstacle, pegs of growing radius, a plate across the finger's path, and a wall with a slit.  The obstacles
are painted into the dye, which a solid cell keeps.  Two batches hold the same members and get the same calls; the recorder of
one draws the dye, the recorder of the other the vorticity (which reads the zero velocity of solid cells through its
ordinary stencil).  Written: a contact sheet per frame as PPM -- every member's vorticity image with its dye image to the
right of it -- and flow_stats.csv, one line per frame and member: max |v.x|, max |v.y|, the remaining divergence by the
solids' rule and the dye totals.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_movie import DT, OMEGA   # noqa: E402
from vorticity_movie import write_sheets   # noqa: E402


def obstacles(dim_x, dim_y):
    """name -> mask[dim_y, dim_x]: the members of the batch."""
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    cx, cy = dim_x // 2, dim_y // 2
    out = {"none": np.zeros((dim_y, dim_x), bool)}
    for r in (2, 4, 7, 10):
        out[f"peg r={r}"] = (i - cx) ** 2 + (j - cy) ** 2 <= r * r
    plate = np.zeros((dim_y, dim_x), bool)
    plate[cy, cx - dim_x // 4:cx + dim_x // 4 + 1] = True
    out["plate"] = plate
    slit = np.zeros((dim_y, dim_x), bool)
    slit[cy - 1:cy + 1, :] = True
    slit[cy - 1:cy + 1, cx - 2:cx + 3] = False
    out["slit"] = slit
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=20)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scaling", type=int, default=4)
    ap.add_argument("--columns", type=int, default=4, help="(vorticity | dye) pairs per row of a contact sheet")
    ap.add_argument("--out", default="pegs")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    dim_x, dim_y = args.size
    masks = obstacles(dim_x, dim_y)
    names, mask = list(masks), np.stack(list(masks.values()))
    batch = len(names)
    view = sfl.View(cap.VIEW_VORTICITY, -20.0, 20.0, sfl.PALETTE_BLUE_WHITE_RED)
    os.makedirs(args.out, exist_ok=True)
    frames = args.steps // args.every
    rows = ["frame,step,member,obstacle,max_abs_vx,max_abs_vy,max_abs_div,dye_r,dye_g,dye_b"]
    with sfl.BatchSolver(dim_x, dim_y, batch) as flow, sfl.BatchSolver(dim_x, dim_y, batch) as dye:
        for b in (flow, dye):
            b.setup_sketch_fields()
            colour = b.download(cap.FIELD_COLOR)
            colour[mask] = (cap.VIEW_MAX_COLOUR, cap.VIEW_MAX_COLOUR, 0)   # the obstacles, painted: a solid cell keeps its dye
            b.upload(cap.FIELD_COLOR, colour)
            b.set_solids(mask)
            for step in range(min(args.steps, dim_y // 3)):   # the finger: one cell per step, upwards from the lower quarter
                b.queue_forces(list(range(batch)), [(dim_x // 2, dim_y // 8 + step)] * batch, [(0.0, 30.0)] * batch, step=step)
            b.record_start(every=args.every, scaling=args.scaling, byteswap=False, capacity=max(frames, 1))
        flow.record_view(view)
        for f in range(frames):   # cut at the frames: the statistics of the step a frame shows
            for b in (flow, dye):
                b.step_n(args.every, DT, 1.0, args.iters, OMEGA)
            for m, s in enumerate(dye.flow_stats(1.0)):
                rows.append(f"{f},{(f + 1) * args.every},{m},{names[m]},{s['max_abs_vx']:.6g},{s['max_abs_vy']:.6g},{s['max_abs_div']:.6g},"
                            + ",".join(str(int(x)) for x in s["dye_sum"]))
        written = write_sheets(flow.frames(), dye.frames(), 0, args.columns, args.out)
    with open(os.path.join(args.out, "flow_stats.csv"), "w") as f:
        f.write("\n".join(rows) + "\n")
    print(f"wrote {written} contact sheets of {batch} members (vorticity | dye) and flow_stats.csv to {args.out}: " + ", ".join(names))


if __name__ == "__main__":
    main()
