#!/usr/bin/env python3
"""The flow beside its dye: B sketches stepped as one batch, recorded twice -- once drawn by vorticity, once by the dye.

    python examples/vorticity_movie.py --batch 8 --steps 120 --every 10 --out sheets

Every member starts from the sketch's fields and is stirred by a finger of its own (the strokes of examples/batch_movie.py,
queued on the timeline before the first step).  Two batches hold the same members and get the same calls; the recorder of
one draws the vorticity (sfl_batch_record_view with a blue-white-red palette: clockwise blue, counter-clockwise red, no
rotation white), the recorder of the other the dye.  Both render on the device between the step launches.  A contact sheet
per frame is written as PPM: every member's vorticity image with its dye image to the right of it.  With --view speed,
pressure or divergence the left images show that scalar instead.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_movie import DT, OMEGA, rgb565_to_rgb888, stroke   # noqa: E402


def write_sheets(views, dyes, number, columns, out):
    """One PPM per frame: pairs (view | dye) of the members in rows of `columns` pairs."""
    for view, dye in zip(views, dyes):
        count, h, w = view.shape
        rows = (count + columns - 1) // columns
        sheet = np.zeros((rows * h, columns * 2 * w, 3), np.uint8)
        for k in range(count):
            r, c = divmod(k, columns)
            sheet[r * h:(r + 1) * h, 2 * c * w:(2 * c + 1) * w] = rgb565_to_rgb888(view[k])
            sheet[r * h:(r + 1) * h, (2 * c + 1) * w:(2 * c + 2) * w] = rgb565_to_rgb888(dye[k])
        with open(os.path.join(out, f"sheet_{number:05d}.ppm"), "wb") as f:
            f.write(b"P6 %d %d 255\n" % (sheet.shape[1], sheet.shape[0]))
            f.write(sheet.tobytes())
        number += 1
    return number


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scaling", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=8, help="frames a recorder holds before they are read out")
    ap.add_argument("--columns", type=int, default=2, help="(view | dye) pairs per row of a contact sheet")
    ap.add_argument("--view", choices=["vorticity", "speed", "pressure", "divergence"], default="vorticity")
    ap.add_argument("--range", type=float, default=None, help="the scalar that reaches the palette's last stop (default: by the view)")
    ap.add_argument("--large", action="store_true", help="batches of large members (up to 20224 cells)")
    ap.add_argument("--out", default="sheets")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    cap = sfl.capi
    top = {"vorticity": 20.0, "speed": 40.0, "pressure": 10.0, "divergence": 0.5}[args.view] if args.range is None else args.range
    view = {"vorticity": sfl.View(cap.VIEW_VORTICITY, -top, top, sfl.PALETTE_BLUE_WHITE_RED),
            "speed": sfl.View(cap.VIEW_SPEED, 0.0, top, sfl.PALETTE_HEAT),
            "pressure": sfl.View(cap.VIEW_PRESSURE, -top, top, sfl.PALETTE_BLUE_WHITE_RED),
            "divergence": sfl.View(cap.VIEW_DIVERGENCE, -top, top, sfl.PALETTE_BLUE_WHITE_RED)}[args.view]
    dim_x, dim_y = args.size
    os.makedirs(args.out, exist_ok=True)
    written = 0
    with sfl.BatchSolver(dim_x, dim_y, args.batch, large=args.large) as flow, \
            sfl.BatchSolver(dim_x, dim_y, args.batch, large=args.large) as dye:
        for b in (flow, dye):
            b.setup_sketch_fields()
            for step in range(args.steps):   # the whole stroke, before the first step
                b.queue_forces(*stroke(step, args.batch, dim_x, dim_y), step=step)
        fill = args.every * args.capacity   # steps that fill a recorder
        for first in range(0, args.steps, fill):
            for b in (flow, dye):
                b.record_start(every=args.every, scaling=args.scaling, byteswap=False, capacity=args.capacity)
            flow.record_view(view)   # (record_start resets to the dye: say it again after every restart)
            for b in (flow, dye):    # asynchronous: both batches step and render before either is read
                b.step_n(min(fill, args.steps - first), DT, 1.0, args.iters, OMEGA)
            written = write_sheets(flow.frames(), dye.frames(), written, args.columns, args.out)
        peak = float(np.nanmax(np.abs(flow.view_scalar(view.what))))
    print(f"wrote {written} contact sheets of {args.batch} members ({args.view} | dye) to {args.out}; "
          f"the last |{args.view}| peaks at {peak:.3g}, the palette ends at {top:.3g}")


if __name__ == "__main__":
    main()
