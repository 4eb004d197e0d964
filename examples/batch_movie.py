#!/usr/bin/env python3
"""An ensemble of movies: B sketches stepped as one batch, each with a finger drag of its own, recorded while they step.

    python examples/batch_movie.py --batch 16 --steps 120 --every 10 --out sheets

Every member starts from the sketch's fields (setup(), ino:196-241: sfl_batch_setup_sketch_fields).  Member m's finger
moves round a circle of its own radius and speed.  The whole stroke is queued before the first step -- queue_forces with
step=k for the records of step k (ino:264-269; the timeline of include/sfl.h) -- and ONE step_n call then runs as many
steps as fill the recorder (sfl_batch_record_start): after every `--every`-th step a frame of every member is rendered on
the device, between the step launches, and the host never waits for one.  When the recorder is full, and at the end,
the frames are read out (sfl_batch_record_read) and written as PPM contact sheets: one sheet per frame, the members side
by side.  Needs a GPU: there is no CPU fallback.
"""
import argparse
import importlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DT, OMEGA = np.float32(1 / 30.0), np.float32(1.96)


def rgb565_to_rgb888(img):
    r = ((img >> 11) & 0x1F).astype(np.uint8) << 3
    g = ((img >> 5) & 0x3F).astype(np.uint8) << 2
    b = (img & 0x1F).astype(np.uint8) << 3
    return np.stack([r, g, b], axis=-1)


def stroke(step, batch, dim_x, dim_y):
    """The finger of every member at this step: (members, cells, velocities) for queue_forces."""
    members, cells, vel = [], [], []
    for m in range(batch):
        radius = (0.15 + 0.25 * m / max(batch - 1, 1)) * min(dim_x, dim_y)
        speed = (0.08 + 0.12 * ((m * 7) % batch) / batch) * min(dim_x, dim_y) * 30
        a = 2 * math.pi * step / 90 * (1 if m % 2 == 0 else -1)
        ci, cj = int(dim_x / 2 + radius * math.cos(a)), int(dim_y / 2 + radius * math.sin(a))
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                members.append(m)
                cells.append((ci + di, cj + dj))
                vel.append((-speed * math.sin(a), speed * math.cos(a)))
    return members, cells, vel


def write_sheets(frames, number, columns, out):
    """One PPM per frame: the members' images in rows of `columns`."""
    for frame in frames:
        count, h, w = frame.shape
        rows = (count + columns - 1) // columns
        sheet = np.zeros((rows * h, columns * w, 3), np.uint8)
        for k in range(count):
            r, c = divmod(k, columns)
            sheet[r * h:(r + 1) * h, c * w:(c + 1) * w] = rgb565_to_rgb888(frame[k])
        with open(os.path.join(out, f"sheet_{number:05d}.ppm"), "wb") as f:
            f.write(b"P6 %d %d 255\n" % (sheet.shape[1], sheet.shape[0]))
            f.write(sheet.tobytes())
        number += 1
    return number


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--every", type=int, default=10)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scaling", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=8, help="frames the recorder holds before they are read out")
    ap.add_argument("--columns", type=int, default=4, help="members per row of a contact sheet")
    ap.add_argument("--large", action="store_true", help="a batch of large members (up to 20224 cells)")
    ap.add_argument("--out", default="sheets")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    dim_x, dim_y = args.size
    os.makedirs(args.out, exist_ok=True)
    written = 0
    with sfl.BatchSolver(dim_x, dim_y, args.batch, large=args.large) as b:
        b.setup_sketch_fields()
        for step in range(args.steps):   # the whole stroke, before the first step
            b.queue_forces(*stroke(step, args.batch, dim_x, dim_y), step=step)
        fill = args.every * args.capacity   # steps that fill the recorder
        for first in range(0, args.steps, fill):
            b.record_start(every=args.every, scaling=args.scaling, byteswap=False, capacity=args.capacity)
            # one call per recorder fill, asynchronous: the steps between two frames are one launch, the frame's render
            # is queued behind it, and the later records of the stroke move down by the steps run
            b.step_n(min(fill, args.steps - first), DT, 1.0, args.iters, OMEGA)
            written = write_sheets(b.frames(), written, args.columns, args.out)
    print(f"wrote {written} contact sheets of {args.batch} members to {args.out}")


if __name__ == "__main__":
    main()
