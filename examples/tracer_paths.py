#!/usr/bin/env python3
"""Pathlines of K tracers through the sketch: where the fluid goes.

    python examples/tracer_paths.py --tracers 48 --steps 240 --out paths.ppm

The sketch's start (sfl_setup_sketch_fields, ino:196-241), one finger drag replayed from the timeline of forces
(ino:264-269), K tracers on a regular lattice that follow every step (sfl_tracers_set with follow) and a trail that keeps
their positions after every `--every`-th step on the device.  One sfl_step_n call runs it all; afterwards the trail is read
once and the pathlines are drawn over the last frame -- on the host, with numpy -- as a PPM.  Needs a GPU: there is no CPU
fallback.
"""
import argparse
import importlib
import math
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from examples.demo_frames import rgb565_to_rgb888  # noqa: E402


def draw_paths(img, paths, scaling, dim_x, dim_y):
    """paths float32[slots, n, 2] in grid coordinates onto img uint8[H, W, 3]: the image has i down and j across
    (sfl_render_rgb565), scaling pixels per cell.  White lines, a red dot where each tracer ends."""
    h, w = img.shape[:2]
    for k in range(paths.shape[1]):
        p = paths[:, k, :]
        p = p[np.isfinite(p).all(axis=1)]
        for a, b in zip(p[:-1], p[1:]):
            steps = int(max(abs(b - a)) * scaling) + 1
            for t in np.linspace(0.0, 1.0, steps + 1):
                x, y = a + (b - a) * t
                r, c = int(round(x * scaling)), int(round(y * scaling))
                if 0 <= r < h and 0 <= c < w:
                    img[r, c] = (255, 255, 255)
        if len(p):
            r, c = int(round(p[-1][0] * scaling)), int(round(p[-1][1] * scaling))
            img[max(r - 1, 0):r + 2, max(c - 1, 0):c + 2] = (255, 0, 0)
    return img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--tracers", type=int, default=48)
    ap.add_argument("--steps", type=int, default=240)
    ap.add_argument("--every", type=int, default=4)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--scaling", type=int, default=8)
    ap.add_argument("--out", default="tracer_paths.ppm")
    args = ap.parse_args()
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    dim_x, dim_y = args.size
    side = max(int(math.sqrt(args.tracers)), 1)
    gi, gj = np.meshgrid(np.linspace(0.15, 0.85, side) * (dim_x - 1), np.linspace(0.15, 0.85, -(-args.tracers // side)) * (dim_y - 1))
    xy = np.stack([gi.ravel(), gj.ravel()], axis=1)[:args.tracers].astype(np.float32)
    with sfl.Solver(dim_x, dim_y) as s:
        s.setup_sketch_fields()
        # one drag along a quarter circle, a point force per step for the first 60 steps
        radius, speed = 0.3 * min(dim_x, dim_y), 0.15 * min(dim_x, dim_y) * 30
        for step in range(min(60, args.steps)):
            a = 0.5 * math.pi * step / 60
            cell = (int(dim_x / 2 + radius * math.cos(a)), int(dim_y / 2 + radius * math.sin(a)))
            s.queue_forces([cell], [(-speed * math.sin(a), speed * math.cos(a))], step=step)
        s.set_tracers(xy, follow=True)
        slots = args.steps // args.every
        s.trail_start(args.every, max(slots, 1))
        s.step_n(args.steps, np.float32(1 / 30.0), 1.0, args.iters, np.float32(1.96))
        paths = np.concatenate([xy[None], s.trail()])
        img = rgb565_to_rgb888(s.render_rgb565(args.scaling, byteswap=False))
        speed_there = s.sample_tracers(sfl.capi.FIELD_VELOCITY, no_slip=True)
    img = draw_paths(np.ascontiguousarray(img), paths, args.scaling, dim_x, dim_y)
    with open(args.out, "wb") as f:
        f.write(b"P6 %d %d 255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())
    moved = np.linalg.norm(paths[-1] - paths[0], axis=1)
    print(f"{len(xy)} tracers, {args.steps} steps, {len(paths) - 1} trail slots: moved {moved.mean():.2f} cells on average, "
          f"{moved.max():.2f} at most; fastest now {np.abs(speed_there).max():.3f} cells per unit of time; wrote {args.out}")


if __name__ == "__main__":
    main()
