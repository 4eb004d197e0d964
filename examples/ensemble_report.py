#!/usr/bin/env python3
"""How far is each (omega, iters) member of examples/omega_study.py's ensemble from a member one can trust?  The same
batch -- the sketch's 61 x 81 start with one drag, one member per (omega, iters) point -- plus ONE reference member run
with 400 iterations at omega 1.9, a few steps, and then, without downloading a field:

  * the distance of every member's velocity and dye from the reference's (sfl_batch_distance), as a table;
  * the mean picture of the ensemble and the picture of where its members disagree -- per cell max - min of the dye
    (sfl_batch_envelope) -- as mean.ppm and spread.ppm.

    python examples/ensemble_report.py [--steps 5] [--out ensemble_report] [--scaling 4]

Needs a GPU: there is no CPU fallback."""
import argparse
import importlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")

OMEGAS = (1.0, 1.5, 1.8, 1.9, 1.96, 1.99)
ITERS = (5, 10, 20, 40, 80)
REFERENCE = (1.9, 400)   # omega, iterations of the member the others are measured against


def rgb565_to_rgb888(img):
    r = ((img >> 11) & 0x1F).astype(np.uint8) << 3
    g = ((img >> 5) & 0x3F).astype(np.uint8) << 2
    b = (img & 0x1F).astype(np.uint8) << 3
    return np.stack([r, g, b], axis=-1)


def write_ppm(path, img565):
    img = rgb565_to_rgb888(img565)
    with open(path, "wb") as f:
        f.write(b"P6 %d %d 255\n" % (img.shape[1], img.shape[0]))
        f.write(img.tobytes())


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default="ensemble_report")
    ap.add_argument("--scaling", type=int, default=4)
    args = ap.parse_args()
    omega, iters = (a.reshape(-1) for a in np.meshgrid(OMEGAS, ITERS, indexing="ij"))   # member = omega-major
    members = len(omega)
    omega, iters = np.append(omega, REFERENCE[0]), np.append(iters, REFERENCE[1])       # the reference is the last member
    batch = members + 1
    with sfl.BatchSolver(61, 81, batch) as b:
        b.setup_sketch_fields()
        b.queue_forces(np.arange(batch), [(30, 40)] * batch, [(40.0, -25.0)] * batch)    # the same drag for every member
        b.step_n_each(args.steps, dt=1 / 30, dx=1.0, iters=iters, omega=omega)
        far = b.distance(ref_member=members, count=members, pressure=False)
        b.envelope(0, members)                                                           # (the reference is not part of the pictures)
        mean = b.envelope_render(sfl.capi.ENV_MEAN, args.scaling, byteswap=False)
        spread = b.envelope_render(sfl.capi.ENV_SPREAD, args.scaling, byteswap=False)
        widest = int(b.envelope_field(sfl.capi.ENV_SPREAD).max())
    print(f"distance from the member with omega {REFERENCE[0]} and {REFERENCE[1]} iterations after {args.steps} steps, 61 x 81")
    print("omega  iters   max |dv.x|   max |dv.y|   dye cells differ   max |d dye| (raw UQ32, per channel)")
    for w, n, r in zip(omega, iters, far):
        print(f"{w:<7.2f}{n:>5d}{r['max_abs_dvx']:>13.3e}{r['max_abs_dvy']:>13.3e}{r['dye_cells_differ']:>19d}   "
              + " ".join(f"{int(x):>10d}" for x in r["max_abs_ddye"]))
    os.makedirs(args.out, exist_ok=True)
    write_ppm(os.path.join(args.out, "mean.ppm"), mean)
    write_ppm(os.path.join(args.out, "spread.ppm"), spread)
    print(f"wrote mean.ppm and spread.ppm ({mean.shape[1]} x {mean.shape[0]}) to {args.out}; the widest spread of a channel is "
          f"{widest} raw units = {widest / 2 ** 32:.4f} of full scale")
