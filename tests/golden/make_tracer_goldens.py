#!/usr/bin/env python3
"""Regenerates the fixtures of the tracers: tests/golden/tracers_reference.txt -- the output of tests/cpp/tracer_driver.cpp
compiled against the REFERENCE's advect.h (/root/reference, build container only), which tests/test_tracers.py compares with
the build against include/sfl -- and tests/golden/tracers_33x17.npz / tracers_61x81.npz, the same run with its fields for
the GPU tests: velocity, dye, pressure, divergence, dt, positions[7, n, 2] (the starts, then after each of 6 advances) and
the four fields sampled at the final positions without and with no_slip.  The fixtures are data: bits the reference's
sample() leaves behind.  Nothing of the reference's source is stored.

A fixture is refused unless every branch of sample() occurs over its tracer-advances: interior, x outside only, y outside
only, corner, a no-slip wall weight inside (0, 1) and a wall weight of 0."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_header_goldens import REF, run_driver  # noqa: E402

DRIVER = "tracer_driver.cpp"


def parse(text):
    """{(dim_x, dim_y): fixture arrays} from the driver's output with fields."""
    shapes = {}
    for line in text.splitlines():
        w = line.split()
        dim = (int(w[1]), int(w[2]))
        s = shapes.setdefault(dim, {"F": [], "P": [], "S": []})
        if w[0] == "D":
            s["dt"], s["n"] = np.array(int(w[3], 16), np.uint32).view(np.float32), int(w[4])
        else:
            s[w[0]].append([int(x, 16) for x in (w[4:] if w[0] == "F" else w[5:])])
    out = {}
    for (dim_x, dim_y), s in shapes.items():
        f = np.array(s["F"], np.uint32).reshape(dim_y, dim_x, 7)
        n = s["n"]
        smp = np.array(s["S"], np.uint32).reshape(2, n, 7)
        out[(dim_x, dim_y)] = dict(
            velocity=f[..., 0:2].copy().view(np.float32), dye=f[..., 2:5].copy(), pressure=f[..., 5].copy().view(np.float32),
            divergence=f[..., 6].copy().view(np.float32), dt=s["dt"], positions=np.array(s["P"], np.uint32).reshape(7, n, 2).view(np.float32),
            sample_velocity=smp[..., 0:2].copy().view(np.float32), sample_dye=smp[..., 2:5].copy(),
            sample_pressure=smp[..., 5].copy().view(np.float32), sample_divergence=smp[..., 6].copy().view(np.float32))
    return out


def branches(fix):
    """How often each branch of sample() is taken by the advances of a fixture (the positions BEFORE each advance)."""
    dim_y, dim_x = fix["pressure"].shape
    pos = fix["positions"][:-1].reshape(-1, 2).astype(np.float64)
    x, y = pos[:, 0], pos[:, 1]
    x_out, y_out = (x < 0) | (x >= dim_x - 1), (y < 0) | (y >= dim_y - 1)
    beyond_x = np.where(x < 0, -x, x - (dim_x - 1))
    beyond_y = np.where(y < 0, -y, y - (dim_y - 1))
    part = ((x_out & (beyond_x > 0) & (beyond_x < 0.5)) | (y_out & (beyond_y > 0) & (beyond_y < 0.5)))
    zero = (x_out & (beyond_x >= 0.5)) | (y_out & (beyond_y >= 0.5))
    return {"interior": int((~x_out & ~y_out).sum()), "x outside only": int((x_out & ~y_out).sum()),
            "y outside only": int((~x_out & y_out).sum()), "corner": int((x_out & y_out).sum()),
            "wall weight in (0, 1)": int(part.sum()), "wall weight 0": int(zero.sum())}


if __name__ == "__main__":
    if not os.path.isdir(REF):
        sys.exit("needs /root/reference")
    fixtures = parse(run_driver(REF, DRIVER, ("TRACER_DRIVER_FIELDS",)))
    for (dim_x, dim_y), fix in fixtures.items():
        seen = branches(fix)
        missing = [name for name, count in seen.items() if count == 0]
        if missing:
            sys.exit(f"tracers_{dim_x}x{dim_y}: no tracer-advance takes {missing}: fixture refused ({seen})")
        moved = int((fix["positions"][0].view(np.uint32) != fix["positions"][-1].view(np.uint32)).any(axis=1).sum())
        print(f"tracers_{dim_x}x{dim_y}: {seen}, {moved} of {fix['positions'].shape[1]} tracers moved")
    text = run_driver(REF, DRIVER)
    with open(os.path.join(HERE, "tracers_reference.txt"), "w") as f:
        f.write(text)
    print(f"tracers_reference.txt: {len(text.splitlines())} lines written")
    for (dim_x, dim_y), fix in fixtures.items():
        np.savez_compressed(os.path.join(HERE, f"tracers_{dim_x}x{dim_y}.npz"), **fix)
