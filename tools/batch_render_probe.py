#!/usr/bin/env python3
"""What the frames of a batch cost (sfl_batch_render_members, sfl_batch_record_*; csrc/batch_render.hip).

    python tools/batch_render_probe.py [--out profiles/batch_render.txt] [--reps R] [--steps N] [--iters I] [--no-gpu]

Writes the file profiles/batch_render.txt holds:
  1. what needs no GPU: the kernel's VGPRs, LDS and scratch from the compiler's resource report (the library's flags);
  2. timed as tools/batch_throughput.py times -- a host clock around a synchronize, one warm-up, the best and the median
     of R repetitions -- at 61 x 81 with B = 1024 and at 128 x 128 (large members) with B = 256, scaling 4, every member
     from the sketch's fields with a drag of its own and 20 steps behind it:
     (a) B calls of sfl_batch_render_rgb565 (B launches, B copies, B waits);
     (b) one sfl_batch_render_members of the same images (checked to be the same bits), and the ratio (a) / (b);
     (c) step_n(N) with a recorder at every = 1 against the same call without one (the frames stay on the device; the
         sfl_batch_record_start that makes room before each repetition is outside the clock);
     the render alone -- (c)'s difference per frame -- as bytes per second by the model 12 B per cell read + 2 B per
     pixel written, next to the 6.3 TB/s a copy achieves on this device.
(b) includes the device-to-host copy of B images, which no kernel can shorten; (c)'s difference does not."""
import argparse
import importlib
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfl = importlib.import_module("esp32-fluid-simulation_amd")

DT, DX, OMEGA = np.float32(1 / 30.0), 1.0, np.float32(1.96)
SCALING = 4
COPY_BYTES_PER_S = 6.3e12
CASES = [((61, 81), 1024, False), ((128, 128), 256, True)]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
HIPCC = "/opt/rocm/bin/hipcc"


def resources():
    """The compiler's resource report of csrc/batch_render.hip, as lines of text."""
    source = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "batch_render.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o",
                            os.path.join(tmp, "batch_render.o")], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    lines = [m.group(1).rstrip() for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr)]
    scratch = [int(m.group(1)) for m in re.finditer(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    if not scratch or any(scratch):
        raise RuntimeError(f"the kernel must not use scratch: {scratch}")
    return lines


def timed(call, sync, reps, before=lambda: None):
    """Seconds of call() + sync(): (best, median) of `reps` repetitions after one warm-up; before() runs outside the clock."""
    before()
    call()
    sync()
    out = []
    for _ in range(reps):
        before()
        t0 = time.perf_counter()
        call()
        sync()
        out.append(time.perf_counter() - t0)
    return min(out), statistics.median(out)


def measure(shape, batch, large, reps, steps, iters):
    dim_x, dim_y = shape
    cells, pixels = dim_x * dim_y, SCALING * (dim_x - 1) * SCALING * (dim_y - 1)
    model = batch * (12 * cells + 2 * pixels)   # bytes of one frame of the whole batch
    out = [f"## {dim_x} x {dim_y}{' (large members)' if large else ''}, B = {batch}, scaling {SCALING}: one frame of the batch = "
           f"{batch * pixels * 2 / 1e6:.1f} MB of pixels, {model / 1e6:.1f} MB by the model"]
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        b.setup_sketch_fields()
        b.queue_forces(np.arange(batch, dtype=np.int32), [(m % dim_x, (m // dim_x) % dim_y) for m in range(batch)],
                       [(10.0 + m % 7, -5.0 + m % 11) for m in range(batch)])
        b.step_n(20, DT, DX, iters, OMEGA)
        b.synchronize()
        nothing = lambda: None
        each = lambda: [b.render_rgb565(m, SCALING) for m in range(batch)]
        a_best, a_med = timed(each, nothing, reps)
        b_best, b_med = timed(lambda: b.render_members(0, batch, SCALING), nothing, reps)
        same = np.array_equal(np.stack(each()), b.render_members(0, batch, SCALING))
        out += [f"(a) {batch} x sfl_batch_render_rgb565:   best {a_best * 1e3:9.3f} ms   median {a_med * 1e3:9.3f} ms",
                f"(b) 1 x sfl_batch_render_members:    best {b_best * 1e3:9.3f} ms   median {b_med * 1e3:9.3f} ms   "
                f"(a) / (b) = {a_best / b_best:.1f} (best), {a_med / b_med:.1f} (median)   same bits: {same}"]
        if not same or b_med >= a_med:
            raise RuntimeError("\n".join(out + ["(b) must give (a)'s bits and beat it"]))
        step = lambda: b.step_n(steps, DT, DX, iters, OMEGA)
        p_best, p_med = timed(step, b.synchronize, reps)
        restart = lambda: b.record_start(every=1, scaling=SCALING, capacity=steps)   # (after the first: no allocation)
        r_best, r_med = timed(step, b.synchronize, reps, before=restart)
        b.record_stop()
        frame = (r_med - p_med) / steps
        out += [f"(c) step_n({steps}), {iters} iterations:        best {p_best * 1e3:9.3f} ms   median {p_med * 1e3:9.3f} ms   without a recorder",
                f"    ... recording at every = 1:       best {r_best * 1e3:9.3f} ms   median {r_med * 1e3:9.3f} ms   "
                f"overhead {100 * (r_med / p_med - 1):.1f} % (median), {frame * 1e6:.1f} us per frame",
                f"    the render alone: {model / frame / 1e12 if frame > 0 else float('nan'):.2f} TB/s by the model, "
                f"{100 * model / frame / COPY_BYTES_PER_S if frame > 0 else float('nan'):.0f} % of a copy's {COPY_BYTES_PER_S / 1e12} TB/s"]
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_render.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50, help="steps of the call timed in (c) = frames recorded")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--no-gpu", action="store_true", help="the resource report only")
    a = ap.parse_args()
    text = ["# The frames of a batch: csrc/batch_render.hip behind sfl_batch_render_members and sfl_batch_record_*.",
            "# Written by tools/batch_render_probe.py (its docstring says what is timed and how).", "",
            "## 1. Resources: hipcc " + " ".join(FLAGS) + " -Rpass-analysis=kernel-resource-usage -c csrc/batch_render.hip"]
    text += ["#   " + line for line in resources()]
    text += ["", f"## 2. Measured: wall clock around a synchronize, one warm-up, {a.reps} repetitions"]
    if a.no_gpu or sfl.device_count() < 1:
        text.append("not measured yet (no GPU in this run)")
    else:
        text.append(f"device: {sfl.device_info(0)[0]}")
        for shape, batch, large in CASES:
            text += [""] + measure(shape, batch, large, a.reps, a.steps, a.iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
