#!/usr/bin/env python3
"""What a scripted stroke costs a batch, three ways (the timeline of include/sfl.h; csrc/batch_play.hip).

    python tools/batch_script_probe.py [--out profiles/batch_script.txt] [--runs R] [--steps N] [--iters I] [--no-gpu]

The sketch's shape, 61 x 81, 20 iterations, N = 120 steps, B = 1024 (the chip is full) and B = 64 (it is not: latency is
everything); every member gets the nine-record stroke of examples/batch_movie.py in every step.  The clock is a host clock
from the first call to the end of sfl_batch_synchronize; the three ways run interleaved -- a, b, c, a, b, c ... -- in one
process, one warm-up round, then R rounds, every time listed, the median compared:
  (a) queue_forces + step_n(1) per step: the only way there was before the timeline (this way runs unchanged on the commit
      before the timeline: --only-a, for a library that has no `step` argument yet);
  (b) the whole stroke queued with step=, then ONE step_n_until with tol < 0: the timeline on per-step launches;
  (c) the whole stroke queued with step=, then ONE step_n: the timeline through batch_play_kernel, one launch.
All three leave the same bits (checked once per batch size: velocity, divergence, pressure, dye).
The spread of (a)'s own runs is the margin: (c) slower than (a) by more than that is a loss.
Also writes what needs no GPU: the kernel's registers, scratch and LDS from the compiler's resource report."""
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
sys.path.insert(0, os.path.join(ROOT, "examples"))
sfl = importlib.import_module("esp32-fluid-simulation_amd")
from batch_movie import stroke  # noqa: E402

DT, DX, OMEGA = np.float32(1 / 30.0), 1.0, np.float32(1.96)
DIM_X, DIM_Y = 61, 81
BATCHES = [1024, 64]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
HIPCC = "/opt/rocm/bin/hipcc"


def resources():
    """The compiler's resource report of csrc/batch_play.hip, as lines of text."""
    source = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "batch_play.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o",
                            os.path.join(tmp, "batch_play.o")], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    return [m.group(1).rstrip() for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr)]


def measure(batch, steps, iters, runs, only_a):
    # (outside the clock: the stroke is a recording, held as the arrays the calls pass on)
    strokes = [tuple(np.ascontiguousarray(a, t) for a, t in zip(stroke(k, batch, DIM_X, DIM_Y), (np.int32, np.int32, np.float32)))
               for k in range(steps)]
    prm = sfl.member_params(batch, DT, DX, iters, OMEGA)
    stops = sfl.member_stops(batch, -1.0, 4)
    out = [f"## B = {batch}: {DIM_X} x {DIM_Y}, {iters} iterations, {steps} steps, {len(strokes[0][0])} records per step"]
    with sfl.BatchSolver(DIM_X, DIM_Y, batch) as b:
        def way_a():
            for k in range(steps):
                b.queue_forces(*strokes[k])
                b.step_n(1, DT, DX, iters, OMEGA)

        def queue_all():
            for k in range(steps):
                b.queue_forces(*strokes[k], step=k)

        def way_b():
            queue_all()
            b.step_n_until(steps, prm, tol=stops)

        def way_c():
            queue_all()
            b.step_n(steps, DT, DX, iters, OMEGA)

        ways = [("a", way_a)] if only_a else [("a", way_a), ("b", way_b), ("c", way_c)]
        fields = {}
        for name, way in ways:   # the same bits, once
            b.setup_sketch_fields()
            way()
            b.synchronize()
            fields[name] = [b.download(f) for f in (0, 2, 3, 1)]
        same = all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for name in fields for x, y in zip(fields[name], fields["a"]))
        out.append(f"the same bits in all four fields: {same}")
        if not same:
            raise RuntimeError("\n".join(out))
        times = {name: [] for name, _ in ways}
        for run in range(runs + 1):   # run 0 is the warm-up
            for name, way in ways:
                b.setup_sketch_fields()
                b.synchronize()
                t0 = time.perf_counter()
                way()
                b.synchronize()
                if run:
                    times[name].append(time.perf_counter() - t0)
        what = {"a": "(a) queue_forces + step_n(1) per step   ", "b": "(b) timeline, step_n_until (per step)   ",
                "c": "(c) timeline, step_n (batch_play_kernel)"}
        med = {name: statistics.median(t) for name, t in times.items()}
        for name, t in times.items():
            out.append(f"{what[name]}: " + " ".join(f"{x * 1e3:9.3f}" for x in t) + f" ms   median {med[name] * 1e3:9.3f} ms"
                       f" = {med[name] / steps * 1e6:7.1f} us per step")
        spread = max(times["a"]) - min(times["a"])
        out.append(f"spread of (a)'s runs (the margin): {spread * 1e3:.3f} ms")
        if not only_a:
            out.append(f"(a) / (b) = {med['a'] / med['b']:.2f}   (a) / (c) = {med['a'] / med['c']:.2f}   (b) / (c) = {med['b'] / med['c']:.2f}   "
                       f"(c) - (a) = {(med['c'] - med['a']) * 1e3:+.3f} ms")
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "batch_script.txt"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--steps", type=int, default=120)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only-a", action="store_true", help="way (a) alone: what a library without the timeline can run")
    ap.add_argument("--no-gpu", action="store_true", help="the resource report only")
    a = ap.parse_args()
    text = ["# A scripted stroke on a batch, three ways: tools/batch_script_probe.py (its docstring says what is timed and how).",
            "# command: python tools/batch_script_probe.py " + " ".join(sys.argv[1:]), ""]
    if not a.only_a:
        text += ["## 1. Resources: hipcc " + " ".join(FLAGS) + " -Rpass-analysis=kernel-resource-usage -c csrc/batch_play.hip"]
        text += ["#   " + line for line in resources()]
    text += ["", f"## 2. Measured: wall clock from the first call to the end of the synchronize, one warm-up round, {a.runs} rounds"]
    if a.no_gpu or sfl.device_count() < 1:
        text.append("not measured yet (no GPU in this run)")
    else:
        text.append(f"device: {sfl.device_info(0)[0]}")
        for batch in BATCHES:
            text += [""] + measure(batch, a.steps, a.iters, a.runs, a.only_a)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
