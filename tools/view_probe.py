#!/usr/bin/env python3
"""What the views cost (sfl_view_*, sfl_batch_view_*, sfl_batch_record_view; csrc/field_view.hip), next to the dye's frames.

    python tools/view_probe.py --step STEP --case K [--out profiles/views.txt] [--reps R] [--steps N] [--iters I]

ONE timed step per invocation, so that each runs in a process of its own under a time limit of its own; the lines are
appended to --out.  The whole file is these invocations chained with && (a step that fails ends the chain):

    python tools/view_probe.py --step resources \\
    && timeout -k 10 300 python tools/view_probe.py --step frame --case 0 && timeout -k 10 300 python tools/view_probe.py --step frame --case 1 \\
    && timeout -k 10 300 python tools/view_probe.py --step members --case 0 && timeout -k 10 300 python tools/view_probe.py --step members --case 1 \\
    && timeout -k 10 300 python tools/view_probe.py --step field --case 0 && timeout -k 10 300 python tools/view_probe.py --step field --case 1

Cases: 0 = 61 x 81 with B = 1024, 1 = 128 x 128 (large members) with B = 256; scaling 4; every member from the sketch's
fields with a drag of its own and 20 steps behind it.  Timed as tools/batch_render_probe.py times: a host clock around a
synchronize, one warm-up, the best and the median of R repetitions.
  resources  no GPU: VGPRs, LDS and scratch of the kernels from the compiler's resource report (the library's flags);
  frame      on the stream: step_n(N) with a recorder at every = 1 that draws the dye, the same with a recorder that draws
             the vorticity (sfl_batch_record_view), and the same call without a recorder -- all three in this process; a
             frame's cost is the difference per frame.  The dye frame of the same run is the yardstick;
  members    sfl_batch_view_render_members against sfl_batch_render_members (both include the copy of B images);
  field      sfl_batch_view_scalar(divergence) of the whole batch, the download of a field of the same bytes (the copy
             the call cannot avoid), their difference, and sfl_batch_flow_stats' velocity pass, which reads the same
             8 B per node and writes nothing.
By the model a view frame reads 8 B per node (4 for the pressure) where the dye frame reads 12, and writes the same 2 B per
pixel."""
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
CASES = [((61, 81), 1024, False), ((128, 128), 256, True)]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math"]
HIPCC = "/opt/rocm/bin/hipcc"


def resources():
    source = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "field_view.hip")
    with tempfile.TemporaryDirectory() as tmp:
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", source, "-o",
                            os.path.join(tmp, "field_view.o")], capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise RuntimeError(r.stderr[-2000:])
    scratch = [int(m.group(1)) for m in re.finditer(r"ScratchSize \[bytes/lane\]: (\d+)", r.stderr)]
    if not scratch or any(scratch):
        raise RuntimeError(f"the kernels must not use scratch: {scratch}")
    return ["## resources: hipcc " + " ".join(FLAGS) + " -Rpass-analysis=kernel-resource-usage -c csrc/field_view.hip"] + \
           ["#   " + m.group(1).rstrip() for m in re.finditer(r"remark: (.*?) \[-Rpass-analysis", r.stderr)]


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


def ms(pair):
    return f"best {pair[0] * 1e3:9.3f} ms   median {pair[1] * 1e3:9.3f} ms"


def prepared(case, iters):
    (dim_x, dim_y), batch, large = CASES[case]
    b = sfl.BatchSolver(dim_x, dim_y, batch, large=large)
    b.setup_sketch_fields()
    b.queue_forces(np.arange(batch, dtype=np.int32), [(m % dim_x, (m // dim_x) % dim_y) for m in range(batch)],
                   [(10.0 + m % 7, -5.0 + m % 11) for m in range(batch)])
    b.step_n(20, DT, DX, iters, OMEGA)
    b.synchronize()
    return b


def measure(step, case, reps, steps, iters):
    (dim_x, dim_y), batch, large = CASES[case]
    cells, pixels = dim_x * dim_y, SCALING * (dim_x - 1) * SCALING * (dim_y - 1)
    view = sfl.View(sfl.capi.VIEW_VORTICITY, -1.0, 1.0, sfl.PALETTE_BLUE_WHITE_RED)
    out = [f"## {step}: {dim_x} x {dim_y}{' (large members)' if large else ''}, B = {batch}, scaling {SCALING}, {reps} repetitions; "
           f"device: {sfl.device_info(0)[0]}"]
    nothing = lambda: None
    with prepared(case, iters) as b:
        if step == "frame":
            run = lambda: b.step_n(steps, DT, DX, iters, OMEGA)
            plain = timed(run, b.synchronize, reps)
            restart = lambda: b.record_start(every=1, scaling=SCALING, capacity=steps)   # (after the first: no allocation)
            dye = timed(run, b.synchronize, reps, before=restart)

            def restart_view():
                restart()
                b.record_view(view)
            vort = timed(run, b.synchronize, reps, before=restart_view)
            b.record_stop()
            f_dye, f_view = (dye[1] - plain[1]) / steps, (vort[1] - plain[1]) / steps
            out += [f"step_n({steps}), {iters} iterations, no recorder:  {ms(plain)}",
                    f"    ... a recorder that draws the dye:        {ms(dye)}   {f_dye * 1e6:8.1f} us per frame (median)",
                    f"    ... a recorder that draws the vorticity:  {ms(vort)}   {f_view * 1e6:8.1f} us per frame (median)",
                    f"    spread of the dye run (median - best) per frame: {(dye[1] - dye[0]) / steps * 1e6:.1f} us; by the model the dye frame "
                    f"moves {batch * (12 * cells + 2 * pixels) / 1e6:.1f} MB, the view frame {batch * (8 * cells + 2 * pixels) / 1e6:.1f} MB"]
        elif step == "members":
            dye = timed(lambda: b.render_members(0, batch, SCALING), nothing, reps)
            vort = timed(lambda: b.view_render_members(view, 0, batch, SCALING), nothing, reps)
            out += [f"sfl_batch_render_members:       {ms(dye)}", f"sfl_batch_view_render_members:  {ms(vort)}   ({batch * pixels * 2 / 1e6:.1f} MB of pixels copied by both)"]
        elif step == "field":
            scalar = timed(lambda: b.view_scalar(sfl.capi.VIEW_DIVERGENCE), nothing, reps)
            copy = timed(lambda: b.download(2), nothing, reps)
            stats = timed(lambda: b.flow_stats(velocity=True, dye=False), nothing, reps)
            out += [f"sfl_batch_view_scalar(divergence):   {ms(scalar)}   ({batch * cells * 4 / 1e6:.1f} MB of scalars copied)",
                    f"sfl_batch_download of as many bytes: {ms(copy)}   difference of the medians {(scalar[1] - copy[1]) * 1e6:.1f} us",
                    f"sfl_batch_flow_stats, velocity pass: {ms(stats)}"]
        else:
            raise ValueError(step)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--step", required=True, choices=["resources", "frame", "members", "field"])
    ap.add_argument("--case", type=int, default=0, choices=[0, 1])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "views.txt"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50, help="steps of the call timed by --step frame = frames recorded")
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    if a.step == "resources":
        text = ["# The views: csrc/field_view.hip behind sfl_view_*, sfl_batch_view_* and sfl_batch_record_view.",
                "# Written by tools/view_probe.py, one invocation per section (its docstring has the command lines).", ""] + resources()
        mode = "w"
    else:
        if sfl.device_count() < 1:
            raise SystemExit("no GPU: nothing measured")
        text = [""] + ["# python tools/view_probe.py " + " ".join(sys.argv[1:])] + measure(a.step, a.case, a.reps, a.steps, a.iters)
        mode = "a"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, mode) as f:
        f.write("\n".join(text) + "\n")
    print("\n".join(text))
    return 0


if __name__ == "__main__":
    sys.exit(main())
