#!/usr/bin/env python3
"""What the viscosity costs: the timings of profiles/viscosity.txt (include/sfl.h "VISCOSITY").

In one process, warmed, host clock around a burst of calls and the synchronise that ends it, the variants alternating:

  1. BATCH COST     61 x 81 x 1024 members at 20 iterations: step_n of (a) a plain batch, (b) a batch with a viscosity set
                    whose members all have nu = 0 (the viscous kernel, the item skipped) and (c) one with nu > 0 in every
                    member and --sweeps sweeps.  (c) - (a) is the added time per step, divided by the sweeps the time per
                    sweep (the set-up of the item included).
  2. CONTEXT COST   2048 x 2048: ONE blocked launch of 8 sweeps (diffuse_velocity) against the masked solve's one launch of
                    8 iterations on the pressure held (poisson_continue with an empty mask set): the like-for-like kernel,
                    same tile, same window, same blocking in time; it moves 4 B per cell where the diffusion moves 8.
  3. OFF MEANS OFF  --off-vs PARENT_TREE (a checkout of the parent commit with its library built): with a viscosity never
                    set, step_n of the batch of 1. and of the context of 2. (40 iterations) under this build's library and
                    under the parent commit's, each in fresh child processes through the PARENT's tools/with_lib.py and
                    binding (which declares the symbols both libraries have), alternating; the difference of the medians
                    beside the run-to-run spread of the parent's own repeats.

usage: python3 tools/viscosity_probe.py [--reps R] [--out FILE]
       python3 tools/viscosity_probe.py --off-vs path/to/parent/checkout [--rounds N] [--out FILE]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OUT = []
DT, DX, OMEGA = 0.05, 1.0, 1.9


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def burst(call, sync, n):
    """Microseconds per call of n calls queued back to back."""
    sync()
    t = time.perf_counter()
    for _ in range(n):
        call()
    sync()
    return (time.perf_counter() - t) * 1e6 / n


def alternate(variants, a, per_round):
    """name -> [us per call], the variants taking turns; the first a.warmup rounds are not kept."""
    us = {name: [] for name in variants}
    for r in range(a.warmup + a.reps):
        for name, (call, sync) in variants.items():
            t = burst(call, sync, per_round)
            if r >= a.warmup:
                us[name].append(t)
    return us


def report(us, base, unit):
    med = {name: statistics.median(u) for name, u in us.items()}
    for name, u in us.items():
        mad = statistics.median(abs(x - med[name]) for x in u)
        say(f"  {name:<34} median {med[name]:9.1f} us per {unit}   min {min(u):9.1f}   max {max(u):9.1f}   MAD {mad:6.1f}   vs {base.split()[0]} {med[name] / med[base]:6.3f} x")
    return med


def batch_of(sfl, batch, nu=None, sweeps=0):
    b = sfl.BatchSolver(61, 81, batch)
    b.setup_sketch_fields()
    if nu is not None:
        b.set_viscosity(nu, sweeps)
    return b


def batch_cost(sfl, a):
    B, iters, steps = 1024, 20, 8
    nu = np.geomspace(1e-3, 1.0, B).astype(np.float32)
    batches = {"(a) plain": batch_of(sfl, B), "(b) viscosity set, every nu = 0": batch_of(sfl, B, 0.0, a.sweeps),
               f"(c) nu > 0, {a.sweeps} sweeps": batch_of(sfl, B, nu, a.sweeps)}
    say(f"1. BATCH COST: 61 x 81 x {B} members, {iters} iterations, step_n({steps}) per burst, {a.warmup} warm-up and {a.reps} timed rounds")
    us = alternate({n: ((lambda b=b: b.step_n(steps, DT, DX, iters, OMEGA)), b.synchronize) for n, b in batches.items()}, a, 1)
    us = {n: [x / steps for x in u] for n, u in us.items()}
    med = report(us, "(a) plain", "step")
    names = list(batches)
    added = med[names[2]] - med[names[0]]
    say(f"  added by the diffusion: {added:.1f} us per step, {added / a.sweeps:.1f} us per sweep; by the viscous kernel with the item skipped: "
        f"{med[names[1]] - med[names[0]]:.1f} us per step; spread of (a): max - min = {max(us[names[0]]) - min(us[names[0]]):.1f} us")
    cap = sfl.capi
    same = all(np.array_equal(batches[names[0]].download(f).view(np.uint32), batches[names[1]].download(f).view(np.uint32))
               for f in (cap.FIELD_VELOCITY, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
    say(f"  after all of it (a) and (b) hold the same bits in velocity, pressure and dye: {same}")
    say()
    for b in batches.values():
        b.close()
    return same


def context_cost(sfl, a):
    dim, k, per = 2048, 8, 20
    cells = dim * dim
    s = sfl.Solver(dim, dim)
    s.setup_sketch_fields()
    s.step_n(2, DT, DX, 16, OMEGA)
    m = sfl.Solver(dim, dim)
    m.setup_sketch_fields()
    m.set_solids(np.zeros((dim, dim), bool))
    m.step_n(2, DT, DX, 16, OMEGA)
    w = sfl.Solver(dim, dim)   # the diffusion with a mask set: the code bytes are read too
    w.setup_sketch_fields()
    w.set_solids(np.zeros((dim, dim), bool))
    w.step_n(2, DT, DX, 16, OMEGA)
    say(f"2. CONTEXT COST: {dim} x {dim}, one launch of {k} sweeps / iterations, {per} calls per burst, {a.warmup} warm-up and {a.reps} timed rounds")
    us = alternate({"(s) masked solve, 8 iterations": ((lambda: m.poisson_continue(DX, k, OMEGA)), m.synchronize),
                    "(d) diffusion, 8 sweeps": ((lambda: s.diffuse_velocity(0.3, DT, DX, k)), s.synchronize),
                    "(e) diffusion, 8 sweeps, mask set": ((lambda: w.diffuse_velocity(0.3, DT, DX, k)), w.synchronize)}, a, per)
    med = report(us, "(s) masked solve, 8 iterations", "launch")
    # bytes model: a 64 x 32 tile loads its 96 x 64 window (3 x the cells) of every field it reads and stores its own cells
    solve_bytes, diff_bytes = 3 * (4 + 4 + 1) + 4, 3 * 8 + 8
    say(f"  bytes per cell and launch by the window model (reads x 3, the window over the tile): solve p + d + code read, p written = {solve_bytes} B; "
        f"diffusion u read (u0 is the same line in a first launch), u written = {diff_bytes} B; compulsory: 13 B and 16 B")
    for name, b in (("(s) masked solve, 8 iterations", solve_bytes), ("(d) diffusion, 8 sweeps", diff_bytes)):
        say(f"  {name}: {cells * b / med[name] / 1e3:.0f} GB/s by the window model, {med[name] / k:.1f} us per sweep / iteration")
    say(f"  ratio diffusion / masked solve: {med['(d) diffusion, 8 sweeps'] / med['(s) masked solve, 8 iterations']:.3f} (bytes model: {diff_bytes / solve_bytes:.3f})")
    say()
    for x in (s, m, w):
        x.close()


def off_leg(a):
    """A child of --off-vs: times the two plain calls under whatever library tools/with_lib.py loaded; one JSON line."""
    sfl = importlib.import_module("esp32-fluid-simulation_amd")
    b = batch_of(sfl, 1024)
    s = sfl.Solver(2048, 2048)
    s.setup_sketch_fields()
    variants = {"batch": ((lambda: b.step_n(8, DT, DX, 20, OMEGA)), b.synchronize), "context": ((lambda: s.step_n(4, DT, DX, 40, OMEGA)), s.synchronize)}
    us = alternate(variants, a, 1)
    print("OFF " + json.dumps({"batch_us_per_step": statistics.median(us["batch"]) / 8, "context_us_per_step": statistics.median(us["context"]) / 4}))


def off_means_off(a):
    own = os.path.join(ROOT, "esp32-fluid-simulation_amd", "lib", "libsfl_hip.so")
    parent = os.path.abspath(a.off_vs)
    libs = {"parent": os.path.join(parent, "esp32-fluid-simulation_amd", "lib", "libsfl_hip.so"), "this build": own}
    got = {name: {"batch_us_per_step": [], "context_us_per_step": []} for name in libs}
    say(f"3. OFF MEANS OFF: viscosity never set; sfl_batch_step_n (61 x 81 x 1024, 20 iterations) and sfl_step_n (2048 x 2048, 40 iterations); "
        f"{a.rounds} fresh processes per library, alternating, each the median of {a.reps} timed rounds behind {a.warmup} warm-up rounds")
    for r in range(a.rounds):
        for name, lib in libs.items():
            cmd = [sys.executable, os.path.join(parent, "tools", "with_lib.py"), lib, os.path.abspath(__file__), "--off-leg", "--reps", str(a.reps),
                   "--warmup", str(a.warmup)]
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=parent)
            line = [x for x in p.stdout.splitlines() if x.startswith("OFF ")]
            if p.returncode != 0 or not line:
                say(f"  a leg under {name} failed (rc {p.returncode}): {p.stderr[-400:]}")
                return False
            for key, value in json.loads(line[0][4:]).items():
                got[name][key].append(value)
    for key in ("batch_us_per_step", "context_us_per_step"):
        p, o = got["parent"][key], got["this build"][key]
        say(f"  {key:<20} parent {statistics.median(p):9.1f} (its repeats: {', '.join(f'{x:.1f}' for x in p)}; max - min {max(p) - min(p):.1f})   "
            f"this build {statistics.median(o):9.1f} ({', '.join(f'{x:.1f}' for x in o)})   difference {statistics.median(o) - statistics.median(p):+.1f} us")
    say()
    return True


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--sweeps", type=int, default=4)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--off-vs", default=None, help="a checkout of the parent commit with its library built: measurement 3 alone")
    ap.add_argument("--off-leg", action="store_true", help="(a child of --off-vs)")
    ap.add_argument("--out", default=None, help="also append the lines to this file")
    a = ap.parse_args()
    if a.off_leg:
        off_leg(a)
        sys.exit(0)
    say("# tools/viscosity_probe.py " + " ".join(sys.argv[1:]))
    if a.off_vs:
        ok = off_means_off(a)
    else:
        sfl = importlib.import_module("esp32-fluid-simulation_amd")
        if sfl.device_count() < 1:
            raise SystemExit("needs a GPU: nothing here is measured without one")
        say(f"# device: {sfl.device_info(0)[0]}")
        ok = batch_cost(sfl, a)
        context_cost(sfl, a)
    if a.out:
        with open(a.out, "a") as f:
            f.write("\n".join(OUT) + "\n")
    sys.exit(0 if ok else 1)
