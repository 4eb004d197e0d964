#!/usr/bin/env python3
"""What the averages cost: the numbers of profiles/means.txt.

Three workloads, each in one process, warmed, the configurations alternating, host clock around the calls and the synchronise
that ends them:

  batch     61 x 81 x 1024 members at 20 iterations
  context   2048 x 2048 at 40 iterations
  large     8192 x 8192 at 40 iterations (--large; ten planes there are 5.4 GB)

and for each

  1. one sample on the stream, per mask: n x mean_sample() and ONE synchronise, beside the step it follows (step_n(n) without
     averages), as microseconds and as bytes per second in the rule's byte model -- 8 B of velocity, 4 B of pressure and 12 B
     of dye per cell as far as the mask reads them, 16 B per live plane.  The yardsticks of the same job: residual(), which
     reads 8 B per cell (p and d), and flow_stats(dye=False), which reads 8 B per cell (the velocity).  Both are synchronous
     calls -- a launch, a copy of one record and a wait each -- so on the small workloads they show the cost of a wait, not
     of a pass; the 8192 x 8192 context is where the comparison per byte means something;
  2. the loop the averages replace: per sample a download of the fields and the sums in numpy (tests/mean_rule.py's
     arithmetic), for the mask 3 (mean velocity and Reynolds stresses);
  3. nothing on: step_n(n) against the parent commit's library (--parent PATH) in the same rounds through the same raw ctypes
     calls, on --objects batches (contexts) of each made in turn.  The ONE condition: this library's median agrees with the
     parent's inside the parent's own spread over its rounds and objects, max - min.  Both values are written down.

usage: python3 tools/mean_probe.py [--parent libsfl_parent.so] [--large] [--objects K] [--reps R] [--steps N] [--out profiles/means.txt]"""
import argparse
import ctypes as C
import importlib
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sfl = importlib.import_module("esp32-fluid-simulation_amd")
capi = sfl.capi

OUT = []
DT, DX, OMEGA = 0.05, 1.0, 1.9
MASKS = (1, 2, 4, 8, 6, 15)
GROUP_OF = (1, 1, 2, 2, 2, 4, 4, 8, 8, 8)


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def timed(call, sync):
    sync()
    t = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t) * 1e6


def model_bytes(what):
    """Bytes per cell and sample in the rule's byte model."""
    fields = (8 if what & 3 else 0) + (4 if what & 4 else 0) + (12 if what & 8 else 0)
    return fields + 16 * sum(1 for g in GROUP_OF if what & g)


class Raw:
    """The few calls of the C ABI the comparison with the parent's library needs, on either library, through the same code."""

    def __init__(self, path, batch, dim_x, dim_y, members):
        self.lib = C.CDLL(path)
        for name, (res, args) in capi.SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = res, args
        self.batch, self.h = batch, C.c_void_p()
        if batch:
            self.ok(self.lib.sfl_batch_create(C.byref(self.h), 0, dim_x, dim_y, members))
            self.ok(self.lib.sfl_batch_setup_sketch_fields(self.h))
        else:
            self.ok(self.lib.sfl_create(C.byref(self.h), 0, dim_x, dim_y))
            self.ok(self.lib.sfl_setup_sketch_fields(self.h))

    def ok(self, rc):
        if rc != capi.OK:
            raise SystemExit(f"{self.lib._name}: {self.lib.sfl_last_error().decode()}")

    def step_n(self, n, iters):
        self.ok((self.lib.sfl_batch_step_n if self.batch else self.lib.sfl_step_n)(self.h, n, DT, DX, iters, OMEGA))

    def synchronize(self):
        self.ok((self.lib.sfl_batch_synchronize if self.batch else self.lib.sfl_synchronize)(self.h))

    def close(self):
        (self.lib.sfl_batch_destroy if self.batch else self.lib.sfl_destroy)(self.h)


def nothing_on(a, batch, dim_x, dim_y, members, iters):
    n = a.steps
    libs = {"this": capi.LIB_PATH}
    if a.parent:
        libs["parent"] = os.path.abspath(a.parent)
    raws = [(name, k, Raw(path, batch, dim_x, dim_y, members)) for k in range(a.objects) for name, path in libs.items()]
    for _, _, r in raws:
        r.step_n(2, iters)
    us = {(name, k): [] for name, k, _ in raws}
    for rnd in range(a.warmup + a.reps):
        for name, k, r in (raws if rnd % 2 == 0 else raws[::-1]):   # (either end first in turn)
            t = timed(lambda: r.step_n(n, iters), r.synchronize)
            if rnd >= a.warmup:
                us[(name, k)].append(t / n)
    per_lib = {}
    for name in libs:
        meds = [statistics.median(us[(name, k)]) for k in range(a.objects)]
        every = [t for k in range(a.objects) for t in us[(name, k)]]
        per_lib[name] = (statistics.median(every), min(every), max(every), meds)
        say(f"  3. {name:<7} nothing on, {a.objects} objects: median {per_lib[name][0]:9.2f} us per step   min {min(every):9.2f}   max {max(every):9.2f}   "
            f"medians of the objects {', '.join(f'{m:.2f}' for m in meds)}")
    if a.parent:
        med, lo, hi, meds = per_lib["parent"]
        gap = per_lib["this"][0] - med
        verdict = "inside" if abs(gap) <= hi - lo else "OUTSIDE"
        say(f"     this - parent = {gap:+.2f} us per step ({100 * gap / med:+.2f} %): {verdict} the parent's own max - min of {hi - lo:.2f} "
            f"(its objects' medians spread {max(meds) - min(meds):.2f})")
    else:
        say("     the parent's library: not measured (no --parent)")
    for _, _, r in raws:
        r.close()
    return per_lib["this"][0]


def workload(a, batch, dim_x, dim_y, members, iters, replaced=True):
    n = a.steps
    cells = dim_x * dim_y * members
    what = f"batch of {members} x ({dim_x} x {dim_y})" if batch else f"context of {dim_x} x {dim_y}"
    say(f"{what}, {cells} cells, step_n({n}) of {iters} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the configurations alternating, "
        f"host clock around the calls + one synchronize:")
    step_us = nothing_on(a, batch, dim_x, dim_y, members, iters)
    s = sfl.BatchSolver(dim_x, dim_y, members) if batch else sfl.Solver(dim_x, dim_y)
    s.setup_sketch_fields()
    s.step_n(2, DT, DX, iters, OMEGA)

    def samples():
        for _ in range(n):
            s.mean_sample()

    def residuals():
        for _ in range(n):
            s.residual() if not batch else s.flow_stats(DX, velocity=False, dye=True)

    def velocity_passes():
        for _ in range(n):
            s.flow_stats(DX, velocity=True, dye=False)

    # ---- 1. one sample per mask, and the yardsticks
    runs = {}
    for what_ in MASKS:
        runs[f"mean_sample, mask {what_:2d}"] = (what_, samples)
    yard_a = "sfl_residual (8 B/cell)" if not batch else "flow_stats, dye pass (12 B/cell)"
    runs[yard_a] = (None, residuals)
    runs["flow_stats, velocity pass (8 B/cell)"] = (None, velocity_passes)
    us = {name: [] for name in runs}
    for k in range(a.warmup + a.reps):
        for name, (what_, call) in runs.items():
            if what_ is not None:
                s.mean_start(what_, 0)
            t = timed(call, s.synchronize)
            if what_ is not None:
                s.mean_stop()
            if k >= a.warmup:
                us[name].append(t / n)
    rates = {}
    for name, (what_, _) in runs.items():
        med = statistics.median(us[name])
        per_cell = model_bytes(what_) if what_ is not None else 12 if "dye" in name else 8
        rates[name] = cells * per_cell / (med * 1e-6) / 1e9
        say(f"  1. {name:<38} median {med:10.2f} us   min {min(us[name]):10.2f}   max {max(us[name]):10.2f}   {per_cell:3d} B/cell   {rates[name]:8.1f} GB/s"
            + (f"   {100 * med / step_us:6.2f} % of the step of {step_us:.2f} us" if what_ is not None else "   (synchronous: launch + copy + wait)"))
    # ---- behind the steps: every = 1 against nothing on, the same object
    for what_ in (3, 15):
        plain_us, on_us = [], []
        for k in range(a.warmup + a.reps):
            t0 = timed(lambda: s.step_n(n, DT, DX, iters, OMEGA), s.synchronize)
            s.mean_start(what_, 1)
            t1 = timed(lambda: s.step_n(n, DT, DX, iters, OMEGA), s.synchronize)
            s.mean_stop()
            if k >= a.warmup:
                plain_us.append(t0 / n)
                on_us.append(t1 / n)
        say(f"  1. step_n with averages on, mask {what_:2d}, every 1: {statistics.median(on_us):9.2f} us per step against {statistics.median(plain_us):9.2f} without "
            f"(+{statistics.median(on_us) - statistics.median(plain_us):.2f}; a context's step_n runs without its fused boundaries while the hook is set)")
    # ---- 2. the loop it replaces: a download per sample and numpy
    if replaced:
        down, host = [], []
        for k in range(2 + 3):
            sync = s.synchronize
            sync()
            t = time.perf_counter()
            v = s.download(capi.FIELD_VELOCITY)
            t1 = time.perf_counter()
            x, y = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
            if k == 0:
                acc = [np.zeros(x.shape) for _ in range(5)]
            for plane, term in zip(acc, (x, y, x * x, y * y, x * y)):
                plane += term
            t2 = time.perf_counter()
            if k >= 2:
                down.append((t1 - t) * 1e6)
                host.append((t2 - t1) * 1e6)
        say(f"  2. the loop it replaces, mask 3: download of the velocity {statistics.median(down):10.1f} us + numpy {statistics.median(host):10.1f} us per sample")
    s.close()
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsfl_hip.so of the parent commit: the step with nothing on is run on it too")
    ap.add_argument("--reps", type=int, default=12)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--objects", type=int, default=3, help="batches (contexts) per library in the comparison with the parent")
    ap.add_argument("--large", action="store_true", help="also the 8192 x 8192 context")
    ap.add_argument("--only", choices=["batch", "context", "large"], default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/mean_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    if a.only in (None, "batch"):
        workload(a, True, 61, 81, 1024, 20)
    if a.only in (None, "context"):
        workload(a, False, 2048, 2048, 1, 40)
    if a.only == "large" or (a.only is None and a.large):
        a.objects, a.steps, a.reps = 1, 4, max(4, a.reps // 2)
        workload(a, False, 8192, 8192, 1, 40, replaced=False)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
