#!/usr/bin/env python3
"""What the torque costs: the numbers of profiles/torque.txt, with the loads and the friction samplers of the same job as
the yardstick -- the torque walks the faces once where the two walk twice.

The two workloads of tools/loads_probe.py and tools/friction_probe.py, each in one process, warmed, its configurations
alternating, host clock around the call and the synchronise that ends it:

  batch    61 x 81 x 1024 members at 20 iterations, one shared disc of radius 8 in every member
  context  2048 x 2048 at 40 iterations, a disc of radius 256

and for each, the configurations with a recorder and (f) in a stream of (20, 3) past the disc -- the sketch's fluid is at rest, where
every product is zero and torque.hip skips the LDS atomic of a zero product --

  (a) step, no recorder            step_n(n) as it ran before there was a torque: the new code in this path is one null-pointer
                                   test and one admission check per call
  (b) step, a torque sample        the same call with the torque recorder on, every = 1, the pivot at the disc's centre
  (c) step, a loads sample         ... with the loads recorder on instead
  (d) step, a friction sample      ... with the friction recorder on instead
  (e) step, loads and friction     ... with those two on: the yardstick of (b)
  (f) torque() alone               the sampler n times through the synchronous call, its copy and wait included; on the stream it
                                   costs (b) - (a)

With --parent PATH (the library of the parent commit, built from a scratch worktree) (a) is also run on that library, the two
alternating in the same rounds through the same raw ctypes calls, on --objects batches (contexts) of each made in turn: where
an object's fields lie moves a step by more than the rounds of one object differ.  The conditions: (a) on this library agrees
with (a) on the parent's inside the spread the probe itself reports for the PARENT's rounds and objects, max - min; and
(b) - (a) is no more than (e) - (a) beyond the spread of (e)'s rounds.  Then (b) to (e) are run on both libraries too
(loads_probe.py samples_against_parent): what a sample costs on this one against what it costs on the parent's.  Everything is
written down as measured either way.

usage: python3 tools/torque_probe.py [--parent libsfl_parent.so] [--objects K] [--reps R] [--steps N] [--out profiles/torque.txt]"""
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
from loads_probe import samples_against_parent   # noqa: E402  (beside this file)

OUT = []
DT, DX, OMEGA = 0.05, 1.0, 1.9


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


def disc(dim_x, dim_y, r):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return ((i - dim_x // 2) ** 2 + (j - dim_y // 2) ** 2 <= r * r).astype(np.uint8)


class Raw:
    """The few calls of the C ABI the comparison with the parent's library needs, on either library, through the same code."""

    def __init__(self, path, batch, dim_x, dim_y, members, mask):
        self.lib = C.CDLL(path)
        for name, (res, args) in capi.SIGNATURES.items():
            if hasattr(self.lib, name):
                fn = getattr(self.lib, name)
                fn.restype, fn.argtypes = res, args
        self.batch, self.h = batch, C.c_void_p()
        ptr = mask.ctypes.data_as(C.POINTER(C.c_uint8))
        if batch:
            self.ok(self.lib.sfl_batch_create(C.byref(self.h), 0, dim_x, dim_y, members))
            self.ok(self.lib.sfl_batch_setup_sketch_fields(self.h))
            self.ok(self.lib.sfl_batch_set_solids(self.h, ptr, 0))
        else:
            self.ok(self.lib.sfl_create(C.byref(self.h), 0, dim_x, dim_y))
            self.ok(self.lib.sfl_setup_sketch_fields(self.h))
            self.ok(self.lib.sfl_set_solids(self.h, ptr))

    def ok(self, rc):
        if rc != capi.OK:
            raise SystemExit(f"{self.lib._name}: {self.lib.sfl_last_error().decode()}")

    def step_n(self, n, iters):
        self.ok((self.lib.sfl_batch_step_n if self.batch else self.lib.sfl_step_n)(self.h, n, DT, DX, iters, OMEGA))

    def synchronize(self):
        self.ok((self.lib.sfl_batch_synchronize if self.batch else self.lib.sfl_synchronize)(self.h))

    def close(self):
        (self.lib.sfl_batch_destroy if self.batch else self.lib.sfl_destroy)(self.h)


def report(us, n, base):
    med = {name: statistics.median(u) for name, u in us.items()}
    for name, u in us.items():
        mad = statistics.median(abs(x - med[name]) for x in u)
        say(f"  {name:<32} median {med[name] / n:9.2f} us per step   min {min(u) / n:9.2f}   max {max(u) / n:9.2f}   MAD {mad / n:7.2f}   "
            f"vs {base} {100 * (med[name] - med[base]) / med[base]:+6.2f} %")
    return med


def workload(a, batch, dim_x, dim_y, members, iters, radius):
    n = a.steps
    mask = disc(dim_x, dim_y, radius)
    what = f"batch of {members} x ({dim_x} x {dim_y})" if batch else f"context of {dim_x} x {dim_y}"
    say(f"{what}, a disc of radius {radius}, step_n({n}) of {iters} iterations, {a.warmup} warm-up and {a.reps} timed rounds, the configurations "
        f"alternating, host clock around call + synchronize:")
    # ---- the parent's library against this one, no recorder: --objects batches (contexts) of each, made in turn
    libs = {"this": capi.LIB_PATH}
    if a.parent:
        libs["parent"] = os.path.abspath(a.parent)
    raws = [(name, k, Raw(path, batch, dim_x, dim_y, members, mask)) for k in range(a.objects) for name, path in libs.items()]
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
        say(f"  (a) {name:<7} no recorder, {a.objects} objects: median {per_lib[name][0]:9.2f} us per step   min {min(every):9.2f}   max {max(every):9.2f}   "
            f"medians of the objects {', '.join(f'{m:.2f}' for m in meds)}")
    if a.parent:
        med, lo, hi, meds = per_lib["parent"]
        say(f"  spread of (a) parent: over the objects' medians {max(meds) - min(meds):.2f} us per step, over its rounds and objects max - min = {hi - lo:.2f}")
        gap = per_lib["this"][0] - med
        verdict = "inside" if abs(gap) <= hi - lo else "OUTSIDE"
        say(f"  this - parent = {gap:+.2f} us per step ({100 * gap / med:+.2f} %): {verdict} the parent's max - min of {hi - lo:.2f}")
    else:
        say("  the parent's library: not measured (no --parent)")
    for _, _, r in raws:
        r.close()
    if a.parent:   # (in the stream of (20, 3), as the recorders below)
        samples_against_parent(a, say, batch, dim_x, dim_y, members, iters, mask,
                               {"(b) step, a torque sample": ("torque",), "(c) step, a loads sample": ("loads",), "(d) step, a friction sample": ("friction",),
                                "(e) step, loads and friction": ("loads", "friction")}, velocity=(20.0, 3.0), pivot=(dim_x // 2, dim_y // 2))
    # ---- the recorders and the sampler alone
    def make():
        s = sfl.BatchSolver(dim_x, dim_y, members) if batch else sfl.Solver(dim_x, dim_y)
        s.setup_sketch_fields()
        # (the sketch's fluid is at rest, and a face whose product is zero skips its LDS atomic in torque.hip: the samplers are
        # timed in a stream past the disc, where pressures, velocities and products are not zero)
        v = np.zeros(((members,) if batch else ()) + (dim_y, dim_x, 2), np.float32)
        v[..., 0], v[..., 1] = 20.0, 3.0
        s.upload(capi.FIELD_VELOCITY, v)
        s.set_solids(mask)
        s.step_n(2, DT, DX, iters, OMEGA)
        return s

    plain, tq, lo_, fr, both = make(), make(), make(), make(), make()
    for s in (plain, tq):
        s.set_body_pivots(np.array([[dim_x // 2, dim_y // 2]], np.float64))

    def torque_recorded():
        tq.torque_start(1, n)
        tq.step_n(n, DT, DX, iters, OMEGA)

    def loads_recorded():
        lo_.loads_start(1, n)
        lo_.step_n(n, DT, DX, iters, OMEGA)

    def friction_recorded():
        fr.friction_start(1, n)
        fr.step_n(n, DT, DX, iters, OMEGA)

    def both_recorded():
        both.loads_start(1, n)
        both.friction_start(1, n)
        both.step_n(n, DT, DX, iters, OMEGA)

    def sampled():
        for _ in range(n):
            plain.torque()

    A, Bt, Cl, Df, E, Fs = ("(a) step, no recorder", "(b) step, a torque sample", "(c) step, a loads sample", "(d) step, a friction sample",
                            "(e) step, loads and friction", "(f) torque() alone, synchronous")
    runs = {A: (lambda: plain.step_n(n, DT, DX, iters, OMEGA), plain.synchronize), Bt: (torque_recorded, tq.synchronize),
            Cl: (loads_recorded, lo_.synchronize), Df: (friction_recorded, fr.synchronize), E: (both_recorded, both.synchronize),
            Fs: (sampled, plain.synchronize)}
    us = {name: [] for name in runs}
    for k in range(a.warmup + a.reps):
        for name, (call, sync) in runs.items():
            t = timed(call, sync)
            if k >= a.warmup:
                us[name].append(t)
    med = report(us, n, A)
    cost, yard, spread = (med[Bt] - med[A]) / n, (med[E] - med[A]) / n, (max(us[E]) - min(us[E])) / n
    say(f"  on the stream a torque sample costs (b) - (a) = {cost:+.2f} us per step; a loads sample (c) - (a) = {(med[Cl] - med[A]) / n:+.2f}, "
        f"a friction sample (d) - (a) = {(med[Df] - med[A]) / n:+.2f}, the two together (e) - (a) = {yard:+.2f}")
    say(f"  torque - (loads and friction) = {cost - yard:+.2f} us per step: {'no more than' if cost - yard <= spread else 'MORE THAN'} "
        f"the two together beyond the spread of (e)'s rounds, max - min = {spread:.2f}")
    recs = tq.torque_history()
    say(f"  (the last sample: faces {int(recs[-1, 0, 0]['faces'])}, max_arm2 {int(recs[-1, 0, 0]['max_arm2'])}, pressure and friction torque at nu = 1: "
        f"{float(recs[-1, 0, 0]['mp']) * 2.0 ** (int(recs[-1, 0, 0]['exp2_p']) - 1):.6g}, {float(recs[-1, 0, 0]['mf']) * 2.0 ** (int(recs[-1, 0, 0]['exp2_f']) - 1):.6g})")
    for s in (plain, tq, lo_, fr, both):
        s.close()
    say()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="libsfl_hip.so of the parent commit: (a) is run on it too")
    ap.add_argument("--reps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--objects", type=int, default=4, help="batches (contexts) per library in the comparison with the parent")
    ap.add_argument("--only", choices=["batch", "context"], default=None)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/torque_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    if a.only != "context":
        workload(a, True, 61, 81, 1024, 20, 8)
    if a.only != "batch":
        workload(a, False, 2048, 2048, 1, 40, 256)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
