#!/usr/bin/env python3
"""Throughput of batches (sfl_batch_*): B independent members of one small grid stepped by one launch per step.

    python tools/batch_throughput.py --size 61 81 --iters 20 [--batches 1 64 256 1024 4096] [--steps K] [--warmup W] [--check]
                                     [--each uniform | spread | spread-sorted] [--until TOL [--every C] [--omega-mix]]
                                     [--large]

Every member starts from the sketch's fields (setup_sketch_fields) with a drag of its own in the first warm-up step, so
that no two members hold the same numbers.  Per B: W warm-up steps, then step_n(K) timed with a host clock around a
synchronize.  One JSON line per B with
  * member-steps/s and microseconds per batch step (one launch that steps every member);
  * the bytes model: 48 B per cell and member-step (velocity in + out 16, dye in + out 24, divergence 4, pressure 4), as
    GB/s and as a fraction of the MI355X's 8 TB/s;
  * the ratio to ONE context's sfl_step_n rate, measured in this process on the same grid, iterations and step count;
  * the ratio to the unmodified reference on one host core: its step at this size as committed in
    profiles/r06_bench_c1_61x81.json (cited, not re-measured; 61 x 81 at 20 iterations only).
--each: step through step_n_each (parameters of each member's own, and the update norm at the end of every step) instead
of step_n.  uniform = every member at --iters; spread = each member's iters drawn from 5 .. 80 with a fixed seed (dt, dx
and omega as always), in that natural order; spread-sorted = the same multiset of iters, members sorted by iters
descending (does the order in which workgroups are handed out matter?).  Every line carries sum_iters, the SOR iterations
of one batch step over all members, so that a line can be set against a uniform run of the same total work.
--until TOL: step through step_n_until -- the members' iters (--iters, or --each's) become caps, and every member's solve
stops at the first check, made in front of every C-th iteration (--every, default 4), whose update norm is <= TOL.  TOL =
-1 stops nothing: the arithmetic of step_n_each with the checks still made, which prices a check.  --omega-mix gives each
member an omega drawn from 1.0 .. 1.99 with a fixed seed instead of 1.96 (a parameter study whose members need different
numbers of iterations).  Such a line carries iters_run_last_step and iters_run_timed: the iterations the members
really ran in the last step and over the K timed steps, against sum_iters (one step at the caps).
--large: a batch of large members (sfl_batch_create_large: up to 20224 cells per member, 8 B of LDS per cell) instead of
sfl_batch_create's (6144 cells, 16 B per cell); a shape both take prices the layout.  Every line carries "large".
--check: after the timed run, members {0, 1, B/2, B - 1} against single contexts given the same start, drag, steps and
that member's parameters -- velocity, divergence, pressure and dye bit for bit."""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfl = importlib.import_module("esp32-fluid-simulation_amd")

DT, DX, OMEGA = np.float32(1 / 30.0), 1.0, np.float32(1.96)
SPREAD_ITERS, SPREAD_SEED = (5, 80), 20261016   # --each spread: iters uniform on [5, 80]
MIX_OMEGAS = (1.0, 1.5, 1.8, 1.9, 1.96, 1.99)   # --omega-mix: drawn with SPREAD_SEED + 1
BYTES_PER_CELL_STEP = 48
HBM_BYTES_PER_S = 8e12
REFERENCE_PROFILE = os.path.join(ROOT, "profiles", "r06_bench_c1_61x81.json")


def reference_step_ms(dim_x, dim_y, iters):
    """The reference's step on one host core at this size, from the committed C1 bench line (None if not measured)."""
    with open(REFERENCE_PROFILE) as f:
        line = json.load(f)
    for entry in line["cpu_baseline"]["sim_step_per_operator"]:
        if tuple(entry["grid"]) == (dim_x, dim_y) and entry["iters"] == iters:
            return entry["ms"]["step"]
    return None


def drag_of(member, dim_x, dim_y):
    """A drag of this member's own: (cell, velocity)."""
    return (member % dim_x, (member // dim_x) % dim_y), (10.0 + member % 7, -5.0 + member % 11)


def time_context(dim_x, dim_y, iters, warmup, steps):
    with sfl.Solver(dim_x, dim_y) as s:
        s.setup_sketch_fields()
        s.step_n(warmup, DT, DX, iters, OMEGA)
        s.synchronize()
        t0 = time.perf_counter()
        s.step_n(steps, DT, DX, iters, OMEGA)
        s.synchronize()
        return steps / (time.perf_counter() - t0)


def member_iters(each, batch, iters):
    """iters of every member: --iters for all (step_n and --each uniform), or the seeded spread, natural or sorted."""
    if each in (None, "uniform"):
        return np.full(batch, iters, np.int32)
    drawn = np.random.default_rng(SPREAD_SEED).integers(SPREAD_ITERS[0], SPREAD_ITERS[1] + 1, batch).astype(np.int32)
    return np.sort(drawn)[::-1].copy() if each == "spread-sorted" else drawn


def check_members(b, members, dim_x, dim_y, iters, total_steps):
    """iters: one value per member of the batch."""
    bad = []
    with sfl.Solver(dim_x, dim_y) as s:
        for m in members:
            s.setup_sketch_fields()
            cell, vel = drag_of(m, dim_x, dim_y)
            s.queue_forces(np.array([cell], np.int32), np.array([vel], np.float32))
            s.step_n(total_steps, DT, DX, int(iters[m]), OMEGA)
            s.synchronize()
            for field in (sfl.capi.FIELD_VELOCITY, sfl.capi.FIELD_DIVERGENCE, sfl.capi.FIELD_PRESSURE, sfl.capi.FIELD_COLOR):
                got = b.download(field, m, 1)[0]
                want = s.download(field)
                if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
                    bad.append((m, field))
    return bad


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--size", type=int, nargs=2, default=[61, 81], metavar=("DIM_X", "DIM_Y"))
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 64, 256, 1024, 4096])
    ap.add_argument("--steps", type=int, default=200, help="timed steps per batch (K)")
    ap.add_argument("--warmup", type=int, default=20, help="untimed steps before them (W)")
    ap.add_argument("--check", action="store_true", help="compare members with single contexts after the timed run")
    ap.add_argument("--each", choices=["uniform", "spread", "spread-sorted"], default=None,
                    help="step through step_n_each with these per-member iters (default: step_n)")
    ap.add_argument("--until", type=float, default=None, metavar="TOL",
                    help="step through step_n_until: iters are caps, a solve stops at update norm <= TOL (-1: never)")
    ap.add_argument("--every", type=int, default=4, help="with --until: a check in front of every C-th iteration")
    ap.add_argument("--omega-mix", action="store_true", help="with --until: each member's omega drawn from 1.0 .. 1.99")
    ap.add_argument("--large", action="store_true", help="a batch of large members (sfl_batch_create_large)")
    ap.add_argument("--label", default="", help="free text carried into every line (e.g. the build variant)")
    a = ap.parse_args()
    if a.until is None and a.omega_mix:
        ap.error("--omega-mix needs --until")
    if a.until is not None and a.check:
        ap.error("--check compares with contexts at fixed iterations: not with --until")
    dim_x, dim_y = a.size
    cells = dim_x * dim_y
    context_rate = time_context(dim_x, dim_y, a.iters, a.warmup, a.steps)
    ref_ms = reference_step_ms(dim_x, dim_y, a.iters)
    ok = True
    for batch in a.batches:
        with sfl.BatchSolver(dim_x, dim_y, batch, large=a.large) as b:
            b.setup_sketch_fields()
            drags = [drag_of(m, dim_x, dim_y) for m in range(batch)]
            b.queue_forces(np.arange(batch, dtype=np.int32), [d[0] for d in drags], [d[1] for d in drags])
            iters = member_iters(a.each, batch, a.iters)
            if a.until is not None:
                omega = OMEGA
                if a.omega_mix:
                    omega = np.random.default_rng(SPREAD_SEED + 1).choice(np.array(MIX_OMEGAS, np.float32), batch)
                prm = sfl.member_params(batch, DT, DX, iters, omega)
                stops = sfl.member_stops(batch, a.until, a.every)
                step_n = lambda n: b.step_n_until(n, prm, tol=stops)
            elif a.each:
                prm = sfl.member_params(batch, DT, DX, iters, OMEGA)
                step_n = lambda n: b.step_n_each(n, prm)
            else:
                step_n = lambda n: b.step_n(n, DT, DX, a.iters, OMEGA)
            step_n(a.warmup)
            b.synchronize()
            t0 = time.perf_counter()
            step_n(a.steps)
            b.synchronize()
            seconds = time.perf_counter() - t0
            rate = batch * a.steps / seconds
            gbs = BYTES_PER_CELL_STEP * cells * rate / 1e9
            line = {
                "grid": [dim_x, dim_y], "iters": a.iters if a.each in (None, "uniform") else "%d..%d" % SPREAD_ITERS,
                "call": "step_n_until" if a.until is not None else "step_n_each" if a.each else "step_n", "each": a.each, "sum_iters": int(iters.sum()),
                "mean_iters": float(iters.mean()), "batch": batch, "large": b.large, "steps": a.steps, "warmup": a.warmup,
                "member_steps_per_s": rate, "us_per_batch_step": seconds / a.steps * 1e6,
                "bytes_model_per_member_step": BYTES_PER_CELL_STEP * cells, "gb_per_s": gbs,
                "frac_of_8tb_s": gbs * 1e9 / HBM_BYTES_PER_S,
                # (one context at --iters: no yardstick for a batch whose members differ)
                "context_steps_per_s": context_rate, "x_one_context": rate / context_rate if len(set(iters)) == 1 else None,
                "x_reference_core": rate * ref_ms / 1e3 if ref_ms and len(set(iters)) == 1 else None,
                "reference_step_ms": ref_ms, "reference_source": "profiles/r06_bench_c1_61x81.json cpu_baseline" if ref_ms else None,
            }
            if a.until is not None:
                ran = b.iterations().astype(np.int64)
                line.update({"until": a.until, "every": a.every, "omega_mix": a.omega_mix,
                             "iters_run_last_step": int(ran[:, 0].sum()), "iters_run_timed": int(ran[:, 1].sum())})
                for key in ("x_one_context", "x_reference_core"):   # (one context at --iters is no yardstick for it)
                    line[key] = None
            if a.label:
                line["label"] = a.label
            if a.check:
                members = sorted({0, min(1, batch - 1), batch // 2, batch - 1})
                bad = check_members(b, members, dim_x, dim_y, iters, a.warmup + a.steps)
                line["check_members"] = members
                line["check_bit_exact"] = not bad
                if a.each:   # the update norm of the last step, as the batch reports it
                    line["residual_of_checked_members"] = [float(r) for r in b.residual()[members]]
                ok = ok and not bad
            print(json.dumps(line), flush=True)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
