#!/usr/bin/env python3
"""What a history costs a step call, and what it saves: the numbers of profiles/history.txt.

In one process, warmed, alternating, host clock around the calls and the synchronise that ends them (a batch's stream is
the library's own: no event of the caller's can be recorded on it), N >= 200 steps per timed window:

  (a)  step_n(N), no history          what the call launched before there were histories -- the comparison
  (b)  step_n(N), history of every 1  one sample launch behind every step; the history is restarted (no allocation: it does
                                      not grow) before every timed call
  (a') (b')                           the same two for step_n_until(N) with a tolerance that never stops a member: the step
                                      call of (c)
  (c)  the twin loop                  N x (step_n_until(1); flow_stats; residual; iterations): what a curve cost before -- four
                                      synchronous calls and at least three host waits per step

  small   61 x 81 x 1024 members, 20 iterations
  large   128 x 128 x 256 members of sfl_batch_create_large, 20 iterations

(b) - (a) over N is the sampler's cost per sample where it runs: behind the step that wrote the fields.  Beside it
tools/history_pass_probe (built from tools/history_pass_probe.hip and the product's sources, here) takes the same sample
on a stream of its own by the sampler and by the passes that existed before -- launch_flow_stats with its memset and both
launches; an update norm per member range is not expressible with update_norm.hip's launch, which takes one field, so the
old way is timed WITHOUT it, and once more with the COST of one such pass over the batch's pressure as a single field (not
a result) -- device events around 200 samples back to back.  Median, minimum and maximum over --reps.

usage: python3 tools/history_probe.py [--build-only] [--reps R] [--steps N] [--out profiles/history.txt]"""
import argparse
import importlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sfl = importlib.import_module("esp32-fluid-simulation_amd")

PASS_PROBE = os.path.join(ROOT, "tools", "history_pass_probe")
CSRC = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc")
OUT = []
DT, DX, ITERS, OMEGA = 0.05, 1.0, 20, 1.9


def say(text=""):
    print(text)
    sys.stdout.flush()
    OUT.append(text)


def line(name, us, per):
    med = statistics.median(us)
    return f"  {name:<44} median {med:10.1f} us   min {min(us):10.1f}   max {max(us):10.1f}   per step {med / per:8.2f} us"


def timed(call, sync):
    sync()
    t = time.perf_counter()
    call()
    sync()
    return (time.perf_counter() - t) * 1e6


def build_pass_probe(rebuild=False):
    """The stand-alone half, compiled from the product's own kernels (--build-only makes it afresh, on a box without a
    GPU too); None where there is no binary and no compiler."""
    sources = [os.path.join(ROOT, "tools", "history_pass_probe.hip"), os.path.join(CSRC, "history.hip"), os.path.join(CSRC, "flow_stats.hip"),
               os.path.join(CSRC, "update_norm.hip")]
    if os.path.exists(PASS_PROBE) and not rebuild:
        return PASS_PROBE
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", *sources, "-o", PASS_PROBE], check=True)
    return PASS_PROBE


def shape(a, name, dim_x, dim_y, members, large):
    n = a.steps
    prm = sfl.member_params(members, DT, DX, ITERS, OMEGA)
    never = sfl.member_stops(members, -1.0, 4)
    make = lambda: sfl.BatchSolver(dim_x, dim_y, members, large=large)
    with make() as plain, make() as hist, make() as plain_u, make() as hist_u, make() as twin:
        for b in (plain, hist, plain_u, hist_u, twin):
            b.setup_sketch_fields()
            b.queue_forces(list(range(members)), [(20, 40)] * members, [(-12.0, 30.0)] * members)
            b.step_n_each(2, prm)
        for b in (hist, hist_u):
            b.history_start(1, n)   # (the allocation: every later start keeps it)

        def loop():
            for _ in range(n):
                twin.step_n_until(1, prm, tol=never)
                twin.flow_stats(DX)
                twin.residual()
                twin.iterations()

        variants = {
            "(a)  step_n, no history": (lambda: None, lambda: plain.step_n(n, DT, DX, ITERS, OMEGA), plain.synchronize),
            "(b)  step_n, history of every 1": (lambda: hist.history_start(1, n), lambda: hist.step_n(n, DT, DX, ITERS, OMEGA), hist.synchronize),
            "(a') step_n_until, no history": (lambda: None, lambda: plain_u.step_n_until(n, prm, tol=never), plain_u.synchronize),
            "(b') step_n_until, history of every 1": (lambda: hist_u.history_start(1, n), lambda: hist_u.step_n_until(n, prm, tol=never), hist_u.synchronize),
            "(c)  the twin loop of synchronous calls": (lambda: None, loop, twin.synchronize),
        }
        us = {v: [] for v in variants}
        for r in range(a.warmup + a.reps):
            for v, (prepare, call, sync) in variants.items():   # alternating: every round runs each variant once
                prepare()
                t = timed(call, sync)
                if r >= a.warmup:
                    us[v].append(t)
        say(f"{name}: {members} x ({dim_x} x {dim_y}){' large' if large else ''}, {ITERS} iterations, windows of {n} steps, {a.reps} rounds, host clock around "
            f"call + synchronize:")
        for v in variants:
            say(line(v, us[v], n))
        med = {v: statistics.median(u) for v, u in us.items()}
        keys = list(variants)
        for base, with_h in ((keys[0], keys[1]), (keys[2], keys[3])):
            diffs = [(h - p) / n for h, p in zip(us[with_h], us[base])]
            say(f"  {with_h[:4].strip()} - {base[:4].strip()}: {statistics.median(diffs):+7.2f} us per sample (round by round: min {min(diffs):+.2f}, max {max(diffs):+.2f}); "
                f"{100 * (med[with_h] - med[base]) / med[base]:+.1f} % of the step")
        say(f"  (c) / (b'): {med[keys[4]] / med[keys[3]]:.2f} x; (b') faster than (c) per step: {'yes' if med[keys[3]] < med[keys[4]] else 'NO'}")
        say(f"  a sample reads {28 * dim_x * dim_y * members / 1e6:.1f} MB (28 B per cell and member)")
        assert hist.history_info() == (n, n, n) and hist.history()["step"][-1, 0] == n
    probe = build_pass_probe()
    if probe is None:
        say("  tools/history_pass_probe: not built (no hipcc here): the passes of before were NOT measured")
        return
    r = subprocess.run([probe, str(dim_x), str(dim_y), str(members), str(a.reps), "200"], capture_output=True, text=True, timeout=600)
    say(f"  the same sample alone on a stream (tools/history_pass_probe, exit {r.returncode}):")
    for text in (r.stdout + r.stderr).splitlines():
        say("  " + text)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    ap.add_argument("--build-only", action="store_true", help="compile tools/history_pass_probe and stop (needs no GPU)")
    a = ap.parse_args()
    if a.build_only:
        raise SystemExit(0 if build_pass_probe(rebuild=True) else "no hipcc here")
    if a.reps < 7 or a.steps < 200:
        raise SystemExit("at least 7 repetitions of at least 200 steps: fewer measure the clock and the scheduler")
    if sfl.device_count() < 1:
        raise SystemExit("needs a GPU: nothing here is measured without one")
    say("# tools/history_probe.py " + " ".join(sys.argv[1:]))
    say(f"# device: {sfl.device_info(0)[0]}")
    shape(a, "small", 61, 81, 1024, False)
    say()
    shape(a, "large", 128, 128, 256, True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(OUT) + "\n")
