"""The timeline of queued forces (include/sfl.h, "the timeline rule"): forces queued for step `step` of the steps to come,
on contexts (sfl_queue_forces_at, sfl_queue_drags_at) and batches (sfl_batch_queue_forces_at), one launch per step.

The yardstick is always code that existed before there was a timeline: a twin object stepped one step at a time, with that
step's records queued by the old step-0 calls in front of each step -- and the oracle's operators where the shape is small.
All four fields are compared bit for bit.  tests/test_batch_play.py has the calls that run their steps in one launch.

The CPU tests need no GPU: the argument checks run before any device is touched, and tests/cpp/timeline_driver.cpp runs the
host side of contexts and batches over a runtime that lives on the host."""
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_bit_equal, random_fields
from test_batch import DT, FIELDS, OMEGA, download_all, member_fields, upload_members

TIMELINE_SYMBOLS = ["sfl_queue_forces_at", "sfl_queue_drags_at", "sfl_forces_pending", "sfl_forget_forces",
                    "sfl_batch_queue_forces_at", "sfl_batch_forces_pending", "sfl_batch_forget_forces"]
F = (0, 2, 3, 1)   # velocity, divergence, pressure, colour: the order of FIELDS


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_timeline_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in TIMELINE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    for cls in (sfl.Solver, sfl.BatchSolver):
        assert inspect.signature(cls.queue_forces).parameters["step"].default == 0
        assert hasattr(cls, "forces_pending") and hasattr(cls, "forget_forces")
    assert inspect.signature(sfl.Solver.queue_drags).parameters["step"].default == 0


def test_null_handles_are_refused_before_any_gpu_is_touched(sfl):
    lib = sfl.capi.lib()
    i = C.c_int(5)
    cells, vel, members = (C.c_int * 2)(1, 1), (C.c_float * 2)(1.0, 2.0), (C.c_int * 1)(0)
    drag = sfl.capi.Drag(1, 1, 1.0, 2.0)
    calls = [
        lambda: lib.sfl_queue_forces_at(None, 0, cells, vel, 1),
        lambda: lib.sfl_queue_drags_at(None, 0, C.cast(C.pointer(drag), C.c_void_p), 1),
        lambda: lib.sfl_forces_pending(None, C.byref(i), C.byref(i)),
        lambda: lib.sfl_forget_forces(None),
        lambda: lib.sfl_batch_queue_forces_at(None, 0, members, cells, vel, 1),
        lambda: lib.sfl_batch_forces_pending(None, C.byref(i), C.byref(i)),
        lambda: lib.sfl_batch_forget_forces(None),
    ]
    assert len(calls) == len(TIMELINE_SYMBOLS)
    for call in calls:
        assert call() == sfl.capi.ERR_INVALID
    assert i.value == 5


def test_the_host_side_of_the_timeline_on_contexts_and_batches():
    """`make -C tests/cpp -f timeline.mk`: tests/cpp/timeline_driver.cpp, a stand-alone program under AddressSanitizer + UBSan.
    NULL, step < 0, a member outside the batch and a drag outside the domain are refused with nothing queued; forces_pending
    after queueing at steps {0, 3, 3, 7}; the shift across step calls of every kind, on two linked ranks too; refused step
    calls (an argument, a full recorder) leave the timeline as it was; forget; and, from launchers that log what they are
    handed, the records every step of every launch applies -- one launch per step, or one per call (cut at the frames)."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "timeline.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "timeline_driver")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]


# ---- GPU ----------------------------------------------------------------------------------------------
def script(n, dim_x, dim_y):
    """The script used throughout, {step: [(cell, velocity), ...]} for a call of n >= 2 steps: records at step 0 and at the
    last step, none at step 1 (n >= 4), at step n - 2 two records on one cell (the later must win) and one cell outside the domain
    (skipped), and one record at step n + 2, which must survive the call."""
    a, b = (dim_x // 2, dim_y // 2), (dim_x - 1, dim_y - 1)
    s = {}
    s.setdefault(0, []).append((a, (55.0, -35.0)))
    s.setdefault(max(n - 2, 0), []).extend([((1, 1), (10.0, 10.0)), ((dim_x, 1), (99.0, 99.0)), ((1, 1), (-8.0, 6.0))])
    s.setdefault(n - 1, []).extend([(b, (-20.0, 12.5)), ((0, 0), (3.0, 4.0))])
    s.setdefault(n + 2, []).append((a, (7.0, -7.0)))
    assert n < 4 or 1 not in s   # (a call of 2 or 3 steps has no room for a step without records)
    return s


def oracle_steps(oracle, v, c, records_of_step, n, dt=DT, dx=1.0, iters=5, omega=OMEGA):
    """n steps of the oracle's operators, the records of step k written between the velocity advection and the divergence
    (ino:264-269; tests/test_batch.py oracle_forced_step).  Returns (v, div, p, colour)."""
    d = p = None
    for k in range(n):
        va = oracle.advect_vec2f(v, v, dt, True)
        for (i, j), u in records_of_step.get(k, ()):
            if 0 <= i < v.shape[1] and 0 <= j < v.shape[0]:
                va[j, i] = u
        d = oracle.divergence(va, dx)
        p = oracle.poisson_solve(d, dx, iters, omega)
        v = oracle.subtract_gradient(va, p, dx)
        c = oracle.advect_vec3uq32(c, v, dt, False)
    return v, d, p, c


def queue(s, records, step=None):
    if records:
        kw = {} if step is None else {"step": step}
        s.queue_forces(np.array([r[0] for r in records], np.int32), np.array([r[1] for r in records], np.float32), **kw)


def context_case(sfl, oracle, dim_x, dim_y, nranks, n=4, iters=4, extra=()):
    v, c, _ = random_fields(dim_x, dim_y, 77 + dim_x, 60.0)
    sc = script(n, dim_x, dim_y)
    for step, records in extra:
        sc.setdefault(step, []).extend(records)
    make = lambda: [sfl.Solver(dim_x, dim_y, 0, r, nranks) for r in range(nranks)]
    got_slabs, twin_slabs = make(), make()
    try:
        for slabs in (got_slabs, twin_slabs):
            if nranks > 1:
                sfl.Solver.link_group(slabs)
            for s in slabs:
                s.upload(0, v[s.row_begin:s.row_end])
                s.upload(1, c[s.row_begin:s.row_end])
        got, twin = got_slabs[0], twin_slabs[0]
        cat = lambda slabs: [np.concatenate([s.download(f) for s in slabs], axis=0) for f in F]
        assert got.forces_pending() == (0, -1)
        for step, records in sc.items():   # steps in an order of their own; step 0 by the old call
            queue(got, records, None if step == 0 else step)
        assert got.forces_pending() == (sum(len(r) for r in sc.values()), n + 2)
        got.step_n(n, DT, 1.0, iters, OMEGA)
        assert got.forces_pending() == (1, 2)
        for k in range(n):
            queue(twin, sc.get(k))
            twin.step_n(1, DT, 1.0, iters, OMEGA)
        got.synchronize(), twin.synchronize()
        first = cat(got_slabs)
        for name, a, b in zip(FIELDS, first, cat(twin_slabs)):
            assert_bit_equal(a, b, f"{name} after step_n({n}) against one step at a time")
        if oracle is not None:
            for name, a, b in zip(FIELDS, first, oracle_steps(oracle, v, c, sc, n, iters=iters)):
                assert_bit_equal(a, b, f"{name} after step_n({n}) against the oracle")
        # the record left over lands in step 2 of the next call: a step with records between two without
        got.step_n(n, DT, 1.0, iters, OMEGA)
        assert got.forces_pending() == (0, -1)
        for k in range(n):
            queue(twin, sc[n + 2] if k == 2 else None)
            twin.step(DT, 1.0, iters, OMEGA)
        got.synchronize(), twin.synchronize()
        for name, a, b in zip(FIELDS, cat(got_slabs), cat(twin_slabs)):
            assert_bit_equal(a, b, f"{name} after the second step_n({n})")
        # forget: what was queued is never applied
        queue(got, sc[0], 1)
        got.forget_forces()
        assert got.forces_pending() == (0, -1)
        got.step_n(2, DT, 1.0, iters, OMEGA)
        twin.step_n(2, DT, 1.0, iters, OMEGA)
        got.synchronize(), twin.synchronize()
        for name, a, b in zip(FIELDS, cat(got_slabs), cat(twin_slabs)):
            assert_bit_equal(a, b, f"{name} after forget")
    finally:
        for s in got_slabs + twin_slabs:
            s.close()


@pytest.mark.gpu
def test_a_context_on_the_one_workgroup_path(sfl, oracle):
    context_case(sfl, oracle, 61, 81, 1)


@pytest.mark.gpu
def test_a_context_with_step_seams(sfl):
    """160 x 128 is above kAdvectTiledMinCells: step_n joins the steps without records by its seam kernel."""
    with sfl.Solver(160, 128) as s:
        assert s.get_option(sfl.capi.OPT_STEP_SEAMS) == 1
    context_case(sfl, None, 160, 128, 1)


@pytest.mark.gpu
def test_two_virtual_ranks_with_a_record_next_to_the_cut(sfl):
    rows = sfl.slab_rows(128, 2, 0)[1]   # the first row of rank 1
    context_case(sfl, None, 160, 128, 2, extra=[(2, [((40, rows), (30.0, -30.0)), ((41, rows - 1), (-25.0, 15.0))])])


@pytest.mark.gpu
def test_drags_at_a_step(sfl):
    dim_x, dim_y = 61, 81
    drags = [(40, 20, 30.0, -12.0), (5, 50, -25.0, 9.0)]
    v, c, _ = random_fields(dim_x, dim_y, 5, 40.0)
    with sfl.Solver(dim_x, dim_y) as s, sfl.Solver(dim_x, dim_y) as twin:
        for x in (s, twin):
            x.upload(0, v), x.upload(1, c)
        s.queue_drags(drags, step=2)
        with pytest.raises(sfl.SflError):
            s.queue_drags([(dim_y, 0, 1.0, 1.0)], step=1)   # coords.x addresses row j = dim_y
        with pytest.raises(sfl.SflError):
            s.queue_drags(drags, step=-1)
        assert s.forces_pending() == (2, 2)
        s.step_n(3, DT, 1.0, 5, OMEGA)
        twin.step_n(2, DT, 1.0, 5, OMEGA)
        twin.queue_drags(drags)
        twin.step(DT, 1.0, 5, OMEGA)
        for name, f in zip(FIELDS, F):
            assert_bit_equal(s.download(f), twin.download(f), name)


def batch_script(n, dim_x, dim_y):
    """The script for B = 3: member 0 has the script's records, member 2 two of its own, member 1 none at all."""
    sc = script(n, dim_x, dim_y)
    per_step = {k: [(0, cell, vel) for cell, vel in r] for k, r in sc.items()}
    per_step[0].append((2, (dim_x - 1, 0), (-40.0, 22.0)))
    per_step[n - 1].insert(0, (2, (0, dim_y - 1), (14.0, 9.0)))
    return per_step


def queue_batch(b, records, step=None):
    if records:
        kw = {} if step is None else {"step": step}
        b.queue_forces([r[0] for r in records], [r[1] for r in records], [r[2] for r in records], **kw)


def assert_batches_equal(b, twin, what):
    for name, got, want in zip(FIELDS, download_all(b), download_all(twin)):
        assert_bit_equal(got, want, f"{what}: {name}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (96, 96)])
def test_a_large_batch_takes_one_launch_per_step(sfl, dim_x, dim_y):
    batch, n, iters = 3, 4, 4
    fields = [member_fields(dim_x, dim_y, 40 + m, 40.0) for m in range(batch)]
    sc = batch_script(n, dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b, sfl.BatchSolver(dim_x, dim_y, batch, large=True) as twin:
        upload_members(b, fields), upload_members(twin, fields)
        for step in sorted(sc, reverse=True):
            queue_batch(b, sc[step], None if step == 0 else step)
        assert b.forces_pending() == (sum(len(r) for r in sc.values()), n + 2)
        b.step_n(n, DT, 1.0, iters, OMEGA)
        assert b.forces_pending() == (1, 2)
        for k in range(n):
            queue_batch(twin, sc.get(k))
            twin.step_n(1, DT, 1.0, iters, OMEGA)
        assert_batches_equal(b, twin, f"step_n({n})")
        b.step_n(3, DT, 1.0, iters, OMEGA)
        assert b.forces_pending() == (0, -1)
        twin.step_n(2, DT, 1.0, iters, OMEGA)
        queue_batch(twin, sc[n + 2])
        twin.step_n(1, DT, 1.0, iters, OMEGA)
        assert_batches_equal(b, twin, "the record left over, in step 2 of the next call")


@pytest.mark.gpu
def test_step_n_until_with_a_negative_tol_is_the_each_call(sfl):
    """The per-step path of a small batch: *_until with tol < 0 never stops early -- the *_each call of the twin, one step
    at a time, bit for bit, the update norm included."""
    dim_x, dim_y, batch, n = 61, 81, 3, 4
    fields = [member_fields(dim_x, dim_y, 60 + m, 40.0) for m in range(batch)]
    prm = sfl.member_params(batch, [DT, DT / 2, DT * 2], [1.0, 0.5, 2.0], [3, 5, 4], [1.96, 1.5, 1.9])
    stops = sfl.member_stops(batch, [-1.0] * batch, [2, 1, 3])
    sc = batch_script(n, dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.BatchSolver(dim_x, dim_y, batch) as twin:
        upload_members(b, fields), upload_members(twin, fields)
        for step, records in sc.items():
            queue_batch(b, records, step)
        b.step_n_until(n, prm, tol=stops)
        assert b.forces_pending() == (1, 2)
        for k in range(n):
            queue_batch(twin, sc.get(k))
            twin.step_n_each(1, prm)
        assert_batches_equal(b, twin, f"step_n_until({n})")
        assert_bit_equal(b.residual(), twin.residual(), "the update norm")
        assert b.iterations()[:, 0].tolist() == [3, 5, 4] and b.iterations()[:, 1].tolist() == [12, 20, 16]
        b.forget_forces()
        b.step_n_until(3, prm, tol=stops)
        twin.step_n_each(3, prm)
        assert_batches_equal(b, twin, "after forget")
