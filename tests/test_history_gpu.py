"""Histories on the GPU (csrc/history.hip behind sfl_batch_history_*, the streaming passes behind sfl_history_*; include/sfl.h
"HISTORIES").

Every case is seeded and built around a TWIN: the same inputs stepped by n x (a step call of one step; the statistics calls
that exist without histories) on a second batch or context.  Asserted everywhere: the records equal the twin's figures as raw
bytes, and the fields of the run with a history equal those of a run of the same calls without one, by the library's own
distance calls: all three counts zero <=> identical bits.  No tolerance anywhere: maxima over bit patterns and integer sums do
not depend on the order of reduction."""
import functools

import numpy as np
import pytest

from conftest import random_fields

pytestmark = pytest.mark.gpu

FV, FC, FDIV, FP = 0, 1, 2, 3       # SFL_FIELD_VELOCITY, SFL_FIELD_COLOR, SFL_FIELD_DIVERGENCE, SFL_FIELD_PRESSURE
FIELDS = (FV, FC, FDIV, FP)
DT, DX, ITERS, OMEGA = 0.05, 0.75, 6, 1.9
ERR_INVALID, ERR_STATE = -1, -5

# (dim_x, dim_y, members, large, recorded first, recorded count): the smallest shapes at which the sampler can go wrong
SHAPES = {
    "2x2": (2, 2, 3, False, 0, 3),            # every cell a corner
    "7x5": (7, 5, 4, False, 0, 4),            # fewer cells than threads
    "61x81": (61, 81, 5, False, 1, 3),        # dye bases at all four alignments; unrecorded members on both sides
    "64x96": (64, 96, 2, False, 0, 2),        # the largest small member
    "96x96-large": (96, 96, 3, True, 0, 3),
    "127x159-large": (127, 159, 2, True, 0, 2),   # 20193 cells, odd in both directions
}


def assert_no_distance(records, what):
    for name in ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ"):
        assert not np.any(records[name]), f"{what}: {name} {records[name]}"


def assert_records(got, want, what):
    """Raw bytes; the message names the first field that differs."""
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for name in got.dtype.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        assert g.tobytes() == w.tobytes(), f"{what}: {name}: got\n{g}\nwant\n{w}"
    raise AssertionError(f"{what}: the records differ outside their named fields")


@functools.lru_cache(maxsize=None)
def member_fields(dim_x, dim_y, batch, seed=0):
    """(velocity, dye, divergence, pressure) of every member: a velocity of up to +-20 cells per unit of time, a dye over
    the whole of UQ32's lower half, two scalars.  Shared: never written to."""
    per = [random_fields(dim_x, dim_y, 900 + 17 * m + dim_x + seed, vamp=20.0) for m in range(batch)]
    v, c, s = (np.stack([f[k] for f in per]) for k in range(3))
    p = np.random.default_rng(31 + dim_y + seed).standard_normal((batch, dim_y, dim_x)).astype(np.float32)
    for a in (v, c, s, p):
        a.setflags(write=False)
    return v, c, s, p


def batch_with(sfl, shape, held=None, batch=None):
    dim_x, dim_y, members, large = SHAPES[shape][:4]
    batch = batch or members
    b = sfl.BatchSolver(dim_x, dim_y, batch, large=large)
    for field, a in zip(FIELDS, held or member_fields(dim_x, dim_y, batch)):
        b.upload(field, a)
    return b


def member_rules(sfl, batch):
    """Different dt, dx, iters and omega per member, and a tolerance that stops members at different k (+inf: at once; a
    negative one: never; the others somewhere in between)."""
    m = np.arange(batch)
    prm = sfl.member_params(batch, DT * (1 + 0.5 * m), 0.6 + 0.3 * m, ITERS + 3 * (m % 3), 1.7 + 0.05 * m)
    stops = sfl.member_stops(batch, np.array([np.inf, -1.0, 2.0, 0.3, 0.02])[m % 5], 1 + m % 3)
    return prm, stops


def run_call(b, kind, n, prm, stops):
    if kind == "uniform":
        b.step_n(n, DT, DX, ITERS, OMEGA)
    elif kind == "each":
        b.step_n_each(n, prm)
    else:
        b.step_n_until(n, prm, tol=stops)


def twin_step(sfl, t, kind, prm, stops, step, first, count):
    """One step of the twin by calls that need no history, and the records those calls give for members [first, first + count)."""
    uniform = sfl.member_params(t.batch, DT, DX, ITERS, OMEGA)
    if kind == "uniform":   # (the *_each call with every member's parameters the same: the uniform call leaves no update norm to read)
        t.step_n_each(1, uniform)
    else:
        run_call(t, kind, 1, prm, stops)
    used = uniform if kind == "uniform" else prm
    rec = np.zeros(count, sfl.HISTORY_DTYPE)
    stats = t.flow_stats(DX if kind == "uniform" else used["dx"], first, count)
    for name in stats.dtype.names:
        rec[name] = stats[name]
    rec["update_norm"] = t.residual(first, count)
    rec["iterations"] = t.iterations(first, count)[:, 0] if kind == "until" else used["iters"][first:first + count]
    rec["step"] = step
    rec["dt"] = used["dt"][first:first + count]
    rec["dx"] = used["dx"][first:first + count]
    return rec


# ---- the three step calls, every shape ------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 3])
@pytest.mark.parametrize("kind", ["uniform", "each", "until"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_records_equal_the_twins_figures(sfl, shape, kind, every):
    """Two calls of 4 and 3 steps -- no multiples of every = 3 -- so the count carries across calls."""
    batch, first, count = SHAPES[shape][2], SHAPES[shape][4], SHAPES[shape][5]
    prm, stops = member_rules(sfl, batch)
    with batch_with(sfl, shape) as h, batch_with(sfl, shape) as plain, batch_with(sfl, shape) as t:
        h.history_start(every, 7 // every, first, count)
        for n in (4, 3):
            run_call(h, kind, n, prm, stops)
            run_call(plain, kind, n, prm, stops)
        assert h.history_info() == (7 // every, 7 // every, 7)
        got = h.history()
        want = []
        for step in range(1, 8):
            rec = twin_step(sfl, t, kind, prm, stops, step, first, count)
            if step % every == 0:
                want.append(rec)
        want = np.stack(want)
        assert got.shape == (7 // every, count)
        assert_records(got, want, f"{shape} {kind} every {every}")
        assert np.all(got["what"] == 3)
        if kind == "until" and count >= 3:   # (the case is about members that stop at different k)
            assert len(set(got["iterations"][0].tolist())) > 1, got["iterations"]
        assert_no_distance(h.distance(plain), "a history changes no field")
        assert_no_distance(h.distance(t), "... and the twin holds the same fields")
        if kind != "uniform":   # the reports keep their validity and their values
            assert h.residual().tobytes() == plain.residual().tobytes()
        if kind == "until":
            assert np.array_equal(h.iterations(), plain.iterations())
        h.history_stop()
        assert h.history_info() == (0, 0, 0)


# ---- a timeline that batch_play.hip runs in one launch, cut at the samples' steps -------------------------------------------
def queue_timeline(b, scale=1.0):
    """Forces in steps 0, 2 and 5, on different members."""
    b.queue_forces([0, 1], [[1, 1], [2, 3]], [[30.0 * scale, -10.0], [5.0, 25.0 * scale]], step=0)
    b.queue_forces([b.batch - 1], [[3, 2]], [[-40.0 * scale, 15.0]], step=2)
    b.queue_forces([1, 1], [[4, 1], [1, 3]], [[12.0, 12.0 * scale], [-7.0, 3.0]], step=5)


def twin_timeline(sfl, t, kind, prm, stops, first, count, every, n):
    """The twin steps one step at a time: its timeline is queued whole and consumed a step per call."""
    queue_timeline(t)
    want = []
    for step in range(1, n + 1):
        rec = twin_step(sfl, t, kind, prm, stops, step, first, count)
        if step % every == 0:
            want.append(rec)
    return np.stack(want)


@pytest.mark.parametrize("kind", ["uniform", "each"])
@pytest.mark.parametrize("shape", ["7x5", "61x81"])
def test_a_timeline_call_is_cut_at_the_samples_steps(sfl, shape, kind):
    """n = 7, every = 2, with and without a frame recorder of every = 3: records, frames and fields each equal their solo
    runs, and the records the twin's."""
    batch, first, count = SHAPES[shape][2], SHAPES[shape][4], SHAPES[shape][5]
    prm, stops = member_rules(sfl, batch)
    with batch_with(sfl, shape) as plain, batch_with(sfl, shape) as solo_h, batch_with(sfl, shape) as solo_r, \
            batch_with(sfl, shape) as both, batch_with(sfl, shape) as t:
        solo_h.history_start(2, 3, first, count)
        solo_r.record_start(every=3, scaling=1, capacity=2)
        both.history_start(2, 3, first, count)
        both.record_start(every=3, scaling=1, capacity=2)
        for b in (plain, solo_h, solo_r, both):
            queue_timeline(b)
            run_call(b, kind, 7, prm, stops)
            assert b.forces_pending() == (0, -1)
        want = twin_timeline(sfl, t, kind, prm, stops, first, count, 2, 7)
        assert_records(solo_h.history(), want, f"{shape} {kind}: history alone")
        assert_records(both.history(), want, f"{shape} {kind}: history and recorder")
        assert both.record_info() == (2, 2, 7) and both.history_info() == (3, 3, 7)
        assert np.array_equal(both.frames(), solo_r.frames())
        for b, what in ((solo_h, "history alone"), (solo_r, "recorder alone"), (both, "both"), (t, "the twin")):
            assert_no_distance(b.distance(plain), what)


def test_all_three_recorders_at_once(sfl):
    """History, frames, and following tracers with a trail: each equals its solo run."""
    shape = "61x81"
    dim_x, dim_y, batch, _, first, count = SHAPES[shape]
    prm, stops = member_rules(sfl, batch)
    xy = np.random.default_rng(3).uniform(-1.0, [dim_x, dim_y], (batch, 9, 2)).astype(np.float32)
    with batch_with(sfl, shape) as plain, batch_with(sfl, shape) as solo_h, batch_with(sfl, shape) as solo_r, \
            batch_with(sfl, shape) as solo_t, batch_with(sfl, shape) as all3:
        for b in (solo_h, all3):
            b.history_start(2, 4, first, count)
        for b in (solo_r, all3):
            b.record_start(every=3, scaling=1, capacity=2)
        for b in (solo_t, all3):
            b.set_tracers(xy, follow=True)
            b.trail_start(every=2, capacity=3)
        for b in (plain, solo_h, solo_r, solo_t, all3):
            queue_timeline(b)
            b.step_n_each(4, prm)
            b.step_n_until(3, prm, tol=stops)
        assert all3.history_info() == (3, 4, 7) and all3.record_info() == (2, 2, 7) and all3.trail_info() == (3, 3, 7)
        assert_records(all3.history(), solo_h.history(), "records")
        assert np.array_equal(all3.frames(), solo_r.frames())
        assert all3.trail().tobytes() == solo_t.trail().tobytes() and all3.tracers().tobytes() == solo_t.tracers().tobytes()
        for b in (solo_h, solo_r, solo_t, all3):
            assert_no_distance(b.distance(plain), "fields")


# ---- values ----------------------------------------------------------------------------------------------------------------
def queue_overflow(b):
    """Member batch - 1: +-3e38 on both sides of one cell, so that its divergence overflows."""
    b.queue_forces([b.batch - 1, b.batch - 1], [[1, b.dim_y - 2], [3, b.dim_y - 2]], [[3e38, 0.0], [-3e38, 0.0]], step=0)


@pytest.mark.parametrize("shape, batch", [("7x5", 4), ("61x81", 5), ("96x96-large", 4)])
def test_special_values(sfl, shape, batch):
    """Member 0's velocity holds one NaN: its three maxima are NaN and its neighbours' records are untouched.  Member 1's
    velocity is -0.0f only: the maxima are +0.0f.  Member 2's dye is 0xFFFFFFFF everywhere under a velocity of zero: the sums
    pass 2^32.  The last member's pressure is uploaded with an inf -- a step's solve starts from zero, so that inf does not
    live to the sample -- and its first step is given forces of +-3e38 around one cell: the divergence overflows, the solve
    leaves a pressure that is not finite, and the update norm follows the definition: a NaN.  Whatever the figures are, they
    are the twin's."""
    dim_x, dim_y = SHAPES[shape][:2]
    v, c, s, p = (a.copy() for a in member_fields(dim_x, dim_y, batch))
    v[0, dim_y // 2, dim_x // 2, 1] = np.nan
    v[1] = -0.0
    v[2] = 0.0
    c[2] = 0xFFFFFFFF
    p[-1, 1, 1] = np.inf
    held = (v, c, s, p)
    with batch_with(sfl, shape, held, batch) as h, batch_with(sfl, shape, held, batch) as plain, batch_with(sfl, shape, held, batch) as t, \
            batch_with(sfl, shape, None, batch) as clean:
        for b in (h, clean):
            b.history_start(1, 2, 0, batch)
        for b in (h, plain, t):
            queue_overflow(b)
        for b in (h, plain, clean):
            b.step_n(2, DT, DX, ITERS, OMEGA)
        got = h.history()
        want = np.stack([twin_step(sfl, t, "uniform", None, None, step, 0, batch) for step in (1, 2)])
        assert_records(got, want, shape)
        assert np.all(np.isnan(got["max_abs_vx"][:, 0])) and np.all(np.isnan(got["max_abs_vy"][:, 0])) and np.all(np.isnan(got["max_abs_div"][:, 0]))
        for name in ("max_abs_vx", "max_abs_vy", "max_abs_div"):
            assert np.all(got[name][:, 1].view(np.uint32) == 0), name   # |-0.0f| reports +0.0f
        assert np.all(got["dye_sum"][:, 2] > 2 ** 32), got["dye_sum"][:, 2]
        assert np.all(np.isnan(got["update_norm"][:, -1])), got["update_norm"]
        if batch > 4:   # a member whose fields are the clean ones: its record is the clean run's
            assert_records(got[:, 3], clean.history()[:, 3], "a neighbour of the special members")
        assert_no_distance(h.distance(plain), "fields")


# ---- capacity --------------------------------------------------------------------------------------------------------------
def test_a_call_one_sample_too_long_is_refused_whole(sfl):
    shape = "7x5"
    batch = SHAPES[shape][2]
    with batch_with(sfl, shape) as h, batch_with(sfl, shape) as plain:
        h.history_start(2, 2)
        h.step_n(3, DT, DX, ITERS, OMEGA)
        plain.step_n(3, DT, DX, ITERS, OMEGA)
        queue_timeline(h)
        pending = h.forces_pending()
        with pytest.raises(sfl.SflError) as e:
            h.step_n(3, DT, DX, ITERS, OMEGA)   # steps 4, 5, 6: samples 1 and 2, and there is room for one
        assert e.value.code == ERR_STATE and "room for 1 more" in str(e.value)
        for call in (lambda: h.step_n_each(3, DT), lambda: h.step_n_until(3, DT, tol=0.1)):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == ERR_STATE
        assert h.history_info() == (1, 2, 3) and h.forces_pending() == pending
        assert_no_distance(h.distance(plain), "a refused call steps nothing")
        first = h.history()
        h.history_start(2, 2)       # ... and the same call fits after a restart
        assert h.history_info() == (0, 2, 0)
        h.step_n(3, DT, DX, ITERS, OMEGA)
        queue_timeline(plain)
        plain.step_n(3, DT, DX, ITERS, OMEGA)
        assert h.history_info() == (1, 2, 3) and h.forces_pending() == (2, 2)   # (the records of step 5 wait, now at step 2)
        assert_no_distance(h.distance(plain), "the call after the restart")
        again = h.history()
        assert again.shape == (1, batch) and np.all(again["step"] == 2) and first.shape == (1, batch)
        with pytest.raises(sfl.SflError) as e:
            h.history_start(2, 2, first=2, count=batch)
        assert e.value.code == ERR_INVALID and h.history_info() == (1, 2, 3)   # a bad range leaves the history as it was


# ---- contexts --------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def context_fields(dim_x, dim_y):
    v, c, s = random_fields(dim_x, dim_y, 4100 + dim_x, vamp=20.0)
    p = np.random.default_rng(11 + dim_y).standard_normal((dim_y, dim_x)).astype(np.float32)
    for a in (v, c, s, p):
        a.setflags(write=False)
    return v, c, s, p


def context_with(sfl, dim_x, dim_y):
    s = sfl.Solver(dim_x, dim_y)
    for field, a in zip(FIELDS, context_fields(dim_x, dim_y)):
        s.upload(field, a)
    return s


def queue_context_forces(s):
    s.queue_forces([[1, 1], [3, 2]], [[25.0, -5.0], [-15.0, 10.0]], step=0)
    s.queue_forces([[2, 3]], [[8.0, 30.0]], step=3)


@pytest.mark.parametrize("every", [1, 2])
@pytest.mark.parametrize("tracers", [False, True], ids=["", "tracers"])
@pytest.mark.parametrize("dims", [(61, 81), (130, 257)], ids=["one-workgroup", "tiled"])
def test_a_contexts_history(sfl, dims, tracers, every):
    """sfl_step and sfl_step_n(5) with SFL_OPT_STEP_SEAMS at its default, queued forces, with and without a following set of
    tracers; the twin is 6 x (sfl_step; sfl_flow_stats; sfl_residual), the run without a history the same two calls."""
    dim_x, dim_y = dims
    xy = np.random.default_rng(8).uniform(0.0, [dim_x - 1, dim_y - 1], (7, 2)).astype(np.float32)
    with context_with(sfl, dim_x, dim_y) as h, context_with(sfl, dim_x, dim_y) as plain, context_with(sfl, dim_x, dim_y) as t:
        assert h.get_option(sfl.capi.OPT_STEP_SEAMS) == 1
        h.history_start(every, 6 // every)
        for s in (h, plain, t):
            queue_context_forces(s)
            if tracers:
                s.set_tracers(xy, follow=True)
        for s in (h, plain):
            s.step(DT, DX, ITERS, OMEGA)
            s.step_n(5, DT, DX, ITERS, OMEGA)
        assert h.history_info() == (6 // every, 6 // every, 6)
        want = np.zeros(0, sfl.HISTORY_DTYPE)
        for step in range(1, 7):
            t.step(DT, DX, ITERS, OMEGA)
            rec = np.zeros(1, sfl.HISTORY_DTYPE)
            stats = t.flow_stats(DX)
            for name in stats.dtype.names:
                rec[name] = stats[name]
            rec["update_norm"], rec["iterations"], rec["step"], rec["dt"], rec["dx"] = t.residual(DX), ITERS, step, DT, DX
            if step % every == 0:
                want = np.concatenate([want, rec])
        got = h.history()
        assert got.shape == (6 // every,)
        assert_records(got, want, f"{dims} every {every}")
        assert_no_distance(h.distance(plain), "a history changes no field")
        assert_no_distance(h.distance(t), "... and the twin holds the same fields")
        if tracers:
            assert h.tracers().tobytes() == plain.tracers().tobytes()
        with pytest.raises(sfl.SflError) as e:
            h.step(DT, DX, ITERS, OMEGA) if every == 1 else h.step_n(2, DT, DX, ITERS, OMEGA)
        assert e.value.code == ERR_STATE and h.history_info() == (6 // every, 6 // every, 6)
        h.history_stop()
        h.step_n(2, DT, DX, ITERS, OMEGA)
        plain.step_n(2, DT, DX, ITERS, OMEGA)
        assert_no_distance(h.distance(plain), "after history_stop")


def test_a_slab_has_no_history(sfl):
    with sfl.Solver(64, 64, rank=0, nranks=2) as slab:
        for call in (lambda: slab.history_start(1, 4), slab.history_info, slab.history_stop, slab.history):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == ERR_STATE and "whole-domain" in str(e.value)
