"""Solid cells inside the grid of a whole-domain context on the GPU (include/sfl.h "SOLIDS OF A CONTEXT";
csrc/context_solids.hip) against tests/solid_rule.py -- the header's rule in numpy float32, itself held to the reference and the
oracle by tests/test_solids.py.  Every comparison is bit for bit.

Shapes: 7 x 5 (inside one tile; without a mask the one-launch step of a small grid); 61 x 81 (the sketch's grid: three tiles
one above the other, without a mask still a small grid); (TX + 1) x (TY + 1) (one cell more than a tile both ways: four
tiles, three of them a sliver); 257 x 130 (5 x 5 ragged tiles; without a mask the fused kernels and the step seams).  The
masks are those of tests/test_solids_gpu.py.  ITERS = 6 is one launch that runs fewer than D = 8 iterations; 2 D + 3 is three
launches, the last a short one."""
import functools

import numpy as np
import pytest

import solid_rule as rule
from conftest import assert_bit_equal, random_fields
from test_context_solids import D, TX, TY
from test_solids_gpu import forces_of, mask_of

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 6, 1.9
ITERS_LONG = 2 * D + 3
SOLVE_ITERS = [0, 1, D - 1, D, D + 1, 2 * D + 3]
NAMES = ("velocity", "divergence", "pressure", "colour")
SHAPES = [(7, 5), (61, 81), (TX + 1, TY + 1), (257, 130)]
IDS = [f"{x}x{y}" for x, y in SHAPES]
KINDS = ["one", "disc", "plate", "channel", "isolated", "all", "seeded", "empty"]


@functools.lru_cache(maxsize=None)
def solid(kind, dim_x, dim_y):
    m = mask_of(kind, dim_x, dim_y)
    m.setflags(write=False)
    return m


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    """Seeded velocity, dye and a right-hand side (solid cells hold values too: the rule reads them as they stand).  Shared, never written."""
    v, c, s = random_fields(dim_x, dim_y, 100, vamp=40.0)
    for a in (v, c, s):
        a.setflags(write=False)
    return v, c, s


def records_of(kind, dim_x, dim_y):
    """step -> [(i, j, vx, vy)]: on a fluid cell (twice on one: the later wins), on a solid cell, outside the grid."""
    return {k: [r[1:] for r in recs] for k, recs in forces_of(dim_x, dim_y, [solid(kind, dim_x, dim_y)]).items()}


@functools.lru_cache(maxsize=None)
def rule_steps(kind, dim_x, dim_y, iters=ITERS, steps=3, forced=True):
    """The fields after `steps` steps of the rule: (v, div, p, colour).  Computed once, shared, never written."""
    from oracle import loader
    cpu = loader.port()
    v, c, _ = fields_of(dim_x, dim_y)
    forces = records_of(kind, dim_x, dim_y) if forced else {}
    state = (v, None, None, c)
    for k in range(steps):
        state = rule.step(cpu, state[0], state[3], solid(kind, dim_x, dim_y), DT, DX, iters, OMEGA, forces.get(k, []))
    for a in state:
        a.setflags(write=False)
    return state


def make(sfl, dim_x, dim_y, mask=None, **kw):
    s = sfl.Solver(dim_x, dim_y, **kw)
    if kw.get("nranks", 1) == 1:
        v, c, _ = fields_of(dim_x, dim_y)
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
    if mask is not None:
        s.set_solids(mask)
    return s


def queue(s, forces, only=None):
    for k, recs in forces.items():
        if recs and only in (None, k):
            s.queue_forces([r[:2] for r in recs], [r[2:] for r in recs], 0 if only is not None else k)


def download_all(sfl, s):
    cap = sfl.capi
    return tuple(s.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))


def assert_fields_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_bit_equal(g, w, f"{what}: {name}")


# ---- 1. three steps with forces against the rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_are_three_steps_of_the_rule(sfl, dim_x, dim_y, kind):
    mask, forces, want = solid(kind, dim_x, dim_y), records_of(kind, dim_x, dim_y), rule_steps(kind, dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask) as s:
        assert s.solids_info() == (True, int(mask.sum())) and np.array_equal(s.solids(), mask)
        queue(s, forces)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, s), want, "step_n(3)")
        assert s.last_solve_info()["launches"] == -(-ITERS // D)
    with make(sfl, dim_x, dim_y, mask) as s:   # ... and step by step, every step's records queued in front of it
        for k in range(3):
            queue(s, forces, only=k)
            s.step(DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, s), want, "step x 3")


def test_three_steps_with_a_solve_of_three_launches(sfl):
    dim_x, dim_y, kind = 257, 130, "seeded"
    with make(sfl, dim_x, dim_y, solid(kind, dim_x, dim_y)) as s:
        s.set_option(sfl.capi.OPT_SOR_FOLD, 1)   # (no effect while solids are set: the masked kernel knows the rule's arithmetic only)
        queue(s, records_of(kind, dim_x, dim_y))
        s.step_n(3, DT, DX, ITERS_LONG, OMEGA)
        assert_fields_equal(download_all(sfl, s), rule_steps(kind, dim_x, dim_y, ITERS_LONG), f"iters {ITERS_LONG}")
        assert s.last_solve_info()["launches"] == 3


# ---- 2. an empty mask is the plain context; so is a cleared one ---------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_an_empty_mask_and_a_cleared_one_give_the_plain_contexts_bits(sfl, dim_x, dim_y):
    cap, forces, rhs = sfl.capi, records_of("disc", dim_x, dim_y), fields_of(dim_x, dim_y)[2]
    with make(sfl, dim_x, dim_y) as plain, make(sfl, dim_x, dim_y, solid("empty", dim_x, dim_y)) as s:
        assert s.solids_info() == (True, 0)
        for x in (plain, s):
            queue(x, forces)
            x.step_n(3, DT, DX, ITERS, OMEGA)
        want = download_all(sfl, plain)
        assert_fields_equal(download_all(sfl, s), want, "an empty mask: step_n(3)")
        for x in (plain, s):
            x.upload(cap.FIELD_DIVERGENCE, rhs)
            x.poisson_solve(DX, ITERS_LONG, OMEGA)
        solved = plain.download(cap.FIELD_PRESSURE)
        assert_bit_equal(s.download(cap.FIELD_PRESSURE), solved, "an empty mask: poisson_solve")
        assert s.residual(DX).view(np.uint32) == plain.residual(DX).view(np.uint32)
        # a disc, then cleared: the plain context again, from the same fields
        s.set_solids(solid("disc", dim_x, dim_y))
        s.step(DT, DX, ITERS, OMEGA)
        s.set_solids(None)
        assert s.solids_info() == (False, 0) and not s.solids().any()
        v, c, _ = fields_of(dim_x, dim_y)
        s.upload(cap.FIELD_VELOCITY, v)
        s.upload(cap.FIELD_COLOR, c)
        queue(s, forces)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, s), want, "cleared: step_n(3)")
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        s.poisson_solve(DX, ITERS_LONG, OMEGA)
        assert_bit_equal(s.download(cap.FIELD_PRESSURE), solved, "cleared: poisson_solve")


# ---- 3. the context against a batch member with the same mask ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["disc", "seeded", "channel"])
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (7, 5)], ids=["61x81", "7x5"])
def test_a_context_equals_a_batch_member_with_the_same_mask(sfl, dim_x, dim_y, kind):
    cap, mask, forces = sfl.capi, solid(kind, dim_x, dim_y), records_of(kind, dim_x, dim_y)
    v, c, _ = fields_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask) as s, sfl.BatchSolver(dim_x, dim_y, 1) as b:
        b.upload(cap.FIELD_VELOCITY, v[None])
        b.upload(cap.FIELD_COLOR, c[None])
        b.set_solids(mask)
        for k, recs in forces.items():
            if recs:
                b.queue_forces([0] * len(recs), [r[:2] for r in recs], [r[2:] for r in recs], k)
        queue(s, forces)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        for name, f in zip(NAMES, (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR)):
            assert_bit_equal(s.download(f), b.download(f)[0], name)


# ---- 4. the solve and its companions ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["seeded", "plate", "isolated"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_solve_the_continued_solve_and_the_update_norm_follow_the_rule(sfl, dim_x, dim_y, kind):
    cap, mask = sfl.capi, solid(kind, dim_x, dim_y)
    rhs = fields_of(dim_x, dim_y)[2]
    with make(sfl, dim_x, dim_y, mask) as s:
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        for iters in SOLVE_ITERS:
            s.poisson_solve(DX, iters, OMEGA)
            want = rule.solve(rhs, mask, DX, iters, OMEGA)
            assert_bit_equal(s.download(cap.FIELD_PRESSURE), want, f"poisson_solve({iters})")
            assert s.last_solve_info()["launches"] == -(-iters // D)
            assert s.residual(DX).view(np.uint32) == rule.update_norm(want, rhs, mask, DX).view(np.uint32), f"residual after {iters}"
        # solve(a) then continue(b) is solve(a + b); continue(0) leaves the pressure alone
        for a, b in ((1, D), (D, D - 1), (D + 1, D + 2), (0, 2 * D + 3)):
            s.poisson_solve(DX, a, OMEGA)
            s.poisson_continue(DX, 0, OMEGA)
            s.poisson_continue(DX, b, OMEGA)
            assert_bit_equal(s.download(cap.FIELD_PRESSURE), rule.solve(rhs, mask, DX, a + b, OMEGA), f"solve({a}) + continue({b})")
        # a pressure that was uploaded: solid cells keep what they hold, and have no say in the norm
        start = (fields_of(dim_x, dim_y)[0][..., 0] * np.float32(0.01)).astype(np.float32)
        s.upload(cap.FIELD_PRESSURE, start)
        s.poisson_continue(DX, D + 1, OMEGA)
        got = s.download(cap.FIELD_PRESSURE)
        assert_bit_equal(got[mask], start[mask], "solid cells are never updated")
        assert s.residual(DX).view(np.uint32) == rule.update_norm(got, rhs, mask, DX).view(np.uint32)


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_solve_until_leaves_the_rules_solve_of_the_count_it_reports(sfl, dim_x, dim_y):
    cap, mask = sfl.capi, solid("disc", dim_x, dim_y)
    rhs = fields_of(dim_x, dim_y)[2]
    with make(sfl, dim_x, dim_y, mask) as s:
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        first = rule.update_norm(rule.solve(rhs, mask, DX, 3, 1.5), rhs, mask, DX)
        for cap_iters, tol, every in ((12, float(first), 3), (7, 0.0, 3), (5, -1.0, 2), (0, 1.0, 1)):
            k, u = s.poisson_solve_until(DX, cap_iters, 1.5, tol, every)
            norms = [rule.update_norm(rule.solve(rhs, mask, DX, n, 1.5), rhs, mask, DX) for n in range(0, cap_iters + 1, every)]
            stops = [n * every for n, x in enumerate(norms) if tol >= 0 and not x > tol]
            assert k == (stops[0] if stops else cap_iters), (cap_iters, tol, every)
            want = rule.solve(rhs, mask, DX, k, 1.5)
            assert_bit_equal(s.download(cap.FIELD_PRESSURE), want, f"solve_until -> {k}")
            assert u.view(np.uint32) == rule.update_norm(want, rhs, mask, DX).view(np.uint32)


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_without_a_fluid_cell_the_norm_is_zero_and_nothing_moves(sfl, dim_x, dim_y):
    cap, mask = sfl.capi, solid("all", dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask) as s:
        s.upload(cap.FIELD_DIVERGENCE, fields_of(dim_x, dim_y)[2])
        s.poisson_solve(DX, ITERS, OMEGA)
        assert not s.download(cap.FIELD_PRESSURE).view(np.uint32).any()
        assert s.residual(DX).view(np.uint32) == 0
        assert s.poisson_solve_until(DX, 5, OMEGA, 0.0, 2)[0] == 0
        assert s.flow_stats(DX, dye=False)["max_abs_div"].view(np.uint32) == 0


# ---- 5. the operators one by one; the statistics ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["seeded", "channel", "disc"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_operators_one_by_one(sfl, dim_x, dim_y, kind):
    cap, mask = sfl.capi, solid(kind, dim_x, dim_y)
    v, _, rhs = fields_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask) as s:
        s.calculate_divergence(DX)
        want = rule.divergence(v, mask, DX)
        assert_bit_equal(s.download(cap.FIELD_DIVERGENCE), want, "calculate_divergence")
        assert_bit_equal(s.download(cap.FIELD_VELOCITY), v, "... touches no velocity, a solid cell's neither")
        stats = s.flow_stats(DX)
        assert stats["max_abs_div"].view(np.uint32) == np.abs(want).max().view(np.uint32)
        assert stats["max_abs_vx"] == np.abs(v[..., 0]).max() and stats["max_abs_vy"] == np.abs(v[..., 1]).max()
        s.upload(cap.FIELD_PRESSURE, rhs)
        s.subtract_gradient(DX)
        assert_bit_equal(s.download(cap.FIELD_VELOCITY), rule.gradient(v, rhs, mask, DX), "subtract_gradient")
        # a NaN wins the maximum
        bad = v.copy()
        j, i = np.argwhere(~mask)[len(np.argwhere(~mask)) // 2]
        bad[j, i, 0] = np.nan
        s.upload(cap.FIELD_VELOCITY, bad)
        assert np.isnan(rule.divergence(bad, mask, DX)).any() and np.isnan(s.flow_stats(DX, dye=False)["max_abs_div"])


# ---- 6. a history's samples ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_every_record_of_a_history_is_what_the_calls_return_after_the_same_step(sfl, dim_x, dim_y):
    mask, forces = solid("seeded", dim_x, dim_y), records_of("seeded", dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask) as s, make(sfl, dim_x, dim_y, mask) as twin:
        s.history_start(1, 4)
        queue(s, forces)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        got = s.history()
        assert len(got) == 3
        for k in range(3):
            queue(twin, forces, only=k)
            twin.step(DT, DX, ITERS, OMEGA)
            stats, norm = twin.flow_stats(DX), twin.residual(DX)
            for name in ("max_abs_vx", "max_abs_vy", "max_abs_div"):
                assert got[k][name].view(np.uint32) == stats[name].view(np.uint32), (k, name)
            assert np.array_equal(got[k]["dye_sum"], stats["dye_sum"]) and got[k]["update_norm"].view(np.uint32) == norm.view(np.uint32), k
            assert got[k]["iterations"] == ITERS and got[k]["step"] == k + 1
        s.history_stop()
        assert_fields_equal(download_all(sfl, s), rule_steps("seeded", dim_x, dim_y), "with a history on")


# ---- 7. refusals -----------------------------------------------------------------------------------------------------------
def test_the_refusals_leave_the_context_stepping_on(sfl):
    cap, (dim_x, dim_y), kind = sfl.capi, (TX + 1, TY + 1), "disc"
    mask = solid(kind, dim_x, dim_y)
    with make(sfl, 64, 512, nranks=2) as slab:
        with pytest.raises(cap.SflError, match="whole-domain contexts only") as e:
            slab.set_solids(np.zeros((512, 64), bool))
        assert e.value.code == cap.ERR_STATE and slab.solids_info() == (False, 0)
    with make(sfl, dim_x, dim_y, mask) as s:
        view = sfl.View(cap.VIEW_DIVERGENCE, -1.0, 1.0, dx=DX)
        for call in (lambda: s.view_scalar(cap.VIEW_DIVERGENCE, DX), lambda: s.view_texels(view), lambda: s.view_render(view, 1)):
            with pytest.raises(cap.SflError, match="divergence view") as e:
                call()
            assert e.value.code == cap.ERR_STATE
        for call in (s.comm_emulate, s.comm_emulate_rccl, lambda: s.comm_attach(bytes(256)), lambda: sfl.Solver.link_group([s])):
            with pytest.raises(cap.SflError, match="solid cells set") as e:
                call()
            assert e.value.code == cap.ERR_STATE
        assert s.solids_info() == (True, int(mask.sum()))
        s.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, s), rule_steps(kind, dim_x, dim_y, forced=False), "after the refusals")


# ---- 8. what stays as it is next to a mask ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (257, 130)], ids=["61x81", "257x130"])
def test_views_tracers_and_render_work_next_to_a_mask_as_ever(sfl, dim_x, dim_y):
    cap, mask = sfl.capi, solid("disc", dim_x, dim_y)
    xy = np.random.default_rng(5).uniform(1, min(dim_x, dim_y) - 2, (64, 2)).astype(np.float32)
    vort = sfl.View(cap.VIEW_VORTICITY, -20.0, 20.0, sfl.solver.PALETTE_BLUE_WHITE_RED, dx=DX)
    with make(sfl, dim_x, dim_y, mask) as s, make(sfl, dim_x, dim_y, mask) as twin, make(sfl, dim_x, dim_y) as plain:
        s.set_tracers(xy, follow=True)      # moved by the masked step through the step's hook
        twin.set_tracers(xy, follow=False)  # ... and by hand behind every step
        s.step_n(3, DT, DX, ITERS, OMEGA)
        for _ in range(3):
            twin.step(DT, DX, ITERS, OMEGA)
            twin.advance_tracers(DT)
        assert_bit_equal(s.tracers(), twin.tracers(), "following tracers")
        fields = download_all(sfl, s)
        assert_fields_equal(fields, download_all(sfl, twin), "the twin")
        assert_fields_equal(fields, rule_steps("disc", dim_x, dim_y, forced=False), "with following tracers")
        # a context WITHOUT a mask that holds the same fields draws the same pictures: the views' kernels are the plain ones
        for f, a in zip((cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR), fields):
            plain.upload(f, a)
        for what in (cap.VIEW_VORTICITY, cap.VIEW_SPEED, cap.VIEW_PRESSURE):
            assert_bit_equal(s.view_scalar(what, DX), plain.view_scalar(what, DX), f"view {what}")
        assert not s.view_scalar(cap.VIEW_SPEED, DX)[mask].any(), "solid cells stand still"
        assert np.array_equal(s.view_render(vort, 2), plain.view_render(vort, 2))
        assert np.array_equal(s.view_texels(vort), plain.view_texels(vort))
        assert np.array_equal(s.render_rgb565(2), plain.render_rgb565(2))
