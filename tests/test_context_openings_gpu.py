"""Openings on the rim of a whole-domain context on the GPU (include/sfl.h "OPENINGS OF A CONTEXT"; csrc/context_openings.hip)
against tests/opening_rule.py, bit for bit.

Shapes: 7 x 5 (less than one 64 x 32 tile), 61 x 81 (the sketch's grid: three tile rows), 65 x 33 (one cell more than a tile
each way: every opening of the east and north sides lies in a ragged tile of its own) and 257 x 130 (5 x 5 ragged tiles).  The
maps and masks are those of tests/test_openings_gpu.py; the iteration counts 0, 1, 7, 8, 9 and 19 straddle the 8 iterations of
one launch of the solve."""
import functools

import numpy as np
import pytest

import load_rule
import opening_rule as rule
from conftest import assert_bit_equal, random_fields
from test_openings_gpu import IN, OUT, map_of, solid_of
from test_solids_gpu import NAMES

pytestmark = pytest.mark.gpu

DT, DX, OMEGA = 1 / 30.0, 0.7, 1.9
SHAPES = [(7, 5), (61, 81), (65, 33), (257, 130)]
IDS = [f"{x}x{y}" for x, y in SHAPES]
# (map, mask, inflow): every map and every mask of the issue occurs
KINDS = {"tunnel": ("west_east", "none", (3.5, 0.0)), "updraft": ("south_north", "seeded", (0.0, 2.5)), "four": ("four", "disc", (2.0, 1.5)),
         "out_only": ("out_only", "seeded", (7.0, 7.0)), "in_only": ("in_only", "disc", (1.5, 0.0)), "slot": ("slot", "channel", (-0.0, 0.0)),
         "on_solid": ("on_solid", "walls", (1.25, -0.5)), "empty": ("empty", "disc", (9.0, 9.0))}


@functools.lru_cache(maxsize=None)
def case(kind, dim_x, dim_y):
    m, s, u = KINDS[kind]
    open, solid = map_of(m, dim_x, dim_y), solid_of(s, dim_x, dim_y)
    open.setflags(write=False)
    solid.setflags(write=False)
    return open, solid, np.array(u, np.float32)


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    v, c, s = random_fields(dim_x, dim_y, 500, vamp=40.0)
    for a in (v, c, s):
        a.setflags(write=False)
    return v, c, s


def records_of(kind, dim_x, dim_y):
    """step -> [(i, j, vx, vy)]: on a fluid cell twice, on an inflow cell, on an outflow cell, on a solid cell."""
    open, solid, _ = case(kind, dim_x, dim_y)
    fluid = np.argwhere(~solid & (open == 0))
    j, i = fluid[len(fluid) // 3]
    out = {0: [(int(i), int(j), 30.0, -20.0), (int(i), int(j), -12.5, 7.25)], 2: []}
    for what, step in ((IN, 0), (OUT, 2)):
        cells = np.argwhere((open == what) & ~solid)
        if len(cells):
            j, i = cells[len(cells) // 2]
            out[step].append((int(i), int(j), 55.0, 66.0))
    if solid.any():
        j, i = np.argwhere(solid)[int(solid.sum()) // 2]
        out[2].append((int(i), int(j), 5.0, 6.0))
    return out


@functools.lru_cache(maxsize=None)
def rule_steps(kind, dim_x, dim_y, iters, steps=3):
    from oracle import loader
    cpu = loader.port()
    open, solid, inflow = case(kind, dim_x, dim_y)
    v, c, _ = fields_of(dim_x, dim_y)
    forces = records_of(kind, dim_x, dim_y)
    state = (v, None, None, c)
    for k in range(steps):
        state = rule.step(cpu, state[0], state[3], solid, open, inflow, DT, DX, iters, OMEGA, forces.get(k, []))
    return state


def make(sfl, dim_x, dim_y, kind=None, masked=True, nranks=1):
    s = sfl.Solver(dim_x, dim_y, nranks=nranks)
    if nranks == 1:
        v, c, _ = fields_of(dim_x, dim_y)
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
    if kind is not None:
        open, solid, inflow = case(kind, dim_x, dim_y)
        if masked and solid.any():
            s.set_solids(solid)
        s.set_openings(open, inflow)
    return s


def queue(s, forces, only=None):
    for k, recs in forces.items():
        if recs and (only is None or only == k):
            s.queue_forces([r[:2] for r in recs], [r[2:] for r in recs], 0 if only is not None else k)


def download_all(sfl, s):
    cap = sfl.capi
    return tuple(s.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))


def assert_fields_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_bit_equal(g, w, f"{what}: {name}")


def bits(x):
    return np.float32(x).view(np.uint32)


# ---- 1. the step ---------------------------------------------------------------------------------------------------------
STEP_CASES = [(7, 5, k, 7) for k in KINDS] + [(61, 81, "four", 8), (61, 81, "in_only", 3), (65, 33, "tunnel", 9), (65, 33, "updraft", 1),
                                                (65, 33, "on_solid", 0), (257, 130, "four", 19), (257, 130, "slot", 8), (257, 130, "out_only", 7)]


@pytest.mark.parametrize("dim_x,dim_y,kind,iters", STEP_CASES, ids=[f"{x}x{y}-{k}-i{it}" for x, y, k, it in STEP_CASES])
def test_three_steps_are_three_steps_of_the_rule_and_step_n_is_three_steps(sfl, dim_x, dim_y, kind, iters):
    open, solid, inflow = case(kind, dim_x, dim_y)
    forces, want = records_of(kind, dim_x, dim_y), rule_steps(kind, dim_x, dim_y, iters)
    with make(sfl, dim_x, dim_y, kind) as s, make(sfl, dim_x, dim_y, kind) as one:
        assert s.openings_info() == (True, int(rule.inflow_cells(open, solid).sum()), int(rule.sides(open, solid)[1].sum()))
        got_map, got_inflow = s.openings()
        assert np.array_equal(got_map, open) and np.array_equal(got_inflow.view(np.uint32), inflow.view(np.uint32))
        assert s.solids_info()[0] == bool(solid.any()) and np.array_equal(s.solids(), solid), "the solids are what they were"
        queue(s, forces)
        s.step_n(3, DT, DX, iters, OMEGA)
        assert_fields_equal(download_all(sfl, s), want, "step_n(3)")
        for k in range(3):
            queue(one, forces, only=k)
            one.step(DT, DX, iters, OMEGA)
        assert_fields_equal(download_all(sfl, one), want, "step x 3")


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (65, 33), (257, 130)], ids=["7x5", "65x33", "257x130"])
def test_an_empty_map_and_a_cleared_map_give_the_bits_of_the_context_without_openings(sfl, dim_x, dim_y, masked):
    forces = records_of("four", dim_x, dim_y)

    def run(s):
        queue(s, forces)
        s.step_n(3, DT, DX, 9, OMEGA)
        return download_all(sfl, s), s.residual(DX), s.flow_stats(DX)

    solid = case("four", dim_x, dim_y)[1]
    with make(sfl, dim_x, dim_y) as plain, make(sfl, dim_x, dim_y) as empty, make(sfl, dim_x, dim_y, "four", masked) as cleared:
        for s in (plain, empty):
            if masked:
                s.set_solids(solid)
        empty.set_openings(np.zeros((dim_y, dim_x), np.uint8), (9.0, 9.0))
        assert empty.openings_info() == (True, 0, 0)
        want, got = run(plain), run(empty)
        assert_fields_equal(got[0], want[0], "an empty map")
        assert bits(got[1]) == bits(want[1]) and got[2].tobytes() == want[2].tobytes()
        other = run(cleared)
        assert not np.array_equal(other[0][0], want[0][0]), "a context with openings is another flow"
        v, c, _ = fields_of(dim_x, dim_y)
        cleared.upload(sfl.capi.FIELD_VELOCITY, v)
        cleared.upload(sfl.capi.FIELD_COLOR, c)
        cleared.set_openings(None)
        assert cleared.openings_info() == (False, 0, 0) and not cleared.openings()[0].any()
        got = run(cleared)
        assert_fields_equal(got[0], want[0], "a cleared map")
        assert bits(got[1]) == bits(want[1]) and got[2].tobytes() == want[2].tobytes()


@pytest.mark.parametrize("kind", ["four", "slot", "on_solid"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES[:3], ids=IDS[:3])
def test_a_context_equals_a_batch_member_of_its_shape(sfl, dim_x, dim_y, kind):
    open, solid, inflow = case(kind, dim_x, dim_y)
    v, c, _ = fields_of(dim_x, dim_y)
    forces = records_of(kind, dim_x, dim_y)
    with make(sfl, dim_x, dim_y, kind) as s, sfl.BatchSolver(dim_x, dim_y, 2) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, np.stack([v, v]))
        b.upload(sfl.capi.FIELD_COLOR, np.stack([c, c]))
        if solid.any():
            b.set_solids(solid)
        b.set_openings(open, inflow)
        queue(s, forces)
        for k, recs in forces.items():
            if recs:
                b.queue_forces([1] * len(recs), [r[:2] for r in recs], [r[2:] for r in recs], k)
        s.step_n(3, DT, DX, 9, OMEGA)
        b.step_n(3, DT, DX, 9, OMEGA)
        cap = sfl.capi
        for name, f in zip(NAMES, (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR)):
            assert_bit_equal(s.download(f), b.download(f)[1], f"context against member 1: {name}")
        assert s.flow_stats(DX)["max_abs_div"].view(np.uint32) == b.flow_stats(DX)[1]["max_abs_div"].view(np.uint32)


# ---- 2. the operators ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tunnel", "four", "updraft", "in_only", "on_solid"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_operators_one_by_one(sfl, dim_x, dim_y, kind):
    cap = sfl.capi
    open, solid, _ = case(kind, dim_x, dim_y)
    v, _, rhs = fields_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, kind) as s:
        s.calculate_divergence(DX)
        want = rule.divergence(v, solid, open, DX)
        assert_bit_equal(s.download(cap.FIELD_DIVERGENCE), want, "calculate_divergence")
        assert_bit_equal(s.download(cap.FIELD_VELOCITY), v, "... touches no velocity and imposes no inflow")
        stats = s.flow_stats(DX)
        assert stats["max_abs_div"].view(np.uint32) == np.abs(want).max().view(np.uint32)
        s.upload(cap.FIELD_PRESSURE, rhs)
        s.subtract_gradient(DX)
        assert_bit_equal(s.download(cap.FIELD_VELOCITY), rule.gradient(v, rhs, solid, open, DX), "subtract_gradient")


@pytest.mark.parametrize("iters", [0, 1, 7, 8, 9, 19])
@pytest.mark.parametrize("dim_x,dim_y,kind", [(7, 5, "four"), (65, 33, "slot"), (257, 130, "four"), (61, 81, "out_only")], ids=["7x5", "65x33", "257x130", "61x81"])
def test_the_solve_the_continued_solve_and_the_update_norm_follow_the_rule(sfl, dim_x, dim_y, kind, iters):
    cap = sfl.capi
    open, solid, _ = case(kind, dim_x, dim_y)
    rhs = fields_of(dim_x, dim_y)[2]
    with make(sfl, dim_x, dim_y, kind) as s:
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        s.poisson_solve(DX, iters, OMEGA)
        want = rule.solve(rhs, solid, open, DX, iters, OMEGA)
        assert_bit_equal(s.download(cap.FIELD_PRESSURE), want, f"poisson_solve({iters})")
        assert s.residual(DX).view(np.uint32) == rule.update_norm(want, rhs, solid, open, DX).view(np.uint32)
        s.poisson_continue(DX, 3, OMEGA)
        more = rule.iterate(want, rhs, solid, open, DX, 3, OMEGA)
        assert_bit_equal(s.download(cap.FIELD_PRESSURE), more, "poisson_continue(3)")
        assert s.residual(DX).view(np.uint32) == rule.update_norm(more, rhs, solid, open, DX).view(np.uint32)


@pytest.mark.parametrize("dim_x,dim_y,kind", [(7, 5, "tunnel"), (65, 33, "four"), (257, 130, "slot")], ids=["7x5", "65x33", "257x130"])
def test_solve_until_leaves_the_rules_solve_of_the_count_it_reports(sfl, dim_x, dim_y, kind):
    cap = sfl.capi
    open, solid, _ = case(kind, dim_x, dim_y)
    rhs = fields_of(dim_x, dim_y)[2]

    def norm_after(n):
        return rule.update_norm(rule.solve(rhs, solid, open, DX, n, 1.5), rhs, solid, open, DX)

    with make(sfl, dim_x, dim_y, kind) as s:
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        first = norm_after(3)
        for cap_iters, tol, every in ((12, float(first), 3), (7, 0.0, 3), (5, -1.0, 2), (0, 1.0, 1)):
            k, u = s.poisson_solve_until(DX, cap_iters, 1.5, tol, every)
            norms = [norm_after(n) for n in range(0, cap_iters + 1, every)]
            stops = [n * every for n, x in enumerate(norms) if tol >= 0 and not x > tol]
            assert k == (stops[0] if stops else cap_iters), (cap_iters, tol, every)
            want = rule.solve(rhs, solid, open, DX, k, 1.5)
            assert_bit_equal(s.download(cap.FIELD_PRESSURE), want, f"solve_until -> {k}")
            assert u.view(np.uint32) == rule.update_norm(want, rhs, solid, open, DX).view(np.uint32)


# ---- 3. statistics and histories -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y,kind", [(7, 5, "four"), (61, 81, "tunnel"), (65, 33, "updraft"), (257, 130, "four")], ids=IDS)
def test_every_record_of_a_history_is_what_the_calls_return_after_the_same_step(sfl, dim_x, dim_y, kind):
    iters, forces = 7, records_of(kind, dim_x, dim_y)
    with make(sfl, dim_x, dim_y, kind) as s, make(sfl, dim_x, dim_y, kind) as twin:
        s.history_start(1, 4)
        queue(s, forces)
        s.step_n(3, DT, DX, iters, OMEGA)
        got = s.history()
        assert len(got) == 3
        for k in range(3):
            queue(twin, forces, only=k)
            twin.step(DT, DX, iters, OMEGA)
            stats, norm = twin.flow_stats(DX), twin.residual(DX)
            for name in ("max_abs_vx", "max_abs_vy", "max_abs_div"):
                assert got[k][name].view(np.uint32) == stats[name].view(np.uint32), (k, name)
            assert np.array_equal(got[k]["dye_sum"], stats["dye_sum"]) and got[k]["update_norm"].view(np.uint32) == norm.view(np.uint32), k
        s.history_stop()
        open, solid, _ = case(kind, dim_x, dim_y)
        v = s.download(sfl.capi.FIELD_VELOCITY)
        assert got[2]["max_abs_div"].view(np.uint32) == np.abs(rule.divergence(v, solid, open, DX)).max().view(np.uint32)
        assert_fields_equal(download_all(sfl, s), rule_steps(kind, dim_x, dim_y, iters), "with a history on")


def test_loads_next_to_openings_are_the_rule_of_the_loads_on_the_downloaded_pressure(sfl):
    dim_x, dim_y = 65, 33
    with make(sfl, dim_x, dim_y, "four") as s:
        s.step_n(2, DT, DX, 9, OMEGA)
        p, got = s.download(sfl.capi.FIELD_PRESSURE), s.loads()
    want = load_rule.loads(p, case("four", dim_x, dim_y)[1])
    assert got.tobytes() == want.tobytes() and got["fx"].any()


def test_a_uniform_flow_passes_through_the_open_channel_and_the_inflow_can_be_changed(sfl, oracle):
    dim_x, dim_y, U = 257, 130, np.float32(3.5)
    solid, open = solid_of("walls", dim_x, dim_y), map_of("west_east", dim_x, dim_y)
    v = np.zeros((dim_y, dim_x, 2), np.float32)
    v[~solid, 0] = U
    with sfl.Solver(dim_x, dim_y) as s:
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.set_solids(solid)
        s.set_openings(open, (U, 0.0))
        assert s.flow_stats(1.0)["max_abs_div"].view(np.uint32) == 0
        s.step(0.0, 1.0, 5, OMEGA)
        got = download_all(sfl, s)
        assert_bit_equal(got[0], v, "velocity")
        assert not got[1].view(np.uint32).any() and not (got[2].view(np.uint32) & 0x7FFFFFFF).any()
        # tiny and signed-zero inflows keep their bits
        for inflow in ((2.0 ** -140, -0.0), (-0.0, 0.0)):
            s.set_inflow(inflow)
            assert np.array_equal(s.openings()[1].view(np.uint32), np.array(inflow, np.float32).view(np.uint32))
            c = s.download(sfl.capi.FIELD_COLOR)
            s.upload(sfl.capi.FIELD_VELOCITY, v)
            s.step(DT, DX, 8, OMEGA)
            want = rule.step(oracle, v, c, solid, open, np.array(inflow, np.float32), DT, DX, 8, OMEGA)
            assert_fields_equal(download_all(sfl, s), want, f"inflow {inflow}")
        s.set_openings(None)
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        assert s.flow_stats(1.0)["max_abs_div"] == U, "the closed rule sees a wall at both ends"


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------
def test_the_refusals_leave_the_context_stepping_on(sfl):
    cap, (dim_x, dim_y), kind = sfl.capi, (65, 33), "four"
    open, solid, inflow = case(kind, dim_x, dim_y)

    def refused(call, *words, code=cap.ERR_STATE):
        with pytest.raises(sfl.SflError) as e:
            call()
        assert e.value.code == code, e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    with make(sfl, 64, 512, nranks=2) as slab:
        refused(lambda: slab.set_openings(np.zeros((512, 64), np.uint8), (1.0, 0.0)), "whole-domain contexts only")
        assert slab.openings_info() == (False, 0, 0)
    with make(sfl, dim_x, dim_y, kind) as s:
        bad = open.copy()
        bad[0, 0] = IN
        refused(lambda: s.set_openings(bad, inflow), "cell (0, 0)", "is a corner", code=cap.ERR_INVALID)
        bad[0, 0], bad[2, 3] = 0, OUT
        refused(lambda: s.set_openings(bad, inflow), "cell (3, 2)", "interior cell", code=cap.ERR_INVALID)
        bad[2, 3], bad[1, 0] = 0, 3
        refused(lambda: s.set_openings(bad, inflow), "cell (0, 1) holds 3", code=cap.ERR_INVALID)
        refused(lambda: s.set_openings(open, (np.nan, 0.0)), "must be finite", code=cap.ERR_INVALID)
        refused(lambda: s.set_inflow((np.inf, 0.0)), "must be finite", code=cap.ERR_INVALID)
        view = sfl.View(cap.VIEW_DIVERGENCE, -1.0, 1.0, dx=DX)
        s.set_solids(None)   # (with solids set their own refusals of the same calls come first)
        for call in (lambda: s.view_scalar(cap.VIEW_DIVERGENCE, DX), lambda: s.view_texels(view), lambda: s.view_render(view, 1)):
            refused(call, "openings set", "divergence view")
        for call in (s.comm_emulate, s.comm_emulate_rccl, lambda: s.comm_attach(bytes(256)), lambda: sfl.Solver.link_group([s])):
            refused(call, "openings set")
        refused(lambda: s.set_viscosity(0.1, 2), "sfl_set_viscosity", "openings set")
        s.set_solids(solid)
        assert s.openings_info()[0] and np.array_equal(s.openings()[0], open)
        queue(s, records_of(kind, dim_x, dim_y))
        s.step_n(3, DT, DX, 9, OMEGA)
        assert_fields_equal(download_all(sfl, s), rule_steps(kind, dim_x, dim_y, 9), "after the refusals")
        s.set_openings(None)
        refused(lambda: s.set_inflow((1.0, 0.0)), "no openings set")
        s.set_viscosity(0.1, 2)
        refused(lambda: s.set_openings(open, inflow), "viscosity is set")
        assert s.openings_info() == (False, 0, 0)
        s.set_viscosity(0.0, 0)
        s.set_openings(open, inflow)
        s.step(DT, DX, 9, OMEGA)
