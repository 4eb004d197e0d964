"""Inflow profiles and the flux of a whole-domain context on the GPU (include/sfl.h "INFLOW PROFILES AND FLUX";
csrc/context_openings.cpp's item 2a with a profile, csrc/inflow.hip) against tests/inflow_rule.py, bit for bit.

Shapes: 5 x 4 (less than one 64 x 32 tile), 130 x 70 and 257 x 130 (ragged tiles both ways); the map opens all four sides, the
mask puts a solid cell under a profiled inflow cell and a disc in the middle.  At 61 x 81 a context equals a batch member of
the same map, mask, profile and fields in every field and in the flux record."""
import functools

import numpy as np
import pytest

import inflow_rule as rule
from conftest import random_fields
from test_context_openings_gpu import assert_fields_equal, download_all
from test_openings_gpu import IN, map_of
from test_solids_gpu import mask_of

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 9, 1.9
SHAPES = [(5, 4), (130, 70), (257, 130)]
IDS = [f"{x}x{y}" for x, y in SHAPES]
INFLOW = np.array((2.0, 1.5), np.float32)


@functools.lru_cache(maxsize=None)
def case(dim_x, dim_y, masked):
    """(map, mask, the profile's records in the order given): a parabola over the west column with one cell named twice, every
    second cell of the south row; masked: a solid cell under the profiled cell (0, dim_y // 2), a disc in the middle."""
    open = map_of("four", dim_x, dim_y)
    solid = mask_of("disc", dim_x, dim_y) if masked and min(dim_x, dim_y) > 4 else np.zeros((dim_y, dim_x), bool)
    if masked:
        solid[dim_y // 2, 0] = True
    west = [(0, j) for j in range(1, dim_y - 1)]
    s = [(j - 0.5) / (dim_y - 2) for j in range(1, dim_y - 1)]
    records = [(west[len(west) // 2], (np.float32(77.0), np.float32(-77.0)))]
    records += [(c, (np.float32(8.0 * 4 * x * (1 - x)), np.float32(0.25))) for c, x in zip(west[::-1], s[::-1])]
    records += [((i, 0), (np.float32(0.5), np.float32(1.0 + i))) for i in range(1, dim_x - 1, 2)]
    open.setflags(write=False)
    solid.setflags(write=False)
    return open, solid, records


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    v, c, _ = random_fields(dim_x, dim_y, 900, vamp=40.0)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y):
    """step -> [(i, j, vx, vy)]: on the profiled inflow cell (0, dim_y // 2) (no effect), on a cell inside."""
    return {0: [(0, dim_y // 2, 55.0, 66.0)], 1: [(dim_x // 2, dim_y // 4, -12.5, 7.25)]}


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, masked, steps=3):
    from oracle import loader
    cpu = loader.port()
    open, solid, records = case(dim_x, dim_y, masked)
    v, c = fields_of(dim_x, dim_y)
    forces = forces_of(dim_x, dim_y)
    state = (v, None, None, c)
    for k in range(steps):
        state = rule.step(cpu, state[0], state[3], solid, open, INFLOW, records, DT, DX, ITERS, OMEGA, forces.get(k, []))
    return state


def make(sfl, dim_x, dim_y, masked, profile=True):
    open, solid, records = case(dim_x, dim_y, masked)
    s = sfl.Solver(dim_x, dim_y)
    reload(sfl, s, dim_x, dim_y)
    if solid.any():
        s.set_solids(solid)
    s.set_openings(open, INFLOW)
    if profile:
        s.set_inflow_profile([c for c, _ in records], [u for _, u in records])
    return s


def reload(sfl, s, dim_x, dim_y):
    v, c = fields_of(dim_x, dim_y)
    s.upload(sfl.capi.FIELD_VELOCITY, v)
    s.upload(sfl.capi.FIELD_COLOR, c)


def queue(s, forces, only=None):
    for k, recs in forces.items():
        if recs and (only is None or only == k):
            s.queue_forces([r[:2] for r in recs], [r[2:] for r in recs], 0 if only is not None else k)


# ---- 1. the step against the rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_with_a_profile_are_three_steps_of_the_rule_and_step_n_is_three_steps(sfl, dim_x, dim_y, masked):
    open, solid, records = case(dim_x, dim_y, masked)
    forces, want = forces_of(dim_x, dim_y), rule_steps(dim_x, dim_y, masked)
    with make(sfl, dim_x, dim_y, masked) as s, make(sfl, dim_x, dim_y, masked) as one:
        rows = rule.unique(records)
        assert len(rows) < len(records), "a cell is named twice"
        cells, vel = s.inflow_profile()
        assert [tuple(c) for c in cells] == [c for c, _ in rows], "the records come back in cell order, duplicates removed"
        assert np.array_equal(vel.view(np.uint32), np.array([u for _, u in rows], np.float32).view(np.uint32))
        queue(s, forces)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, s), want, "step_n(3)")
        for k in range(3):
            queue(one, forces, only=k)
            one.step(DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, one), want, "step x 3")


# ---- 2. the anchor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_a_uniform_profile_and_a_cleared_profile_give_the_bits_of_the_context_without_one(sfl, dim_x, dim_y, masked):
    open, solid, records = case(dim_x, dim_y, masked)
    forces = forces_of(dim_x, dim_y)
    every = [(int(i), int(j)) for j, i in np.argwhere(open == IN)]

    def run(s):
        queue(s, forces)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        return download_all(sfl, s)

    with make(sfl, dim_x, dim_y, masked, profile=False) as plain, make(sfl, dim_x, dim_y, masked, profile=False) as uniform, make(sfl, dim_x, dim_y, masked) as cleared:
        want = run(plain)
        uniform.set_inflow_profile(every, [tuple(INFLOW)] * len(every))
        assert len(uniform.inflow_profile()[0]) == len(every)
        assert_fields_equal(run(uniform), want, "a uniform profile")
        assert not np.array_equal(run(cleared)[0], want[0]), "a profile is another flow"
        reload(sfl, cleared, dim_x, dim_y)
        cleared.set_inflow_profile(None, None)
        assert len(cleared.inflow_profile()[0]) == 0
        assert_fields_equal(run(cleared), want, "a cleared profile")
        # set_inflow keeps a profile, and the cells it does not name follow the new inflow; a new map drops it
        reload(sfl, uniform, dim_x, dim_y)
        uniform.set_inflow_profile(every[:1], [tuple(INFLOW)])
        uniform.set_inflow((9.0, -9.0))
        uniform.set_inflow(INFLOW)
        assert len(uniform.inflow_profile()[0]) == 1
        assert_fields_equal(run(uniform), want, "the inflow changed and changed back under a profile")
        uniform.set_openings(open, INFLOW)
        assert len(uniform.inflow_profile()[0]) == 0


# ---- 3. the flux ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_flux_after_no_step_and_after_three_is_the_rules_record_byte_for_byte(sfl, dim_x, dim_y, masked):
    open, solid, _ = case(dim_x, dim_y, masked)
    with make(sfl, dim_x, dim_y, masked) as s:
        for what, steps in (("after no step", 0), ("after three steps", 3)):
            if steps:
                s.step_n(steps, DT, DX, ITERS, OMEGA)
            got, want = s.openings_flux(), rule.flux(s.download(sfl.capi.FIELD_VELOCITY), open, solid)
            assert got.dtype == sfl.OPEN_FLUX_DTYPE and got.shape == () and got.tobytes() == want.tobytes(), (what, got, want)
        assert int(got["inflow_cells"]) > 0 and int(got["nonfinite"]) == 0 and int(got["inflow"]) != 0
        assert tuple(sfl.openings_flux_xy(got)) == rule.flux_xy(got)


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_flux_counts_a_nan_and_an_inf_and_sums_the_rest_and_reports_zeros_where_nothing_is_live(sfl, dim_x, dim_y):
    open = map_of("four", dim_x, dim_y)
    v = fields_of(dim_x, dim_y)[0].copy()
    v[dim_y // 2, 0, 0] = np.nan       # a west inflow cell
    v[dim_y // 2, -1, 0] = -np.inf     # an east outflow cell
    v[1, 0, 1] = np.nan                # the tangential component of a west cell: no part of n
    v[-1, dim_x // 2, 1] = np.float32(1e-42)   # a denormal beside ordinary normals
    with sfl.Solver(dim_x, dim_y) as s:
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        assert s.openings_flux().tobytes() == bytes(40), "a context without openings reports zeros"
        s.set_openings(open, INFLOW)
        got, want = s.openings_flux(), rule.flux(v, open)
        assert got.tobytes() == want.tobytes() and int(got["nonfinite"]) == 2, (got, want)
        s.upload(sfl.capi.FIELD_VELOCITY, (v * np.float32(1e-42)).astype(np.float32))   # denormal normals, the NaN and the Inf still there
        got, want = s.openings_flux(), rule.flux((v * np.float32(1e-42)).astype(np.float32), open)
        assert got.tobytes() == want.tobytes() and int(got["exp2"]) < -126 - 32, (got, want)
        s.set_solids(open != 0)   # every open cell solid
        assert s.openings_flux().tobytes() == bytes(40), "no live open cell: zeros"
        s.set_solids(None)
        s.set_openings(None)
        assert s.openings_flux().tobytes() == bytes(40), "cleared: zeros again"


# ---- 4. a context and a batch member ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
def test_a_context_equals_a_batch_member_of_the_same_map_mask_profile_and_fields(sfl, masked):
    dim_x, dim_y = 61, 81
    open, solid, records = case(dim_x, dim_y, masked)
    v, c = fields_of(dim_x, dim_y)
    cells, vel = [c_ for c_, _ in records], [u for _, u in records]
    with make(sfl, dim_x, dim_y, masked) as s, sfl.BatchSolver(dim_x, dim_y, 2) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, np.stack([v, v]))
        b.upload(sfl.capi.FIELD_COLOR, np.stack([c, c]))
        if solid.any():
            b.set_solids(solid)
        b.set_openings(open, INFLOW)
        b.set_inflow_profile(cells, vel)
        assert s.openings_flux().tobytes() == b.openings_flux()[1].tobytes(), "the flux before a step"
        s.step_n(3, DT, DX, ITERS, OMEGA)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        cap = sfl.capi
        for field in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR):
            got, want = s.download(field), b.download(field)[1]
            assert np.array_equal(np.ascontiguousarray(got).view(np.uint32), np.ascontiguousarray(want).view(np.uint32)), field
        flux = s.openings_flux()
        assert flux.tobytes() == b.openings_flux()[1].tobytes() and int(flux["inflow"]) != 0, "the flux record"
        assert flux.tobytes() == rule.flux(s.download(cap.FIELD_VELOCITY), open, solid).tobytes()
