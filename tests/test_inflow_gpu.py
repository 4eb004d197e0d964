"""Inflow profiles and the flux of a batch on the GPU (include/sfl.h "INFLOW PROFILES AND FLUX"; csrc/batch_openings.hip's
profile kernels, csrc/inflow.hip) against tests/inflow_rule.py, bit for bit.

Shapes: 3 x 3 (one open cell per side: the smallest grid that carries an opening), 7 x 5, 61 x 81 and 96 x 64 (6144 cells, the
largest member); five members with a map each.  A profile shared by all members and records per member through `members`; a force
record on a profiled cell and a solid cell under one (neither has an effect); with and without masks; step_n and step_n_each."""
import functools

import numpy as np
import pytest

import inflow_rule as rule
from conftest import random_fields
from test_openings_gpu import IN, map_of
from test_solids_gpu import assert_fields_equal, assert_members_equal, download_all, mask_of, queue

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 6, 1.9
SHAPES = [(3, 3), (7, 5), (61, 81), (96, 64)]
IDS = [f"{x}x{y}" for x, y in SHAPES]
B = 5
MAPS = ("four", "four", "west_east", "four", "in_only")   # every member's west column is an inflow
INFLOW = np.array([(3.5, 0.0), (2.0, 1.5), (-0.0, 0.0), (1.25, -0.5), (1.5, 0.0)], np.float32)
EACH = dict(dt=[1 / 30.0, 1 / 60.0, 1 / 20.0, 1 / 45.0, 1 / 30.0], dx=[0.7, 1.0, 1.3, 0.37, 1.0], iters=[5, 8, 3, 9, 0], omega=[1.9, 1.5, 1.96, 1.7, 1.9])


@functools.lru_cache(maxsize=None)
def members_of(dim_x, dim_y, masked):
    """(maps uint8[B, dim_y, dim_x], masks bool[B, dim_y, dim_x]): member 1 has a solid cell under the profiled inflow cell
    (0, dim_y // 2), member 2 a disc, member 3 a solid cell under the south inflow cell (dim_x // 2, 0)."""
    maps = np.stack([map_of(k, dim_x, dim_y) for k in MAPS])
    masks = np.zeros((B, dim_y, dim_x), bool)
    if masked:
        masks[1, dim_y // 2, 0] = True
        masks[2] = mask_of("disc", dim_x, dim_y)
        masks[3, 0, dim_x // 2] = True
    maps.setflags(write=False)
    masks.setflags(write=False)
    return maps, masks


def profiles_of(dim_x, dim_y, mode):
    """(members or None, cells, vel, per member the records in the order given).  shared: a parabola over the west column with
    one cell named twice; members: per member another peak, the south row too where the member's map opens it, in an order that
    is not the cells' and not the members'."""
    west = [(0, j) for j in range(1, dim_y - 1)]
    s = [(j - 0.5) / (dim_y - 2) for j in range(1, dim_y - 1)]
    if mode == "shared":
        cells = [west[len(west) // 2]] + west[::-1]
        vel = [(77.0, -77.0)] + [(np.float32(8.0 * 4 * x * (1 - x)), np.float32(0.25)) for x in s[::-1]]
        return None, cells, vel, [list(zip(cells, vel))] * B
    who, cells, vel = [], [], []
    for m in (3, 0, 4, 1):   # member 2 gets no record: the uniform inflow alone
        for (i, j), x in zip(west, s):
            who.append(m), cells.append((i, j)), vel.append((np.float32((m + 1) * 4 * x * (1 - x)), np.float32(-0.0)))
        if MAPS[m] == "four":
            for i in range(1, dim_x - 1, 2):
                who.append(m), cells.append((i, 0)), vel.append((np.float32(0.5), np.float32(1.0 + i)))
    who.append(0), cells.append(west[0]), vel.append((np.float32(-3.0), np.float32(3.0)))   # a later record on a cell of member 0
    return who, cells, vel, [[(c, u) for w, c, u in zip(who, cells, vel) if w == m] for m in range(B)]


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    v, c = zip(*(random_fields(dim_x, dim_y, 700 + m, vamp=40.0)[:2] for m in range(B)))
    v, c = np.stack(v), np.stack(c)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y):
    """step -> [(member, i, j, vx, vy)]: on the profiled inflow cell (0, dim_y // 2) of every member (no effect), on a cell inside."""
    return {0: [(m, 0, dim_y // 2, 55.0, 66.0) for m in range(B)], 1: [(m, dim_x // 2, dim_y // 2, -12.5, 7.25) for m in range(B)]}


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, mode, masked, each, steps=3):
    from oracle import loader
    cpu = loader.port()
    maps, masks = members_of(dim_x, dim_y, masked)
    v, c = fields_of(dim_x, dim_y)
    forces, rows = forces_of(dim_x, dim_y), profiles_of(dim_x, dim_y, mode)[3]
    out = []
    for m in range(B):
        dt, dx, iters, omega = (EACH["dt"][m], EACH["dx"][m], EACH["iters"][m], EACH["omega"][m]) if each else (DT, DX, ITERS, OMEGA)
        state = (v[m], None, None, c[m])
        for k in range(steps):
            mine = [r[1:] for r in forces.get(k, []) if r[0] == m]
            state = rule.step(cpu, state[0], state[3], masks[m], maps[m], INFLOW[m], rows[m], dt, dx, iters, omega, mine)
        out.append(state)
    return out


def make(sfl, dim_x, dim_y, masked, profile=None):
    maps, masks = members_of(dim_x, dim_y, masked)
    b = sfl.BatchSolver(dim_x, dim_y, B)
    reload(sfl, b, dim_x, dim_y)
    if masked:
        b.set_solids(masks)
    b.set_openings(maps, INFLOW)
    if profile is not None:
        who, cells, vel, _ = profile
        b.set_inflow_profile(cells, vel, who)
    return b


def reload(sfl, b, dim_x, dim_y):
    v, c = fields_of(dim_x, dim_y)
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)


def step3(b, each, n=3):
    if each:
        b.step_n_each(n, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
    else:
        b.step_n(n, DT, DX, ITERS, OMEGA)


def test_the_members_hold_the_cases_they_are_there_for():
    for dim_x, dim_y in SHAPES:
        maps, masks = members_of(dim_x, dim_y, True)
        assert maps[1][dim_y // 2, 0] == IN and masks[1][dim_y // 2, 0] and maps[3][0, dim_x // 2] == IN and masks[3][0, dim_x // 2]
        for mode in ("shared", "members"):
            who, cells, vel, rows = profiles_of(dim_x, dim_y, mode)
            for m in range(B):
                assert rule.check_profile(rows[m], maps[m]) is None
            assert len(rule.unique(rows[0])) < len(rows[0]), "a cell is named twice"
        assert (0, dim_y // 2) in [c for c, _ in rows[1]], "member 1's solid inflow cell carries a record"
        assert not rows[2] and rows[3]


# ---- 1. the step against the rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("mode", ["shared", "members"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_with_a_profile_are_three_steps_of_the_rule(sfl, dim_x, dim_y, mode, masked, each):
    profile = profiles_of(dim_x, dim_y, mode)
    want = rule_steps(dim_x, dim_y, mode, masked, each)
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, masked, profile) as b:
        held = sum(len(rule.unique(row)) for row in profile[3])
        assert b.inflow_profile_info() == (True, held)
        for m in range(B):
            cells, vel = b.inflow_profile(m)
            rows = rule.unique(profile[3][m])
            assert [tuple(c) for c in cells] == [c for c, _ in rows], "the records come back in cell order, duplicates removed"
            assert np.array_equal(vel.view(np.uint32), np.array([u for _, u in rows], np.float32).reshape(-1, 2).view(np.uint32))
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, each)
        once = download_all(sfl, b)
        assert_members_equal(once, want, "three steps in one call")
        # ... and one step called three times gives the same bits
        reload(sfl, b, dim_x, dim_y)
        for k in range(3):
            queue(b, forces.get(k, []))
            step3(b, each, 1)
        assert_fields_equal(download_all(sfl, b), once, "one step x 3")


# ---- 2. the anchor -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_a_uniform_profile_and_a_cleared_profile_give_the_bits_of_the_batch_without_one(sfl, dim_x, dim_y, masked):
    maps, _ = members_of(dim_x, dim_y, masked)
    who, cells, vel = [], [], []
    for m in range(B):   # every inflow cell of every member, named with the member's uniform inflow
        for j, i in np.argwhere(maps[m] == IN):
            who.append(m), cells.append((int(i), int(j))), vel.append(tuple(INFLOW[m]))
    forces = forces_of(dim_x, dim_y)

    def run(b):
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, False, 2)
        step3(b, True, 1)
        return download_all(sfl, b), b.residual()

    with make(sfl, dim_x, dim_y, masked) as plain, make(sfl, dim_x, dim_y, masked, (who, cells, vel, None)) as uniform, \
            make(sfl, dim_x, dim_y, masked, profiles_of(dim_x, dim_y, "members")) as cleared:
        want = run(plain)
        assert plain.inflow_profile_info() == (False, 0) and uniform.inflow_profile_info() == (True, len(cells))
        got = run(uniform)
        assert_fields_equal(got[0], want[0], "a uniform profile")
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))
        other = run(cleared)
        assert not np.array_equal(other[0][0], want[0][0]), "a profile is another flow"
        reload(sfl, cleared, dim_x, dim_y)
        cleared.set_inflow_profile(None, None)
        assert cleared.inflow_profile_info() == (False, 0) and len(cleared.inflow_profile(0)[0]) == 0
        got = run(cleared)
        assert_fields_equal(got[0], want[0], "a cleared profile")
        # a new map drops a profile; set_inflow keeps one
        uniform.set_inflow(INFLOW)
        assert uniform.inflow_profile_info() == (True, len(cells))
        uniform.set_openings(maps, INFLOW)
        assert uniform.inflow_profile_info() == (False, 0)


# ---- 3. the flux ---------------------------------------------------------------------------------------------------------
def assert_flux_is_the_rules(sfl, b, maps, masks, what):
    v = b.download(sfl.capi.FIELD_VELOCITY)
    got = b.openings_flux()
    assert got.dtype == sfl.OPEN_FLUX_DTYPE and got.shape == (B,)
    for m in range(B):
        want = rule.flux(v[m], maps[m], masks[m])
        assert got[m].tobytes() == want.tobytes(), (what, m, got[m], want)
    part = b.openings_flux(1, 3)
    assert part.tobytes() == got[1:4].tobytes(), "a range of members"
    return got


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_flux_after_no_step_and_after_three_is_the_rules_record_byte_for_byte(sfl, dim_x, dim_y, masked):
    maps, masks = members_of(dim_x, dim_y, masked)
    with make(sfl, dim_x, dim_y, masked, profiles_of(dim_x, dim_y, "shared")) as b:
        assert_flux_is_the_rules(sfl, b, maps, masks, "after no step")
        step3(b, False)
        got = assert_flux_is_the_rules(sfl, b, maps, masks, "after three steps")
        assert (got["inflow_cells"] > 0).all() and (got["nonfinite"] == 0).all() and (got["inflow"] != 0).any()
        xy = sfl.openings_flux_xy(got)
        assert xy.shape == (B, 2) and np.array_equal(xy[0], rule.flux_xy(got[0]))


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_the_flux_counts_a_nan_and_an_inf_and_sums_the_rest_and_reports_zeros_where_nothing_is_live(sfl, dim_x, dim_y):
    maps, _ = members_of(dim_x, dim_y, False)
    masks = np.zeros((B, dim_y, dim_x), bool)
    masks[4] = maps[4] != 0   # every open cell of member 4 is solid
    v = fields_of(dim_x, dim_y)[0].copy()
    v[0, dim_y // 2, 0, 0] = np.nan      # member 0: a NaN on a west inflow cell
    v[1, dim_y // 2, -1, 0] = -np.inf    # member 1: an Inf on an east outflow cell
    v[1, 0, dim_x // 2, 1] = np.nan      # ... and a NaN on a south inflow cell
    v[3, dim_y // 2, 0, 1] = np.nan      # member 3: the tangential component of a west cell -- no part of n
    v[2] *= np.float32(1e-42)            # member 2: denormal normals
    with sfl.BatchSolver(dim_x, dim_y, B) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        assert b.openings_flux().tobytes() == bytes(40 * B), "a batch without openings reports zeros"
        b.set_solids(masks)
        b.set_openings(maps, INFLOW)
        got = assert_flux_is_the_rules(sfl, b, maps, masks, "planted")
        assert [int(n) for n in got["nonfinite"]] == [1, 2, 0, 0, 0]
        assert got[4].tobytes() == bytes(40) and int(got[2]["exp2"]) < -126 - 32
        b.set_openings(None)
        assert b.openings_flux().tobytes() == bytes(40 * B), "cleared: zeros again"
