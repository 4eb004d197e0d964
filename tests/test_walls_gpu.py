"""Wall velocities in batches on the GPU (include/sfl.h "WALL VELOCITIES"; csrc/batch_walls.hip, csrc/walls.cpp): every field
after three steps is bit for bit what tests/wall_rule.py computes -- step_n and step_n_each, shared and per-member tables and
masks, with and without item 3a, with openings and a profile in the same step -- and the anchors: a table of +0.0f and a
cleared table give the bits of the batch without one, n steps of one call are n calls of one step, a new mask drops the table.
There are no tolerances: every comparison is of bits."""
import functools

import numpy as np
import pytest

import wall_rule as rule
from conftest import random_fields
from test_openings_gpu import IN, OUT
from test_solids_gpu import assert_fields_equal, assert_members_equal, download_all, queue

pytestmark = pytest.mark.gpu

F = np.float32
DT, DX, ITERS, OMEGA = 1 / 30.0, 0.5, 5, 1.9
SHAPES = [(3, 3), (7, 5), (61, 81), (96, 64)]
IDS = [f"{x}x{y}" for x, y in SHAPES]
B = 4
NU = np.array([0.05, 0.0, 0.3, 0.01], F)   # member 1 skips item 3a
EACH = dict(dt=[1 / 30.0, 1 / 60.0, 1 / 20.0, 1 / 45.0], dx=[0.5, 1.0, 1.3, 0.37], iters=[5, 8, 3, 0], omega=[1.9, 1.5, 1.96, 1.7])
DENORMAL, LARGEST = F(1e-44), np.finfo(F).max
INFLOW = np.array([(3.5, 0.0), (2.0, 1.5), (-0.0, 0.0), (1.25, -0.5)], F)


def lid(dim_x, dim_y):
    m = np.zeros((dim_y, dim_x), bool)
    m[-1, :] = True   # the top rim row, both corners included
    return m


def disc(dim_x, dim_y):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return (i - dim_x // 2) ** 2 + (j - dim_y // 2) ** 2 <= (min(dim_x, dim_y) // 4) ** 2


@functools.lru_cache(maxsize=None)
def masks_of(dim_x, dim_y, per_member):
    """bool[B, dim_y, dim_x].  3 x 3: the centre cell alone, every fluid cell on the rim.  Else shared: a lid and a disc in
    every member; per member: a lid | a disc | a lid and the cell (0, 1) beside the inflow cell (0, 2) | a lid and a disc,
    and in every member the corner cell (dim_x - 1, 0), so that a table all members share has a cell to name."""
    if (dim_x, dim_y) == (3, 3):
        one = np.zeros((3, 3), bool)
        one[1, 1] = True
        masks = np.stack([one] * B)
    else:
        both = lid(dim_x, dim_y) | disc(dim_x, dim_y)
        beside = lid(dim_x, dim_y).copy()
        beside[1, 0] = True
        masks = np.stack([both] * B if not per_member else [lid(dim_x, dim_y), disc(dim_x, dim_y), beside, both])
        masks[:, 0, -1] = True
    masks.setflags(write=False)
    return masks


def wall_values(k):
    """Ordinary values beside a -0.0f and a denormal."""
    special = [(F(-0.0), F(1.5)), (DENORMAL, F(-2.0))]
    return special[k] if k < 2 else (F(0.5 + 0.25 * (k % 5)), F(-1.0 + 0.125 * (k % 9)))


def largest_of(dim_x, dim_y, mask):
    """The records that carry the largest finite float: the disc's centre cell and the one east of it, where the disc is at
    least eight cells deep.  One sample of 3.4e38 overflows a step to Inf and NaN within three steps, and the reference's
    advection, which the rule runs, indexes with the velocity it is handed: it does not survive a NaN.  So the value sits
    where no back-trace of these fields reaches (they move a few cells per step) and no fluid cell is a neighbour; the small
    shapes, where every wall cell touches a fluid one, carry none.  What that leaves for THIS value: only item 8's store of the
    bits as given into the velocity is observed.  The extended item 3 is NOT exercised for it -- no reader of the step's working
    velocity (item 3a, the divergence) ever sees the cell; the -0.0f, the denormal and the ordinary values, which sit on cells
    with fluid neighbours, are what holds item 3 and its readers to the rule."""
    cx, cy = dim_x // 2, dim_y // 2
    if min(dim_x, dim_y) // 4 < 8 or not (mask[cy, cx] and mask[cy, cx + 1]):
        return []
    return [((cx, cy), (F(0.75), LARGEST)), ((cx + 1, cy), (-LARGEST, F(-0.0)))]


def tables_of(dim_x, dim_y, per_member, mode):
    """(members or None, cells, vel, per member the records in the order given).  shared: every solid cell all members share,
    in an order that is not the cells', one cell named twice; members: per member its own solid cells with its own values,
    member 2 without a record, a later record on a cell of member 0."""
    masks = masks_of(dim_x, dim_y, per_member)
    if mode == "shared":
        common = np.logical_and.reduce(masks)
        cells = [(int(i), int(j)) for j, i in zip(*np.nonzero(common))][::-1]
        cells = [cells[len(cells) // 2]] + cells
        vel = [(F(77.0), F(-77.0))] + [wall_values(k) for k in range(len(cells) - 1)]
        for c, u in largest_of(dim_x, dim_y, common):
            cells.append(c), vel.append(u)
        return None, cells, vel, [list(zip(cells, vel))] * B
    who, cells, vel = [], [], []
    for m in (3, 0, 1):
        for k, (j, i) in enumerate(zip(*np.nonzero(masks[m]))):
            who.append(m), cells.append((int(i), int(j))), vel.append(wall_values(k + m))
        for c, u in largest_of(dim_x, dim_y, masks[m]):
            who.append(m), cells.append(c), vel.append(u)
    again = [c for w, c in zip(who, cells) if w == 0][2 % sum(w == 0 for w in who)]
    who.append(0), cells.append(again), vel.append((F(-3.0), F(3.0)))
    return who, cells, vel, [[(c, u) for w, c, u in zip(who, cells, vel) if w == m] for m in range(B)]


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    v, c = zip(*(random_fields(dim_x, dim_y, 900 + m, vamp=40.0)[:2] for m in range(B)))
    v, c = np.stack(v), np.stack(c)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y):
    """step -> [(member, i, j, vx, vy)]: on the wall cell at the grid's centre or top row (no effect), on a fluid cell."""
    return {0: [(m, dim_x // 2, dim_y - 1, 55.0, 66.0) for m in range(B)] + [(m, dim_x // 2, dim_y // 2, 5.0, 6.0) for m in range(B)],
            1: [(m, 0, 0, -12.5, 7.25) for m in range(B)]}


@functools.lru_cache(maxsize=None)
def open_map(dim_x, dim_y):
    """West column an inflow, east column an outflow (3 x 3: one cell each)."""
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[1:-1, 0], m[1:-1, -1] = IN, OUT
    m.setflags(write=False)
    return m


def profile_of(dim_x, dim_y):
    return [((0, j), (F(1.0 + j), F(0.25))) for j in range(1, dim_y - 1, 2)]


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, per_member, mode, sweeps, each, opened, steps=3):
    """The members after `steps` steps of the rule: [(v, div, p, colour)].  Computed once, shared, never written.  mode None:
    no table; opened: False, "uniform" (openings alone) or "profile" (with the records of profile_of)."""
    from oracle import loader
    cpu = loader.port()
    masks = masks_of(dim_x, dim_y, per_member)
    v, c = fields_of(dim_x, dim_y)
    forces = forces_of(dim_x, dim_y)
    rows = tables_of(dim_x, dim_y, per_member, mode)[3] if mode else [[] for _ in range(B)]
    out = []
    for m in range(B):
        dt, dx, iters, omega = (EACH["dt"][m], EACH["dx"][m], EACH["iters"][m], EACH["omega"][m]) if each else (DT, DX, ITERS, OMEGA)
        extra = dict(open=open_map(dim_x, dim_y), inflow=INFLOW[m], profile=profile_of(dim_x, dim_y) if opened == "profile" else ()) if opened else dict(nu=NU[m], sweeps=sweeps)
        state = (v[m], None, None, c[m])
        for k in range(steps):
            mine = [r[1:] for r in forces.get(k, []) if r[0] == m]
            state = rule.step(cpu, state[0], state[3], masks[m], rows[m], dt, dx, iters, omega, mine, **extra)
            assert np.isfinite(state[0]).all(), "the rule's own fields stay finite: the reference's advection needs that"
        out.append(state)
    return out


def reload(sfl, b, dim_x, dim_y):
    v, c = fields_of(dim_x, dim_y)
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)


def make(sfl, dim_x, dim_y, per_member, sweeps=0, opened=False, table=None):
    masks = masks_of(dim_x, dim_y, per_member)
    b = sfl.BatchSolver(dim_x, dim_y, B)
    reload(sfl, b, dim_x, dim_y)
    b.set_solids(masks if per_member else masks[0])
    if opened:
        b.set_openings(open_map(dim_x, dim_y), INFLOW)
        if opened == "profile":
            cells, vel = zip(*profile_of(dim_x, dim_y))
            b.set_inflow_profile(list(cells), list(vel))
    elif sweeps:
        b.set_viscosity(NU, sweeps)
    if table is not None and table[1]:
        b.set_wall_velocity(table[1], table[2], table[0])
    return b


def step3(b, each, n=3):
    if each:
        b.step_n_each(n, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
    else:
        b.step_n(n, DT, DX, ITERS, OMEGA)


def test_the_members_hold_the_cases_they_are_there_for():
    for dim_x, dim_y in SHAPES:
        for per_member in (False, True):
            masks = masks_of(dim_x, dim_y, per_member)
            for mode in ("shared", "members"):
                who, cells, vel, rows = tables_of(dim_x, dim_y, per_member, mode)
                for m in range(B):
                    assert rule.check_table(rows[m], masks[m]) is None
                if cells:
                    assert len(rule.unique(rows[0])) < len(rows[0]), "a cell is named twice"
                if mode == "members":
                    assert not rows[2] and rows[3], "member 2 has no record"
            bits = np.array([u for row in tables_of(dim_x, dim_y, per_member, "members")[3] for _, u in rule.unique(row)], F).view(np.uint32)
            if (dim_x, dim_y) != (3, 3):
                assert 0x80000000 in bits and DENORMAL.view(np.uint32) in bits
            if min(dim_x, dim_y) >= 32:
                assert LARGEST.view(np.uint32) in bits and (-LARGEST).view(np.uint32) in bits
        if (dim_x, dim_y) != (3, 3):
            masks = masks_of(dim_x, dim_y, True)
            assert masks[0][-1, 0] and masks[0][-1, -1], "the rim row with both corners"
            assert masks[2][1, 0] and open_map(dim_x, dim_y)[2, 0] == IN and not masks[2][2, 0], "a wall cell beside an inflow cell"
    assert masks_of(3, 3, False)[0].sum() == 1 and masks_of(3, 3, False)[0][1, 1]
    assert NU[1] == 0


# ---- 1. the step against the rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
@pytest.mark.parametrize("sweeps", [0, 3], ids=["inviscid", "sweeps3"])
@pytest.mark.parametrize("per_member,mode", [(False, "shared"), (True, "members"), (True, "shared"), (False, "members")],
                         ids=["mask1-table1", "maskB-tableB", "maskB-table1", "mask1-tableB"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_with_a_wall_table_are_three_steps_of_the_rule(sfl, dim_x, dim_y, per_member, mode, sweeps, each):
    table = tables_of(dim_x, dim_y, per_member, mode)
    want = rule_steps(dim_x, dim_y, per_member, mode, sweeps, each, False)
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, per_member, sweeps, False, table) as b:
        held = sum(len(rule.unique(row)) for row in table[3])
        assert b.wall_velocity_info() == (True, held)
        for m in range(B):
            cells, vel = b.wall_velocity(m)
            rows = rule.unique(table[3][m])
            assert [tuple(c) for c in cells] == [c for c, _ in rows], "the records come back in cell order, duplicates removed"
            assert np.array_equal(vel.view(np.uint32), np.array([u for _, u in rows], F).reshape(-1, 2).view(np.uint32))
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, each)
        once = download_all(sfl, b)
        assert_members_equal(once, want, "three steps in one call")
        # ... and one step called three times gives the same bits (anchor c)
        reload(sfl, b, dim_x, dim_y)
        for k in range(3):
            queue(b, forces.get(k, []))
            step3(b, each, 1)
        assert_fields_equal(download_all(sfl, b), once, "one step x 3")


@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
@pytest.mark.parametrize("mode", ["shared", "members"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_with_walls_openings_and_a_profile_are_three_steps_of_the_rule(sfl, dim_x, dim_y, mode, each):
    table = tables_of(dim_x, dim_y, True, mode)
    want = rule_steps(dim_x, dim_y, True, mode, 0, each, "profile")
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, True, 0, "profile", table) as b:
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, each)
        assert_members_equal(download_all(sfl, b), want, "three steps in one call")
        # ... and without the profile: the same kernels with no row of it
        b.set_inflow_profile(None, None)
        reload(sfl, b, dim_x, dim_y)
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, each)
        assert_members_equal(download_all(sfl, b), rule_steps(dim_x, dim_y, True, mode, 0, each, "uniform"), "the openings without a profile")


# ---- 2. the anchors ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sweeps,opened", [(0, False), (3, False), (0, "uniform"), (0, "profile")], ids=["solids", "viscous", "openings", "profile"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_a_table_of_zeros_a_cleared_table_and_a_new_mask_give_the_bits_of_the_batch_without_one(sfl, dim_x, dim_y, sweeps, opened):
    masks = masks_of(dim_x, dim_y, True)
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, True, sweeps, opened) as b:
        assert b.wall_velocity_info() == (False, 0)
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, False)
        plain = download_all(sfl, b)
    assert_members_equal(plain, rule_steps(dim_x, dim_y, True, None, sweeps, False, opened), "no table: the rule without one")
    who, cells = zip(*[(m, (int(i), int(j))) for m in range(B) for j, i in zip(*np.nonzero(masks[m]))])
    zeros = np.zeros((len(cells), 2), F)
    moving = tables_of(dim_x, dim_y, True, "members")
    with make(sfl, dim_x, dim_y, True, sweeps, opened) as b:
        b.set_wall_velocity(list(cells), zeros, list(who))   # anchor (a)
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, False)
        assert_fields_equal(download_all(sfl, b), plain, "a table of +0.0f")
        b.set_wall_velocity(moving[1], moving[2], moving[0])
        b.set_wall_velocity(None, None)   # cleared
        assert b.wall_velocity_info() == (False, 0) and len(b.wall_velocity(0)[0]) == 0
        reload(sfl, b, dim_x, dim_y)
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, False)
        assert_fields_equal(download_all(sfl, b), plain, "a cleared table")
        b.set_wall_velocity(moving[1], moving[2], moving[0])
        b.set_solids(masks)   # the same mask again: the table goes all the same
        assert b.wall_velocity_info() == (False, 0)
        reload(sfl, b, dim_x, dim_y)
        for k, records in forces.items():
            queue(b, records, k)
        step3(b, False)
        assert_fields_equal(download_all(sfl, b), plain, "a new mask drops the table")


def test_from_rest_a_lid_moves_nothing_without_viscosity_and_drags_the_row_beside_it_with(sfl):
    dim_x, dim_y = 61, 81
    cells = [(i, dim_y - 1) for i in range(dim_x)]
    for u in (2.5, -2.5):
        vel = [(u, 0.0)] * dim_x
        with sfl.BatchSolver(dim_x, dim_y, 3) as b:
            b.set_solids(lid(dim_x, dim_y))
            b.set_viscosity(np.array([0.0, 0.05, 0.5], F), 3)
            b.set_wall_velocity(cells, vel)
            b.step_n(1, DT, DX, ITERS, OMEGA)
            v = b.download(sfl.capi.FIELD_VELOCITY)
            assert np.all(v[0][:-1] == 0), "nu = 0: every fluid cell compares equal to zero"
            for m in (1, 2):
                assert np.all(np.sign(v[m][-2, :, 0]) == np.sign(u)), "the row beside the lid has the sign of the lid's u"
            assert np.array_equal(v[:, -1], np.broadcast_to(np.array(vel, F), (3, dim_x, 2))), "item 8: the lid holds its velocity"
            b.set_viscosity(None, 0)
            b.upload(sfl.capi.FIELD_VELOCITY, np.zeros_like(v))
            b.step_n(3, DT, DX, ITERS, OMEGA)
            v = b.download(sfl.capi.FIELD_VELOCITY)
            assert np.all(v[:, :-1] == 0), "no viscosity, three steps from rest: every fluid cell compares equal to zero"


# ---- 3. the recorders behind a step ---------------------------------------------------------------------------------------
def test_the_samples_of_the_body_recorders_behind_a_step_are_the_queries_after_it(sfl):
    dim_x, dim_y = 61, 81
    table = tables_of(dim_x, dim_y, True, "members")
    masks = masks_of(dim_x, dim_y, True)
    with make(sfl, dim_x, dim_y, True, 3, False, table) as b:
        b.set_bodies(masks.astype(np.uint8))
        b.loads_start(1, 2), b.friction_start(1, 2), b.torque_start(1, 2)
        for k in range(2):
            step3(b, False, 1)
            for query, history in ((b.loads, b.loads_history), (b.friction, b.friction_history), (b.torque, b.torque_history)):
                assert history()[k].tobytes() == query().tobytes(), (k, query.__name__)


# ---- 4. the refusals that need a batch -------------------------------------------------------------------------------------
def test_refusals_leave_the_table_as_it_was(sfl):
    dim_x, dim_y = 7, 5
    masks = masks_of(dim_x, dim_y, True)
    table = tables_of(dim_x, dim_y, True, "members")
    cap = sfl.capi
    with sfl.BatchSolver(dim_x, dim_y, B) as b:
        with pytest.raises(sfl.SflError, match="no solids set") as e:
            b.set_wall_velocity([(0, 0)], [(1.0, 0.0)])
        assert e.value.code == cap.ERR_STATE
        b.set_wall_velocity(None, None)   # clearing nothing is fine
        b.set_solids(masks)
        b.set_wall_velocity(table[1], table[2], table[0])
        before = [b.wall_velocity(m) for m in range(B)]
        fluid = (1, 1)
        assert not masks[:, 1, 1].any()
        for args, words in ((([(0, dim_y - 1), fluid], [(1.0, 0.0)] * 2, [0, 0]), "record 1 names cell (1, 1), which is not solid in the mask of member 0"),
                            (([(0, dim_y - 1)], [(1.0, 0.0)]), "record 0 names cell (0, 4), which is not solid in the mask of member 1"),
                            (([(dim_x, 0)], [(1.0, 0.0)]), "record 0 names cell (7, 0), which is not inside the grid of 7 x 5"),
                            (([(0, dim_y - 1)], [(1.0, 0.0)], [B]), "record 0 names member 4"),
                            (([(0, dim_y - 1)], [(np.inf, 0.0)]), "must be finite (record 0")):
            with pytest.raises(sfl.SflError) as e:
                b.set_wall_velocity(*args)
            assert e.value.code == cap.ERR_INVALID and words in str(e.value), (words, str(e.value))
            after = [b.wall_velocity(m) for m in range(B)]
            assert all(np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32)) for x, y in zip(before, after))
        assert b.wall_velocity_info()[0]


# ---- 5. the relative figures ---------------------------------------------------------------------------------------------
def test_relative_friction_and_torque_subtract_the_walls_share_and_leave_the_records_alone(sfl):
    dim_x, dim_y = 61, 81
    masks = masks_of(dim_x, dim_y, True)
    labels = masks.astype(np.uint8)
    labels[:, -1, :] *= 2   # the lid is body 2 where there is one, everything else body 1
    pivots = np.array([[dim_x // 2, dim_y // 2], [0.5, dim_y - 1]], np.float64)
    table = tables_of(dim_x, dim_y, True, "members")
    with make(sfl, dim_x, dim_y, True, 3, False, None) as b:
        b.set_bodies(labels, 2)
        b.set_body_pivots(pivots)
        step3(b, False)
        records = b.friction().tobytes(), b.torque().tobytes()
        plain_f, plain_t = b.friction_xy(), b.torque_xy(DX)
        assert np.array_equal(b.friction_xy(relative=True), plain_f) and np.array_equal(b.torque_xy(DX, relative=True), plain_t), "no table: no share"
        b.set_wall_velocity(table[1], table[2], table[0])
        assert (b.friction().tobytes(), b.torque().tobytes()) == records, "the records keep their definition: no byte moves"
        shares = [sfl.wall_shares(masks[m], labels[m], 2, np.round(2 * pivots).astype(int), *b.wall_velocity(m)) for m in range(B)]
        nu = NU.astype(np.float64)[:, None]
        assert np.array_equal(b.friction_xy(relative=True), nu[:, :, None] * (b.friction_xy(1.0) - np.stack([f for f, _ in shares])))
        want_t = plain_t.copy()
        want_t[..., 1] -= np.stack([t for _, t in shares]) * nu * DX
        assert np.array_equal(b.torque_xy(DX, relative=True), want_t)
        assert np.array_equal(b.friction_xy(relative=True)[2], plain_f[2]), "member 2 has no record"
        assert not np.array_equal(b.friction_xy(relative=True)[0], plain_f[0])
    with sfl.Solver(dim_x, dim_y) as s:
        s.set_solids(masks[3])
        s.set_viscosity(0.3, 3)
        s.set_bodies(labels[3], 2)
        s.set_body_pivots(pivots)
        cells, vel = zip(*rule.unique(table[3][3]))
        s.set_wall_velocity(list(cells), list(vel))
        s.step(DT, DX, ITERS, OMEGA)
        f, t = sfl.wall_shares(masks[3], labels[3], 2, np.round(2 * pivots).astype(int), *s.wall_velocity())
        assert np.array_equal(s.friction_xy(relative=True), np.float64(np.float32(0.3)) * (s.friction_xy(1.0) - f[None]))
        want_t = s.torque_xy(DX)
        want_t[..., 1] -= t[None] * np.float64(np.float32(0.3)) * DX
        assert np.array_equal(s.torque_xy(DX, relative=True), want_t)
