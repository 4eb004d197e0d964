"""Wall velocities in whole-domain contexts on the GPU (include/sfl.h "WALL VELOCITIES"; csrc/context_walls.hip,
csrc/context_walls.cpp): every field after three steps is bit for bit what tests/wall_rule.py computes, at 61 x 81 -- where a
context holds what a batch member of that shape holds (anchor b) -- and at 130 x 70, three by three ragged tiles of the
diffusion, with wall cells on both sides of a tile seam so that a window reads a wall out of its halo; with three sweeps and
with nine, which is two launches; with and without openings; step against step_n; the download and the refusals.  There are no
tolerances: every comparison is of bits."""
import functools

import numpy as np
import pytest

import wall_rule as rule
from conftest import assert_bit_equal, random_fields
from test_openings_gpu import IN, OUT

pytestmark = pytest.mark.gpu

F = np.float32
DT, DX, ITERS, OMEGA, NU = 1 / 30.0, 0.5, 5, 1.9, 0.3
NAMES = ("velocity", "divergence", "pressure", "colour")
SHAPES = [(61, 81), (130, 70)]
IDS = [f"{x}x{y}" for x, y in SHAPES]


@functools.lru_cache(maxsize=None)
def mask_of(dim_x, dim_y):
    """A lid on the top rim, and a block over columns 63, 64 and rows 31, 32 (130 x 70: across the seam of the tiles of 64 x
    32 cells) or at the same place from the centre (61 x 81)."""
    m = np.zeros((dim_y, dim_x), bool)
    m[-1, :] = True
    i0, j0 = (63, 31) if dim_x > 64 else (dim_x // 2, dim_y // 2)
    m[j0:j0 + 2, i0:i0 + 2] = True
    m.setflags(write=False)
    return m


def table_of(dim_x, dim_y):
    """Every solid cell, in an order that is not the cells', one cell named twice; a -0.0f and a denormal beside ordinary values."""
    cells = [(int(i), int(j)) for j, i in zip(*np.nonzero(mask_of(dim_x, dim_y)))][::-1]
    vel = [(F(0.5 + 0.25 * (k % 5)), F(-1.0 + 0.125 * (k % 9))) for k in range(len(cells))]
    vel[0], vel[1] = (F(-0.0), F(1.5)), (F(1e-44), F(-2.0))
    return [(cells[3], (F(77.0), F(-77.0)))] + list(zip(cells, vel))


@functools.lru_cache(maxsize=None)
def open_map(dim_x, dim_y):
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[1:-1, 0], m[1:-1, -1] = IN, OUT
    m.setflags(write=False)
    return m


def forces_of(dim_x, dim_y):
    """step -> [(i, j, vx, vy)]: on a lid cell (no effect), on a fluid cell."""
    return {0: [(dim_x // 2, dim_y - 1, 55.0, 66.0), (5, 6, 5.0, 6.0)], 1: [(1, 1, -12.5, 7.25)]}


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    v, c = random_fields(dim_x, dim_y, 900, vamp=40.0)[:2]   # (member 0 of tests/test_walls_gpu.py)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, sweeps, opened, walls=True, steps=3):
    from oracle import loader
    cpu = loader.port()
    v, c = fields_of(dim_x, dim_y)
    extra = dict(open=open_map(dim_x, dim_y), inflow=(F(3.5), F(0.25))) if opened else dict(nu=NU, sweeps=sweeps)
    state = (v, None, None, c)
    for k in range(steps):
        state = rule.step(cpu, state[0], state[3], mask_of(dim_x, dim_y), table_of(dim_x, dim_y) if walls else [], DT, DX, ITERS, OMEGA,
                          forces_of(dim_x, dim_y).get(k, []), **extra)
        assert np.isfinite(state[0]).all()
    return state


def make(sfl, dim_x, dim_y, sweeps, opened, walls=True):
    s = sfl.Solver(dim_x, dim_y)
    reload(sfl, s, dim_x, dim_y)
    s.set_solids(mask_of(dim_x, dim_y))
    if opened:
        s.set_openings(open_map(dim_x, dim_y), (3.5, 0.25))
    elif sweeps:
        s.set_viscosity(NU, sweeps)
    if walls:
        cells, vel = zip(*table_of(dim_x, dim_y))
        s.set_wall_velocity(list(cells), list(vel))
    return s


def reload(sfl, s, dim_x, dim_y):
    v, c = fields_of(dim_x, dim_y)
    s.upload(sfl.capi.FIELD_VELOCITY, v)
    s.upload(sfl.capi.FIELD_COLOR, c)


def download_all(sfl, s):
    cap = sfl.capi
    s.synchronize()
    return tuple(s.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))


def assert_fields(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_bit_equal(g, w, f"{what}: {name}")


def queue(s, records, step=0):
    if records:
        s.queue_forces([r[:2] for r in records], [r[2:] for r in records], step)


def test_the_cases_are_the_ones_the_shapes_are_there_for():
    m = mask_of(130, 70)
    assert m[31, 63] and m[31, 64] and m[32, 63] and m[32, 64] and m[-1].all() and not m[30, 63]
    for dim_x, dim_y in SHAPES:
        t = table_of(dim_x, dim_y)
        assert rule.check_table(t, mask_of(dim_x, dim_y)) is None and len(rule.unique(t)) == len(t) - 1 == mask_of(dim_x, dim_y).sum()


@pytest.mark.parametrize("sweeps,opened", [(0, False), (3, False), (9, False), (0, True)], ids=["inviscid", "sweeps3", "sweeps9", "openings"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_three_steps_of_a_context_are_three_steps_of_the_rule_and_of_a_batch_member(sfl, dim_x, dim_y, sweeps, opened):
    want = rule_steps(dim_x, dim_y, sweeps, opened)
    forces = forces_of(dim_x, dim_y)
    rows = rule.unique(table_of(dim_x, dim_y))
    with make(sfl, dim_x, dim_y, sweeps, opened) as s:
        assert s.wall_velocity_info() == len(rows)
        cells, vel = s.wall_velocity()
        assert [tuple(c) for c in cells] == [c for c, _ in rows], "the records come back in cell order, duplicates removed"
        assert np.array_equal(vel.view(np.uint32), np.array([u for _, u in rows], F).reshape(-1, 2).view(np.uint32))
        for k, records in forces.items():
            queue(s, records, k)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        once = download_all(sfl, s)
        assert_fields(once, want, "step_n(3)")
        reload(sfl, s, dim_x, dim_y)
        for k in range(3):
            queue(s, forces.get(k, []))
            s.step(DT, DX, ITERS, OMEGA)
        assert_fields(download_all(sfl, s), once, "step x 3")
    if (dim_x, dim_y) == (61, 81):   # anchor (b)
        with sfl.BatchSolver(dim_x, dim_y, 2) as b:
            v, c = fields_of(dim_x, dim_y)
            b.upload(sfl.capi.FIELD_VELOCITY, np.stack([v, v]))
            b.upload(sfl.capi.FIELD_COLOR, np.stack([c, c]))
            b.set_solids(mask_of(dim_x, dim_y))
            if opened:
                b.set_openings(open_map(dim_x, dim_y), (3.5, 0.25))
            elif sweeps:
                b.set_viscosity(NU, sweeps)
            cells, vel = zip(*table_of(dim_x, dim_y))
            b.set_wall_velocity(list(cells), list(vel))
            for k, records in forces.items():
                b.queue_forces([1] * len(records), [r[:2] for r in records], [r[2:] for r in records], k)
            b.step_n(3, DT, DX, ITERS, OMEGA)
            cap = sfl.capi
            member = tuple(b.download(f)[1] for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
        assert_fields(member, once, "a batch member of the context's shape")


@pytest.mark.parametrize("sweeps,opened", [(0, False), (9, False), (0, True)], ids=["inviscid", "sweeps9", "openings"])
def test_a_table_of_zeros_a_cleared_table_and_a_new_mask_give_the_bits_of_the_context_without_one(sfl, sweeps, opened):
    dim_x, dim_y = 130, 70
    forces = forces_of(dim_x, dim_y)
    cells = [c for c, _ in rule.unique(table_of(dim_x, dim_y))]
    moving = list(zip(*table_of(dim_x, dim_y)))

    def run(s):
        for k, records in forces.items():
            queue(s, records, k)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        return download_all(sfl, s)

    with make(sfl, dim_x, dim_y, sweeps, opened, walls=False) as s:
        plain = run(s)
        assert_fields(plain, rule_steps(dim_x, dim_y, sweeps, opened, walls=False), "no table: the rule without one")
        s.set_wall_velocity(cells, np.zeros((len(cells), 2), F))   # anchor (a)
        reload(sfl, s, dim_x, dim_y)
        assert_fields(run(s), plain, "a table of +0.0f")
        s.set_wall_velocity(list(moving[0]), list(moving[1]))
        s.set_wall_velocity(None, None)
        assert s.wall_velocity_info() == 0 and len(s.wall_velocity()[0]) == 0
        reload(sfl, s, dim_x, dim_y)
        assert_fields(run(s), plain, "a cleared table")
        s.set_wall_velocity(list(moving[0]), list(moving[1]))
        s.set_solids(mask_of(dim_x, dim_y))
        assert s.wall_velocity_info() == 0
        reload(sfl, s, dim_x, dim_y)
        assert_fields(run(s), plain, "a new mask drops the table")


def test_refusals_leave_the_table_as_it_was(sfl):
    dim_x, dim_y = 61, 81
    cap = sfl.capi
    with sfl.Solver(dim_x, dim_y) as s:
        with pytest.raises(sfl.SflError, match="no solids set") as e:
            s.set_wall_velocity([(0, 0)], [(1.0, 0.0)])
        assert e.value.code == cap.ERR_STATE
        s.set_wall_velocity(None, None)
        s.set_solids(mask_of(dim_x, dim_y))
        cells, vel = zip(*table_of(dim_x, dim_y))
        s.set_wall_velocity(list(cells), list(vel))
        before = s.wall_velocity()
        for args, words in ((([(0, dim_y - 1), (1, 1)], [(1.0, 0.0)] * 2), "record 1 names cell (1, 1), which is not solid in the mask"),
                            (([(dim_x, 0)], [(1.0, 0.0)]), "record 0 names cell (61, 0), which is not inside the grid of 61 x 81"),
                            (([(0, dim_y - 1)], [(0.0, -np.inf)]), "must be finite (record 0")):
            with pytest.raises(sfl.SflError) as e:
                s.set_wall_velocity(*args)
            assert e.value.code == cap.ERR_INVALID and words in str(e.value), (words, str(e.value))
            after = s.wall_velocity()
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1].view(np.uint32), after[1].view(np.uint32))
