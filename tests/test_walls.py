"""Wall velocities, the CPU side (include/sfl.h "WALL VELOCITIES"): the six calls as the header declares and the binding sees
them; the rule as tests/wall_rule.py restates it, anchored on tests/solid_rule.py, tests/viscosity_rule.py and
tests/opening_rule.py (a table of +0.0f: the bits of no table) and on what a lid does from rest; rigid_wall_velocity against a
loop; every refusal that needs no device; and the host units (csrc/walls.cpp, csrc/context_walls.cpp, csrc/wall_table.h) run
through by tests/cpp/walls_driver.cpp over a runtime that lives on the host.  tests/test_walls_gpu.py and
tests/test_context_walls_gpu.py have the kernels."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import opening_rule
import solid_rule
import viscosity_rule
import wall_rule as rule
from conftest import ROOT, assert_bit_equal, random_fields

F = np.float32
DT, DX, ITERS, OMEGA = 1 / 30.0, 0.5, 5, 1.9
NAMES = ("velocity", "divergence", "pressure", "colour")
CONTEXT = ("sfl_set_wall_velocity", "sfl_wall_velocity_info", "sfl_wall_velocity_download")
BATCH = ("sfl_batch_set_wall_velocity", "sfl_batch_wall_velocity_info", "sfl_batch_wall_velocity_download")


def lid_and_block(dim_x, dim_y):
    m = np.zeros((dim_y, dim_x), bool)
    m[-1, :] = True
    m[dim_y // 2, dim_x // 2] = True
    return m


# ---- the header and the binding ------------------------------------------------------------------------------------------
def test_the_six_calls_are_declared_exported_and_bound(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, pi, pf, pl = C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    want = {"sfl_set_wall_velocity": [vp, pi, pf, i], "sfl_wall_velocity_info": [vp, pi], "sfl_wall_velocity_download": [vp, pi, pf, i],
            "sfl_batch_set_wall_velocity": [vp, pi, pi, pf, i], "sfl_batch_wall_velocity_info": [vp, pi, pl],
            "sfl_batch_wall_velocity_download": [vp, i, pi, pf, i, pi]}
    assert set(want) == set(CONTEXT + BATCH)
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for line in ("SFL_API int sfl_set_wall_velocity(sfl_context *ctx, const int *cells_ij, const float *vel_xy, int n);",
                 "SFL_API int sfl_wall_velocity_info(sfl_context *ctx, int *records);",
                 "SFL_API int sfl_wall_velocity_download(sfl_context *ctx, int *cells_ij, float *vel_xy, int capacity);",
                 "SFL_API int sfl_batch_set_wall_velocity(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n);",
                 "SFL_API int sfl_batch_wall_velocity_info(sfl_batch *b, int *set, int64_t *records);",
                 "SFL_API int sfl_batch_wall_velocity_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records);"):
        assert line in header, line
    for name in ("set_wall_velocity", "wall_velocity", "wall_velocity_info"):
        assert callable(getattr(sfl.BatchSolver, name, None)) and callable(getattr(sfl.Solver, name, None)), name
    assert callable(sfl.rigid_wall_velocity)
    assert lib.sfl_abi_version() == 1


def test_the_header_states_the_rule_in_its_own_section_behind_the_torque():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    start, end = header.index("/* --- WALL VELOCITIES"), header.index("/* A batch is used from one thread at a time")
    assert header.index("/* --- TORQUE") < header.index("SFL_API int sfl_torque_read(") < start < end
    section = header[start:end]
    for words in ("ITEM 3, EXTENDED", "ITEM 8, NEW, behind item 7", "bits as given", "a -0.0f or a denormal is stored as it stands",
                  "Items 4 to 7 are unchanged", "impermeable wall at rest", "traced back with\n *       (0, 0)", "read a solid neighbour as it is",
                  "NORMAL to a wet face is\n * accepted and acts through those two items only", "from rest and without viscosity a wall moves nothing",
                  "a lid drags the row beside it", "names the first\n *       offending record", "The velocity must be finite", "the later wins",
                  "unique\n *       cells in cell order", "n == 0 clears it", "DROPS the table", "step calls only", "the two tables never meet",
                  "KEEP THEIR DEFINITION", "the wall AT REST", "+0.0f gives the bits of no table", "a context holds what a batch member of\n *       its shape holds",
                  "a shared table counts once per member", "argument checks come first", "no solids set gives SFL_ERR_STATE", "leaves the table as it was"):
        assert words in section, words
    for name in CONTEXT + BATCH:
        assert f"SFL_API int {name}(" in section, name


# ---- the rule's anchors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (61, 81)])
def test_a_table_of_zeros_gives_the_bits_of_the_solids_the_viscous_and_the_openings_step(oracle, dim_x, dim_y):
    v, c, _ = random_fields(dim_x, dim_y, 31, vamp=30.0)
    solid = lid_and_block(dim_x, dim_y)
    zeros = [((int(i), int(j)), (F(0.0), F(0.0))) for j, i in zip(*np.nonzero(solid))]
    forces = [(2, 2, 3.0, -2.0), (dim_x // 2, dim_y - 1, 5.0, 6.0)]   # the second on a wall cell: no effect
    open_map = np.zeros((dim_y, dim_x), np.uint8)
    open_map[1:-1, 0], open_map[1:-1, -1] = opening_rule.INFLOW, opening_rule.OUTFLOW
    inflow = (F(3.5), F(-0.25))
    cases = (("solids", dict(), lambda s: solid_rule.step(oracle, s[0], s[3], solid, DT, DX, ITERS, OMEGA, forces)),
             ("viscous", dict(nu=0.3, sweeps=3), lambda s: viscosity_rule.step(oracle, s[0], s[3], DT, DX, ITERS, OMEGA, 0.3, 3, solid, forces)),
             ("openings", dict(open=open_map, inflow=inflow), lambda s: opening_rule.step(oracle, s[0], s[3], solid, open_map, inflow, DT, DX, ITERS, OMEGA, forces)))
    for what, extra, plain in cases:
        a, b, e = (v, None, None, c), (v, None, None, c), (v, None, None, c)
        for k in range(3):
            a = rule.step(oracle, a[0], a[3], solid, zeros, DT, DX, ITERS, OMEGA, forces, **extra)
            e = rule.step(oracle, e[0], e[3], solid, [], DT, DX, ITERS, OMEGA, forces, **extra)
            b = plain(b)
            for name, x, y, z in zip(NAMES, a, b, e):
                assert_bit_equal(x, y, f"{what}, step {k}: {name}")
                assert_bit_equal(z, y, f"{what}, empty table, step {k}: {name}")
    # ... another table is another flow once item 3a or the next step's advection has read it; of two records the later wins
    moving = [(cell, (F(2.5), F(-0.5))) for cell, _ in zeros]
    one = rule.step(oracle, v, c, solid, moving, DT, DX, ITERS, OMEGA, nu=0.3, sweeps=3)
    assert not np.array_equal(one[0][~solid], viscosity_rule.step(oracle, v, c, DT, DX, ITERS, OMEGA, 0.3, 3, solid)[0][~solid])
    assert np.array_equal(one[0][solid], np.broadcast_to(np.array([2.5, -0.5], F), (int(solid.sum()), 2))), "item 8"
    inviscid = rule.step(oracle, v, c, solid, moving, DT, DX, ITERS, OMEGA)
    for name, x, y in zip(NAMES[1:], inviscid[1:], solid_rule.step(oracle, v, c, solid, DT, DX, ITERS, OMEGA)[1:]):
        assert_bit_equal(x, y, f"without item 3a the first step's {name} does not see the table")
    twice = [(moving[0][0], (F(9.0), F(9.0)))] + moving
    assert_bit_equal(rule.step(oracle, v, c, solid, twice, DT, DX, ITERS, OMEGA, nu=0.3, sweeps=3)[0], one[0], "the later record wins")
    assert rule.unique(twice) == rule.unique(moving) and [cell for cell, _ in rule.unique(twice[::-1])] == [cell for cell, _ in zeros]
    assert rule.check_table([((0, dim_y - 1), (1, 1)), ((1, 1), (1, 1))], solid) == 1 and rule.check_table([((dim_x, 0), (1, 1))], solid) == 0
    assert rule.check_table([((0, dim_y - 1), (np.inf, 1))], solid) == 0


@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (61, 81)])
@pytest.mark.parametrize("u", [2.5, -2.5])
def test_from_rest_a_lid_moves_nothing_without_viscosity_and_drags_the_row_beside_it_with(oracle, dim_x, dim_y, u):
    solid = np.zeros((dim_y, dim_x), bool)
    solid[-1, :] = True
    lid = [((i, dim_y - 1), (F(u), F(0.0))) for i in range(dim_x)]
    c = random_fields(dim_x, dim_y, 5)[1]
    state = (np.zeros((dim_y, dim_x, 2), F), None, None, c)
    for _ in range(3):
        state = rule.step(oracle, state[0], state[3], solid, lid, DT, DX, ITERS, OMEGA)
        assert np.all(state[0][~solid] == 0), "nu = 0: every fluid cell compares equal to zero"
        assert np.all(state[0][solid] == np.array([u, 0.0], F))
    # With nu > 0 item 3a drags the row beside the lid: before the projection every cell of it has the sign of the lid's u.  The
    # step's result has it too where the projection is a correction and not the whole: at 61 x 81.  In a box seven cells wide five
    # over-relaxed iterations leave a pressure whose gradient is as large as the dragged velocity itself (the rule gives
    # +6.7e-4 beside -5.7e-3 there), so that shape checks the drag in front of the projection alone.
    for nu in (0.05, 0.5):
        rest = np.zeros((dim_y, dim_x, 2), F)
        rule.impose(rest, lid)
        dragged = viscosity_rule.diffuse(rest, nu, DT, DX, 3, solid)
        assert np.all(np.sign(dragged[-2, :, 0]) == np.sign(u)) and np.all(dragged[:-2, :, 1] == 0), "item 3a drags the row beside the lid"
        if dim_x >= 61:
            one = rule.step(oracle, np.zeros((dim_y, dim_x, 2), F), c, solid, lid, DT, DX, ITERS, OMEGA, nu=nu, sweeps=3)
            assert np.all(np.sign(one[0][-2, :, 0]) == np.sign(u)), "the row beside the lid has the sign of the lid's u"


# ---- rigid_wall_velocity --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (61, 81)])
def test_rigid_wall_velocity_is_the_loop_of_the_header(sfl, dim_x, dim_y):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    labels = np.zeros((dim_y, dim_x), np.uint8)
    labels[-1, :] = 1
    labels[(i - dim_x // 2) ** 2 + (j - dim_y // 2) ** 2 <= (min(dim_x, dim_y) // 4) ** 2] = 2
    for body, u, v, omega, pivot2 in ((1, 2.5, 0.0, 0.0, (0, 0)), (2, 0.0, 0.0, 0.3, (2 * (dim_x // 2), 2 * (dim_y // 2))),
                                      (2, -1.1, 0.7, -1.7, (dim_x, dim_y + 1)), (3, 1.0, 1.0, 1.0, (0, 0))):
        cells, vel = sfl.rigid_wall_velocity(labels, body, u, v, omega, pivot2)
        want = rule.rigid(labels, body, u, v, omega, pivot2)
        assert cells.dtype == np.int32 and vel.dtype == np.float32 and cells.shape == vel.shape == (len(want), 2)
        assert [tuple(c) for c in cells] == [c for c, _ in want]
        assert np.array_equal(vel.view(np.uint32), np.array([w for _, w in want], F).reshape(-1, 2).view(np.uint32))
    cells, vel = sfl.rigid_wall_velocity(labels, 2, omega=0.5, pivot2=(2 * (dim_x // 2), 2 * (dim_y // 2)))
    centre = [k for k, c in enumerate(cells) if tuple(c) == (dim_x // 2, dim_y // 2)]
    assert len(centre) == 1 and np.all(vel[centre[0]] == 0), "the pivot's own cell is at rest"
    with pytest.raises(ValueError, match="labels of shape"):
        sfl.rigid_wall_velocity(labels.astype(np.float32), 1)


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    cells, good = (C.c_int * 4)(0, 1, 0, 2), (C.c_float * 4)(1.0, 0.0, 2.0, 0.0)
    nan, inf = (C.c_float * 4)(1.0, 0.0, 2.0, float("nan")), (C.c_float * 4)(float("-inf"), 0.0, 2.0, 0.0)
    n, w = C.c_int(5), C.c_int64(5)
    refusals = [
        (lambda: lib.sfl_set_wall_velocity(None, cells, good, -1), "sfl_set_wall_velocity: n must be >= 0 (got -1)"),
        (lambda: lib.sfl_set_wall_velocity(None, None, good, 2), "sfl_set_wall_velocity: cells_ij is NULL with n = 2"),
        (lambda: lib.sfl_set_wall_velocity(None, cells, None, 2), "sfl_set_wall_velocity: vel_xy is NULL with n = 2"),
        (lambda: lib.sfl_set_wall_velocity(None, cells, nan, 2), "sfl_set_wall_velocity: the velocity of a record must be finite (record 1: (2, nan))"),
        (lambda: lib.sfl_set_wall_velocity(None, cells, inf, 2), "sfl_set_wall_velocity: the velocity of a record must be finite (record 0: (-inf, 0))"),
        (lambda: lib.sfl_set_wall_velocity(None, cells, good, 2), "sfl_set_wall_velocity: ctx is NULL"),
        (lambda: lib.sfl_set_wall_velocity(None, None, None, 0), "sfl_set_wall_velocity: ctx is NULL"),
        (lambda: lib.sfl_wall_velocity_info(None, C.byref(n)), "sfl_wall_velocity_info: ctx is NULL"),
        (lambda: lib.sfl_wall_velocity_download(None, cells, good, 2), "sfl_wall_velocity_download: ctx is NULL"),
        (lambda: lib.sfl_batch_set_wall_velocity(None, None, cells, good, -3), "sfl_batch_set_wall_velocity: n must be >= 0 (got -3)"),
        (lambda: lib.sfl_batch_set_wall_velocity(None, None, None, good, 1), "sfl_batch_set_wall_velocity: cells_ij is NULL with n = 1"),
        (lambda: lib.sfl_batch_set_wall_velocity(None, None, cells, None, 1), "sfl_batch_set_wall_velocity: vel_xy is NULL with n = 1"),
        (lambda: lib.sfl_batch_set_wall_velocity(None, None, cells, nan, 2), "sfl_batch_set_wall_velocity: the velocity of a record must be finite (record 1: (2, nan))"),
        (lambda: lib.sfl_batch_set_wall_velocity(None, None, cells, good, 2), "sfl_batch_set_wall_velocity: batch is NULL"),
        (lambda: lib.sfl_batch_wall_velocity_info(None, C.byref(n), C.byref(w)), "sfl_batch_wall_velocity_info: batch is NULL"),
        (lambda: lib.sfl_batch_wall_velocity_download(None, 0, cells, good, 2, C.byref(n)), "sfl_batch_wall_velocity_download: batch is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert n.value == 5 and w.value == 5


def test_the_python_front_end_checks_the_shapes_before_the_library_sees_the_records(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2

        def __del__(self):
            pass

    class FakeContext(sfl.Solver):
        def __init__(self):
            self._h, self._lib = None, None
            self.dim_x, self.dim_y = 4, 3

        def __del__(self):
            pass

    for fake in (Fake(), FakeContext()):
        with pytest.raises(ValueError, match="wall velocity: cells of shape"):
            fake.set_wall_velocity([0, 1], [[1.0, 0.0]])
        with pytest.raises(ValueError, match="wall velocity: cells of shape"):
            fake.set_wall_velocity([[0.5, 1.0]], [[1.0, 0.0]])
        with pytest.raises(ValueError, match="wall velocity: vel of shape"):
            fake.set_wall_velocity([[0, 1]], [[1.0, 0.0], [2.0, 0.0]])
    with pytest.raises(ValueError, match="wall velocity: members of shape"):
        Fake().set_wall_velocity([[0, 1]], [[1.0, 0.0]], members=[0, 1])


# ---- the host units ------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver(target):
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "walls.mk", "-j4"] + ([target] if target else []), check=True, stdout=subprocess.DEVNULL)
    return os.path.join(cpp, "walls_driver_san" if target else "walls_driver")


@pytest.mark.parametrize("target", ["", "san"], ids=["plain", "asan-ubsan"])
def test_the_host_side_of_the_wall_tables(target):
    """`make -C tests/cpp -f walls.mk [san]`: tests/cpp/walls_driver.cpp, a stand-alone program, built plain and -- the same
    program -- under -fsanitize=address,undefined.  Its head comment lists what it checks."""
    r = subprocess.run([driver(target)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


# ---- the wall's share of the friction and of the friction torque ---------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (61, 81)])
def test_the_walls_shares_are_a_walk_over_the_wet_faces(sfl, dim_x, dim_y):
    import friction_rule
    import torque_rule
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    labels = np.zeros((dim_y, dim_x), np.uint8)
    labels[-1, :] = 1
    labels[(i - dim_x // 2) ** 2 + (j - dim_y // 2) ** 2 <= (min(dim_x, dim_y) // 4) ** 2] = 2
    labels[0, 0] = 3          # labelled but fluid: counts for nothing
    solid = labels > 0
    solid[0, 0] = False
    solid[1, dim_x - 1] = True   # solid in no body: no face of any
    pivot2 = np.array([[0, 0], [2 * (dim_x // 2), 2 * (dim_y // 2)], [3, -5]])
    lid = sfl.rigid_wall_velocity(labels, 1, 2.5, 0.5)
    disc = sfl.rigid_wall_velocity(labels, 2, 0.25, -0.75, 0.3, pivot2[1])
    cells, vel = np.concatenate([lid[0], disc[0]]), np.concatenate([lid[1], disc[1]])
    friction, torque = sfl.wall_shares(solid, labels, 3, pivot2, cells, vel)
    assert friction.shape == (3, 2) and torque.shape == (3,) and friction.dtype == torque.dtype == np.float64
    wall = {(int(a), int(b)): (float(u), float(v)) for (a, b), (u, v) in zip(cells, vel)}
    want_f, want_t = np.zeros((3, 2)), np.zeros(3)
    for jj in range(dim_y):           # the brute-force walk: every solid cell of a body, its four neighbours
        for ii in range(dim_x):
            b = int(labels[jj, ii])
            if not solid[jj, ii] or b == 0:
                continue
            u, v = wall.get((ii, jj), (0.0, 0.0))
            rx, ry = ii - pivot2[b - 1, 0] / 2.0, jj - pivot2[b - 1, 1] / 2.0
            for di, dj in ((-1, 0), (1, 0), (0, -1), (0, 1)):
                if not (0 <= ii + di < dim_x and 0 <= jj + dj < dim_y) or solid[jj + dj, ii + di]:
                    continue
                if di:
                    want_f[b - 1, 1] += v
                    want_t[b - 1] += rx * v
                else:
                    want_f[b - 1, 0] += u
                    want_t[b - 1] -= ry * u
    # (float32 values of like size, arms of a few bits: every float64 product and sum is exact, whatever the order)
    assert np.array_equal(friction, want_f) and np.array_equal(torque, want_t)
    assert np.all(friction[2] == 0) and torque[2] == 0 and friction[0, 0] != 0 and torque[1] != 0
    # ... and the anchor on the records' own rules: a fluid that moves with a uniformly translating wall has the wall's share
    uniform = np.zeros((dim_y, dim_x, 2), F)
    uniform[...] = (1.5, -0.25)
    moving = (np.argwhere(solid & (labels > 0))[:, ::-1], np.broadcast_to(np.array([1.5, -0.25], F), (int((solid & (labels > 0)).sum()), 2)))
    friction, torque = sfl.wall_shares(solid, labels, 3, pivot2, *moving)
    assert np.array_equal(friction, friction_rule.friction_xy(friction_rule.friction(uniform, solid, labels, 3), 1.0))
    rec = torque_rule.torque(np.zeros((dim_y, dim_x), F), uniform, solid, labels, 3, pivot2)
    assert np.array_equal(torque, torque_rule.torque_xy(rec, 1.0, 1.0, 1.0)[..., 1])
