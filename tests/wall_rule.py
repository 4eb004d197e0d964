"""The walls' rule of include/sfl.h ("WALL VELOCITIES") restated in numpy float32 on top of tests/solid_rule.py,
tests/viscosity_rule.py, tests/opening_rule.py and tests/inflow_rule.py: the existing step with two statements added.  What
tests/test_walls.py checks for its anchors, and what tests/test_walls_gpu.py and tests/test_context_walls_gpu.py hold the
kernels of csrc/batch_walls.hip and csrc/context_walls.hip to, bit for bit.

Layout as in solid_rule: velocity float32[dim_y, dim_x, 2], node (i, j) at [j, i]; `solid` bool[dim_y, dim_x].  A wall table
is a list of ((i, j), (u, v)) records in the order given.  Not part of the product."""
import numpy as np

import inflow_rule
import opening_rule
import solid_rule
import viscosity_rule

F = np.float32


def check_table(walls, solid):
    """The index of the first record that may not be staged, or None: a cell outside the grid, a fluid cell, a velocity
    that is not finite."""
    solid = np.asarray(solid, bool)
    dim_y, dim_x = solid.shape
    for k, ((i, j), (u, v)) in enumerate(walls):
        if not (0 <= i < dim_x and 0 <= j < dim_y) or not solid[j, i] or not (np.isfinite(F(u)) and np.isfinite(F(v))):
            return k
    return None


def unique(walls):
    """The records in cell order (dim_x * j + i ascending), of two on one cell the later kept."""
    last = {}
    for (i, j), u in walls:
        last[(int(j), int(i))] = u
    return [((i, j), last[(j, i)]) for j, i in sorted(last)]


def impose(u, walls):
    """The records into the velocity, bits as given, later ones over earlier ones."""
    for (i, j), w in walls:
        u[j, i] = np.asarray(w, F)


def step(cpu, v, colour, solid, walls, dt, dx=1.0, iters=10, omega=1.96, forces=(), nu=0.0, sweeps=0, open=None, inflow=(0.0, 0.0), profile=()):
    """One step by the rule with the wall table `walls`.  open None: the solids' step with item 3a (nu, sweeps); else the
    openings' step with the uniform `inflow` and the records of `profile` (no viscosity there: the library refuses it).
    Returns (v, div, p, colour) as cpu.step does."""
    solid = np.asarray(solid, bool)
    assert check_table(walls, solid) is None
    assert open is None or (F(nu) == F(0.0) or sweeps == 0)
    dim_y, dim_x = solid.shape
    u = cpu.advect_vec2f(np.ascontiguousarray(v, F), np.ascontiguousarray(v, F), dt, True)   # item 1
    for i, j, fx, fy in forces:                                                              # item 2
        if 0 <= i < dim_x and 0 <= j < dim_y:
            u[j, i] = (fx, fy)
    if open is not None:
        inflow_rule.impose(u, solid, open, inflow, profile)                                  # item 2a
    u[solid] = 0.0                                                                           # item 3 ...
    impose(u, walls)                                                                         # ... extended
    if open is None:
        u = np.ascontiguousarray(viscosity_rule.diffuse(u, nu, dt, dx, sweeps, solid))       # item 3a
        d = solid_rule.divergence(u, solid, dx)                                              # items 4 - 6: a wall at rest
        p = solid_rule.solve(d, solid, dx, iters, omega)
        u = np.ascontiguousarray(solid_rule.gradient(u, p, solid, dx))
    else:
        d = opening_rule.divergence(u, solid, open, dx)
        p = opening_rule.solve(d, solid, open, dx, iters, omega)
        u = np.ascontiguousarray(opening_rule.gradient(u, p, solid, open, dx))
    colour = cpu.advect_vec3uq32(np.ascontiguousarray(colour), u, dt, False)                 # item 7: a solid cell's u is (0, 0)
    impose(u, walls)                                                                         # item 8
    return u, d, p, colour


def rigid(labels, body, u, v, omega, pivot2):
    """rigid_wall_velocity by a loop: [((i, j), (wu, wv))] in cell order, every operation one float32 rounding."""
    labels = np.asarray(labels)
    out = []
    for j in range(labels.shape[0]):
        for i in range(labels.shape[1]):
            if labels[j, i] != body:
                continue
            rx = F(0.5) * F(2 * i - pivot2[0])
            ry = F(0.5) * F(2 * j - pivot2[1])
            out.append(((i, j), (F(F(u) - F(F(omega) * ry)), F(F(v) + F(F(omega) * rx)))))
    return out
