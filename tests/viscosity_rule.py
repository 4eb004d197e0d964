"""The viscosity's rule of include/sfl.h ("VISCOSITY", item 3a of a step) restated in numpy float32: what
tests/test_viscosity.py holds the tile core of csrc/diffuse_tile.h to on the host, and tests/test_viscosity_gpu.py the kernels
of csrc/batch_viscous.hip and csrc/context_viscous.hip, bit for bit.

Every product, sum and quotient is one float32 numpy operation, so each is rounded on its own, in the order the header
states.  Fields are laid out as everywhere in the tests: velocity float32[dim_y, dim_x, 2], node (i, j) at [j, i]; `solid`
is bool[dim_y, dim_x] or None.  The advections and the solids' items come from tests/solid_rule.py and the `cpu` argument.
Not part of the product."""
import numpy as np

import solid_rule

F = np.float32


def coefficients(nu, dt, dx):
    """a = (nu * dt) / (dx * dx) and c = 1.0f / (1.0f + 4.0f * a), every operation rounded on its own."""
    nu_dt = F(nu) * F(dt)
    dx2 = F(dx) * F(dx)
    a = F(nu_dt / dx2)
    four_a = F(4.0) * a
    return a, F(F(1.0) / F(F(1.0) + four_a))


def _neighbours(u):
    """The west, east, south and north neighbour of every node of u[dim_y, dim_x]; outside the domain the node's own
    value negated, as it stands: the no-slip ghost."""
    w, e, s, n = (np.negative(u) for _ in range(4))
    w[:, 1:] = u[:, :-1]
    e[:, :-1] = u[:, 1:]
    s[1:, :] = u[:-1, :]
    n[:-1, :] = u[1:, :]
    return w, e, s, n


def sweep_colour(u, u0, a, c, colour, solid):
    """One half-sweep: every fluid cell of the colour takes (u0 + a * (((W + E) + S) + N)) * c; the others keep theirs."""
    dim_y, dim_x = u.shape[:2]
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    take = ((i + j) & 1) == colour
    if solid is not None:
        take &= ~np.asarray(solid, bool)
    out = u.copy()
    with np.errstate(all="ignore"):
        for q in (0, 1):
            w, e, s, n = _neighbours(u[..., q])
            total = np.add(np.add(np.add(w, e, dtype=F), s, dtype=F), n, dtype=F)
            fresh = np.multiply(np.add(u0[..., q], np.multiply(a, total, dtype=F), dtype=F), c, dtype=F)
            out[..., q] = np.where(take, fresh, u[..., q])
    return out


def diffuse(v, nu, dt, dx, sweeps, solid=None):
    """Item 3a on the velocity v: `sweeps` times colour 0, then colour 1.  nu == 0 or sweeps == 0: v itself, untouched."""
    if F(nu) == F(0.0) or sweeps == 0:
        return v
    a, c = coefficients(nu, dt, dx)
    u0 = np.ascontiguousarray(v, F)
    u = u0.copy()
    for _ in range(sweeps):
        for colour in (0, 1):
            u = sweep_colour(u, u0, a, c, colour, solid)
    return u


def step(cpu, v, colour, dt, dx=1.0, iters=10, omega=1.96, nu=0.0, sweeps=0, solid=None, forces=()):
    """One step with item 3a.  solid None: the plain step's operators around it (cpu.divergence, cpu.poisson_solve,
    cpu.subtract_gradient); else the solids' rule (tests/solid_rule.py).  Returns (v, div, p, colour) as cpu.step does."""
    dim_y, dim_x = v.shape[:2]
    u = cpu.advect_vec2f(np.ascontiguousarray(v, F), np.ascontiguousarray(v, F), dt, True)   # item 1
    for i, j, fx, fy in forces:                                                              # item 2
        if 0 <= i < dim_x and 0 <= j < dim_y:
            u[j, i] = (fx, fy)
    if solid is not None:
        u[np.asarray(solid, bool)] = 0.0                                                     # item 3
    u = np.ascontiguousarray(diffuse(u, nu, dt, dx, sweeps, solid))                          # item 3a
    if solid is None:
        d = cpu.divergence(u, dx)
        p = cpu.poisson_solve(d, dx, iters, omega)
        u = np.ascontiguousarray(cpu.subtract_gradient(u, p, dx))
    else:
        d = solid_rule.divergence(u, solid, dx)
        p = solid_rule.solve(d, solid, dx, iters, omega)
        u = np.ascontiguousarray(solid_rule.gradient(u, p, solid, dx))
    return u, d, p, cpu.advect_vec3uq32(np.ascontiguousarray(colour), u, dt, False)          # item 7
