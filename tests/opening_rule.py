"""The openings' rule of include/sfl.h ("OPENINGS") restated in numpy float32 on top of tests/solid_rule.py: what
tests/test_openings.py checks for its anchors and its fixed points, and what tests/test_openings_gpu.py holds the kernels of
csrc/batch_openings.hip to, bit for bit.

Every product, sum and difference is one float32 numpy operation, in the order the header states.  Layout as in solid_rule:
velocity float32[dim_y, dim_x, 2], scalars float32[dim_y, dim_x], node (i, j) at [j, i]; `solid` bool[dim_y, dim_x] (None: no
solid cell); `open` uint8[dim_y, dim_x] of 0, INFLOW, OUTFLOW.  Not part of the product."""
import numpy as np

import solid_rule as sr

F = np.float32
NEG0 = F(-0.0)
INFLOW, OUTFLOW = 1, 2


def check_map(open):
    """The first cell that may not hold what it holds, as (i, j), or None: a byte above 2, a nonzero byte on a corner or inside."""
    open = np.asarray(open)
    dim_y, dim_x = open.shape
    for j, i in zip(*np.nonzero(open)):
        outside = int(i == 0) + int(i == dim_x - 1) + int(j == 0) + int(j == dim_y - 1)
        if open[j, i] > OUTFLOW or outside != 1:
            return int(i), int(j)
    return None


def _solid(solid, shape):
    return np.zeros(shape, bool) if solid is None else np.asarray(solid, bool)


def sides(open, solid=None):
    """Which neighbour of every cell is OPEN -- four bool arrays W, E, S, N -- and which cells are live outflow cells: an
    opening counts only where the cell is fluid."""
    open = np.asarray(open, np.uint8)
    assert check_map(open) is None
    dim_y, dim_x = open.shape
    live = (open != 0) & ~_solid(solid, open.shape)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return (live & (i == 0), live & (i == dim_x - 1), live & (j == 0), live & (j == dim_y - 1)), live & (open == OUTFLOW)


def inflow_cells(open, solid=None):
    """The fluid inflow cells (item 2a)."""
    open = np.asarray(open, np.uint8)
    return (open == INFLOW) & ~_solid(solid, open.shape)


def divergence(v, solid, open, dx=1.0):
    """Item 4: a cell with an open neighbour takes the safe form; the open neighbour's term is the cell's own component with
    the sign opposite to a wall's.  Every other cell: solid_rule's."""
    solid = _solid(solid, np.asarray(open).shape)
    (ow, oe, os_, on), _ = sides(open, solid)
    any_open = ow | oe | os_ | on
    vx, vy = v[..., 0].astype(F), v[..., 1].astype(F)
    pw, pe, ps, pn = sr.present(solid)
    with np.errstate(all="ignore"):
        wx, ex, _, _ = sr._shifted(vx, F(0))
        _, _, sy, ny = sr._shifted(vy, F(0))
        tw = np.where(pw, -wx, np.where(ow, -vx, vx))
        te = np.where(pe, ex, np.where(oe, vx, -vx))
        ts = np.where(ps, -sy, np.where(os_, -vy, vy))
        tn = np.where(pn, ny, np.where(on, vy, -vy))
        safe = np.zeros_like(vx)
        for term in (tw, te, ts, tn):
            safe = safe + term
        d = (safe * sr.two_dx_inv(dx)).astype(F)
    return np.where(any_open, d, sr.divergence(v, solid, dx)).astype(F)


def _k_and_z(solid, open):
    """n = present + 1 for an outflow cell, k from n by the solids' table; z = -0.0f iff all four neighbours are present."""
    _, outflow = sides(open, solid)
    present = sr.count_present(solid)
    n = present + outflow
    kf = np.select([n == 4, n == 3, n == 2, n == 1], [F(-0.25), F(-1.0 / 3.0), F(-0.5), F(-1.0)], F(0.0)).astype(F)
    z = np.where(present == 4, NEG0, F(0.0)).astype(F)
    return kf, z


def iterate(p, d, solid, open, dx=1.0, iters=10, omega=1.96):
    """Item 5's iterations on the pressure as it stands: solid_rule.iterate with the k above (the open neighbour is absent:
    it contributes -0.0f to the sum)."""
    solid = _solid(solid, np.asarray(open).shape)
    dim_y, dim_x = solid.shape
    kf, z = _k_and_z(solid, open)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    om, one_minus = F(omega), F(1.0) - F(omega)
    p = np.array(p, F)
    with np.errstate(all="ignore"):
        rhs = (F(dx) * d.astype(F)).astype(F)
        for _ in range(iters):
            for colour in (0, 1):
                fresh = one_minus * p + om * sr._p_gs(p, rhs, solid, kf, z)
                p = np.where((((i + j) & 1) == colour) & ~solid, fresh, p).astype(F)
    return p


def solve(d, solid, open, dx=1.0, iters=10, omega=1.96):
    return iterate(np.zeros(np.asarray(open).shape, F), d, solid, open, dx, iters, omega)


def update_norm(p, d, solid, open, dx=1.0):
    """solid_rule.update_norm with the k of item 5."""
    solid = _solid(solid, np.asarray(open).shape)
    kf, z = _k_and_z(solid, open)
    with np.errstate(all="ignore"):
        rhs = (F(dx) * d.astype(F)).astype(F)
        diff = (sr._p_gs(p.astype(F), rhs, solid, kf, z) - p.astype(F)).astype(F)
    bits = np.ascontiguousarray(diff).view(np.uint32) & np.uint32(0x7FFFFFFF)
    bits = bits[~solid]
    worst = np.uint32(bits.max()) if bits.size else np.uint32(0)
    return np.array([worst], np.uint32).view(F)[0]


def gradient(v, p, solid, open, dx=1.0):
    """Item 6: an outflow neighbour's pressure is +0.0f, an inflow neighbour's the cell's own, as an absent one's."""
    solid = _solid(solid, np.asarray(open).shape)
    (ow, oe, os_, on), outflow = sides(open, solid)
    pw, pe, ps, pn = sr.present(solid)
    p = p.astype(F)
    w, e, s, n = sr._shifted(p, F(0))
    zero = np.zeros_like(p)
    k = sr.two_dx_inv(dx)
    out = np.zeros_like(v, dtype=F)
    with np.errstate(all="ignore"):
        gw = np.where(pw, w, np.where(ow & outflow, zero, p))
        ge = np.where(pe, e, np.where(oe & outflow, zero, p))
        gs = np.where(ps, s, np.where(os_ & outflow, zero, p))
        gn = np.where(pn, n, np.where(on & outflow, zero, p))
        out[..., 0] = v[..., 0] - (ge - gw) * k
        out[..., 1] = v[..., 1] - (gn - gs) * k
    out[solid] = 0.0
    return out


def step(cpu, v, colour, solid, open, inflow, dt, dx=1.0, iters=10, omega=1.96, forces=()):
    """One step by the rule.  `forces`: (i, j, vx, vy) records in queue order; `inflow`: (u, v).  Returns (v, div, p, colour)."""
    solid = _solid(solid, np.asarray(open).shape)
    dim_y, dim_x = solid.shape
    u = cpu.advect_vec2f(np.ascontiguousarray(v, F), np.ascontiguousarray(v, F), dt, True)   # item 1
    for i, j, fx, fy in forces:                                                              # item 2
        if 0 <= i < dim_x and 0 <= j < dim_y:
            u[j, i] = (fx, fy)
    u[inflow_cells(open, solid)] = np.asarray(inflow, F)                                     # item 2a
    u[solid] = 0.0                                                                           # item 3
    d = divergence(u, solid, open, dx)
    p = solve(d, solid, open, dx, iters, omega)
    u = np.ascontiguousarray(gradient(u, p, solid, open, dx))
    return u, d, p, cpu.advect_vec3uq32(np.ascontiguousarray(colour), u, dt, False)          # item 7


def flux(v, open, solid=None):
    """(into the domain through the live inflow cells, out of it through the live outflow cells): the sums of the outward or
    inward normal velocity component, in float64.  A diagnostic of the tests; the library has none."""
    (ow, oe, os_, on), outflow = sides(open, solid)
    vx, vy = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
    outward = np.where(ow, -vx, 0) + np.where(oe, vx, 0) + np.where(os_, -vy, 0) + np.where(on, vy, 0)
    live = ow | oe | os_ | on
    return float(-outward[live & ~outflow].sum()), float(outward[outflow].sum())
