"""The rule of include/sfl.h "INFLOW PROFILES AND FLUX" restated in numpy on top of tests/opening_rule.py: the step with a
per-cell inflow profile (item 2a extended) in float32, and the flux record in exact integers.  What tests/test_inflow.py checks
for its anchors, and what tests/test_inflow_gpu.py and tests/test_context_inflow_gpu.py hold the kernels to, bit for bit.

Layout as in opening_rule: velocity float32[dim_y, dim_x, 2], node (i, j) at [j, i].  A profile is a sequence of records
((i, j), (u, v)) in the order given -- of two records on one cell the later wins.  Not part of the product."""
import math

import numpy as np

import opening_rule as orule

F = np.float32
INFLOW, OUTFLOW = orule.INFLOW, orule.OUTFLOW
# struct sfl_open_flux, 40 bytes
FLUX_DTYPE = np.dtype([("inflow", "<i8"), ("outflow", "<i8"), ("exp2", "<i4"), ("max_abs_n", "<f4"), ("inflow_cells", "<u4"),
                       ("outflow_cells", "<u4"), ("nonfinite", "<u4"), ("reserved", "<u4")])


def check_profile(profile, open):
    """The index of the first record that does not name a cell whose map byte is INFLOW, or None."""
    open = np.asarray(open)
    dim_y, dim_x = open.shape
    for k, ((i, j), _) in enumerate(profile):
        if not (0 <= i < dim_x and 0 <= j < dim_y) or open[j, i] != INFLOW:
            return k
    return None


def unique(profile):
    """The records with duplicates removed -- the later wins -- in cell-index order: ((i, j), (u, v)) tuples."""
    held = {}
    for (i, j), (u, v) in profile:
        held[(int(j), int(i))] = (F(u), F(v))
    return [((i, j), uv) for (j, i), uv in sorted(held.items())]


def impose(u, solid, open, inflow, profile):
    """Item 2a with a profile, in place: every fluid inflow cell holds the uniform inflow, then a fluid inflow cell named by a
    record that record's velocity."""
    fluid_inflow = orule.inflow_cells(open, solid)
    u[fluid_inflow] = np.asarray(inflow, F)
    for (i, j), uv in unique(profile):
        if fluid_inflow[j, i]:
            u[j, i] = uv
    return u


def step(cpu, v, colour, solid, open, inflow, profile, dt, dx=1.0, iters=10, omega=1.96, forces=()):
    """One step by the rule: opening_rule.step with item 2a as above.  Returns (v, div, p, colour)."""
    assert check_profile(profile, open) is None
    solid = orule._solid(solid, np.asarray(open).shape)
    dim_y, dim_x = solid.shape
    u = cpu.advect_vec2f(np.ascontiguousarray(v, F), np.ascontiguousarray(v, F), dt, True)   # item 1
    for i, j, fx, fy in forces:                                                              # item 2
        if 0 <= i < dim_x and 0 <= j < dim_y:
            u[j, i] = (fx, fy)
    impose(u, solid, open, inflow, profile)                                                  # item 2a
    u[solid] = 0.0                                                                           # item 3
    d = orule.divergence(u, solid, open, dx)
    p = orule.solve(d, solid, open, dx, iters, omega)
    u = np.ascontiguousarray(orule.gradient(u, p, solid, open, dx))
    return u, d, p, cpu.advect_vec3uq32(np.ascontiguousarray(colour), u, dt, False)          # item 7


def normals(v, open, solid=None):
    """(n of every live open cell as float32, which of them are outflow cells), in cell-index order."""
    (ow, oe, os_, on), outflow = orule.sides(open, solid)
    live = ow | oe | os_ | on
    vx, vy = np.asarray(v)[..., 0].astype(F), np.asarray(v)[..., 1].astype(F)
    n = np.where(ow, -vx, np.where(oe, vx, np.where(os_, -vy, vy))).astype(F)
    return n[live], outflow[live]


def flux(v, open, solid=None):
    """The flux record of the velocity v through the live open cells: a FLUX_DTYPE scalar, every sum in Python integers."""
    n, out = normals(v, open, solid)
    rec = np.zeros((), FLUX_DTYPE)
    finite = np.isfinite(n)
    rec["inflow_cells"], rec["outflow_cells"], rec["nonfinite"] = int((~out).sum()), int(out.sum()), int((~finite).sum())
    n, out = n[finite], out[finite]
    biggest = F(np.abs(n).max()) if n.size else F(0.0)
    q = math.frexp(float(biggest))[1] - 1 - 32 if biggest != 0 else 0
    terms = [int(math.trunc(math.ldexp(float(x), -q))) for x in n]
    assert all(abs(t) < 2 ** 33 for t in terms)
    rec["inflow"] = -sum(t for t, o in zip(terms, out) if not o)
    rec["outflow"] = sum(t for t, o in zip(terms, out) if o)
    rec["exp2"], rec["max_abs_n"] = q, biggest
    return rec


def flux_xy(rec):
    """(inflow, outflow) * 2^exp2 as float64."""
    return math.ldexp(int(rec["inflow"]), int(rec["exp2"])), math.ldexp(int(rec["outflow"]), int(rec["exp2"]))
