"""The solids' rule of include/sfl.h ("SOLIDS") restated in numpy float32: what tests/test_solids.py checks against the
reference and the oracle, and what tests/test_solids_gpu.py holds the kernels of csrc/batch_solids.hip to, bit for bit.

Every product, sum and difference is one float32 numpy operation, so each is rounded on its own, in the order the header
states.  Fields are laid out as everywhere in the tests: velocity float32[dim_y, dim_x, 2], scalars float32[dim_y, dim_x],
node (i, j) at [j, i]; `solid` is bool[dim_y, dim_x].  The two advections are not restated: they are unchanged by the rule
and come from the `cpu` argument, the `oracle` or the `reference` fixture.  Not part of the product."""
import numpy as np

F = np.float32
W, E, S, N, FLUID = 1, 2, 4, 8, 16
NEG0 = F(-0.0)


def two_dx_inv(dx):
    """k = 1.0f / (2.0f * dx), as calculate_divergence forms it."""
    return F(1.0) / (F(2.0) * F(dx))


def _shifted(a, fill):
    """The west, east, south and north neighbours of every node of a[dim_y, dim_x]; `fill` outside the domain."""
    w, e, s, n = (np.full_like(a, fill) for _ in range(4))
    w[:, 1:] = a[:, :-1]
    e[:, :-1] = a[:, 1:]
    s[1:, :] = a[:-1, :]
    n[:-1, :] = a[1:, :]
    return w, e, s, n


def present(solid):
    """Which neighbours of every cell are present -- inside the domain and fluid: four bool arrays, W, E, S, N."""
    solid = np.asarray(solid, bool)
    return _shifted(~solid, False)


def codes(solid):
    """The code byte of every cell: bit 0 W, 1 E, 2 S, 3 N neighbour present, bit 4 the cell is fluid; a solid cell's is 0."""
    solid = np.asarray(solid, bool)
    w, e, s, n = present(solid)
    c = w * W + e * E + s * S + n * N + FLUID
    return np.where(solid, 0, c).astype(np.uint8)


def count_present(solid):
    """`present` of every FLUID cell (0..4); -1 in a solid one."""
    w, e, s, n = present(solid)
    return np.where(np.asarray(solid, bool), -1, w.astype(int) + e + s + n)


def divergence(v, solid, dx=1.0):
    """Item 4: all four neighbours present (-W.x + E.x) + (-S.y + N.y), else 0.0f + the four terms in the order W, E, S, N,
    an absent neighbour's term the cell's own component with the ghost's sign; times k; 0.0f in a solid cell."""
    solid = np.asarray(solid, bool)
    vx, vy = v[..., 0].astype(F), v[..., 1].astype(F)
    pw, pe, ps, pn = present(solid)
    with np.errstate(all="ignore"):
        wx, ex, _, _ = _shifted(vx, F(0))
        _, _, sy, ny = _shifted(vy, F(0))
        tw, te = np.where(pw, -wx, vx), np.where(pe, ex, -vx)
        ts, tn = np.where(ps, -sy, vy), np.where(pn, ny, -vy)
        fast = (tw + te) + (ts + tn)
        safe = np.zeros_like(vx)
        for term in (tw, te, ts, tn):
            safe = safe + term
        d = np.where(pw & pe & ps & pn, fast, safe) * two_dx_inv(dx)
    return np.where(solid, F(0.0), d).astype(F)


def _k_and_z(solid):
    n = count_present(solid)
    kf = np.select([n == 4, n == 3, n == 2, n == 1], [F(-0.25), F(-1.0 / 3.0), F(-0.5), F(-1.0)], F(0.0)).astype(F)
    z = np.where(n == 4, NEG0, F(0.0)).astype(F)
    return kf, z


def _p_gs(p, rhs, solid, kf, z):
    """k * (dx * d - ((((z + W) + E) + S) + N)) for every cell from the pressure as it stands, -0.0f for an absent neighbour."""
    pw, pe, ps, pn = present(solid)
    w, e, s, n = _shifted(p, F(0))
    with np.errstate(all="ignore"):
        total = (((z + np.where(pw, w, NEG0)) + np.where(pe, e, NEG0)) + np.where(ps, s, NEG0)) + np.where(pn, n, NEG0)
        return (kf * (rhs - total)).astype(F)


def solve(d, solid, dx=1.0, iters=10, omega=1.96):
    """Item 5: p = 0, then `iters` times the even cells, then the odd ones; solid cells are never updated."""
    return iterate(np.zeros(np.asarray(solid).shape, F), d, solid, dx, iters, omega)


def iterate(p, d, solid, dx=1.0, iters=10, omega=1.96):
    """Item 5's iterations on the pressure `p` as it stands: `iters` times the even cells, then the odd ones; a solid cell
    keeps what it holds and is never read."""
    solid = np.asarray(solid, bool)
    dim_y, dim_x = solid.shape
    kf, z = _k_and_z(solid)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    om, one_minus = F(omega), F(1.0) - F(omega)
    p = np.array(p, F)
    with np.errstate(all="ignore"):
        rhs = (F(dx) * d.astype(F)).astype(F)
        for _ in range(iters):
            for colour in (0, 1):
                fresh = one_minus * p + om * _p_gs(p, rhs, solid, kf, z)
                p = np.where((((i + j) & 1) == colour) & ~solid, fresh, p).astype(F)
    return p


def update_norm(p, d, solid, dx=1.0):
    """max over FLUID cells of |p_gs - p| on the pressure as it stands, over bit patterns (any NaN wins); 0.0f without one."""
    solid = np.asarray(solid, bool)
    kf, z = _k_and_z(solid)
    with np.errstate(all="ignore"):
        rhs = (F(dx) * d.astype(F)).astype(F)
        diff = (_p_gs(p.astype(F), rhs, solid, kf, z) - p.astype(F)).astype(F)
    bits = np.ascontiguousarray(diff).view(np.uint32) & np.uint32(0x7FFFFFFF)
    bits = bits[~solid]
    worst = np.uint32(bits.max()) if bits.size else np.uint32(0)
    return np.array([worst], np.uint32).view(F)[0]


def gradient(v, p, solid, dx=1.0):
    """Item 6: v - grad p with an absent neighbour's pressure the cell's own; (0, 0) in a solid cell."""
    solid = np.asarray(solid, bool)
    pw, pe, ps, pn = present(solid)
    p = p.astype(F)
    w, e, s, n = _shifted(p, F(0))
    k = two_dx_inv(dx)
    out = np.zeros_like(v, dtype=F)
    with np.errstate(all="ignore"):
        gx = (np.where(pe, e, p) - np.where(pw, w, p)) * k
        gy = (np.where(pn, n, p) - np.where(ps, s, p)) * k
        out[..., 0] = v[..., 0] - gx
        out[..., 1] = v[..., 1] - gy
    out[solid] = 0.0
    return out


def step(cpu, v, colour, solid, dt, dx=1.0, iters=10, omega=1.96, forces=()):
    """One step by the rule.  `forces`: (i, j, vx, vy) records in queue order.  Returns (v, div, p, colour) as cpu.step does."""
    solid = np.asarray(solid, bool)
    dim_y, dim_x = solid.shape
    u = cpu.advect_vec2f(np.ascontiguousarray(v, F), np.ascontiguousarray(v, F), dt, True)   # item 1
    for i, j, fx, fy in forces:                                                              # item 2
        if 0 <= i < dim_x and 0 <= j < dim_y:
            u[j, i] = (fx, fy)
    u[solid] = 0.0                                                                           # item 3
    d = divergence(u, solid, dx)
    p = solve(d, solid, dx, iters, omega)
    u = np.ascontiguousarray(gradient(u, p, solid, dx))
    return u, d, p, cpu.advect_vec3uq32(np.ascontiguousarray(colour), u, dt, False)          # item 7
