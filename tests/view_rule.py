"""The views of include/sfl.h ("VIEWS") restated in numpy float32: what tests/test_views_gpu.py applies to downloaded fields.

Every product, sum and quotient is one float32 numpy operation, so each is rounded on its own, in the order the header
states.  Fields are laid out as everywhere in the tests: velocity float32[dim_y, dim_x, 2], pressure float32[dim_y, dim_x],
node (i, j) at [j, i].  tests/test_views.py checks this file against the oracle (the divergence bit for bit, the draw chain
through render_rgb565) and against known values; it is not part of the product."""
import numpy as np

SPEED, VORTICITY, PRESSURE, DIVERGENCE = 0, 1, 2, 3
MAX_COLOUR = 0xFC000000
F = np.float32


def two_dx_inv(dx):
    """k = 1.0f / (2.0f * dx), as calculate_divergence forms it."""
    return F(1.0) / (F(2.0) * F(dx))


def _neighbours(a, ghost):
    """West, east, south and north neighbours of every node of a[dim_y, dim_x]; outside the domain: ghost (same shape)."""
    w, e, s, n = ghost.copy(), ghost.copy(), ghost.copy(), ghost.copy()
    w[:, 1:] = a[:, :-1]
    e[:, :-1] = a[:, 1:]
    s[1:, :] = a[:-1, :]
    n[:-1, :] = a[1:, :]
    return w, e, s, n


def divergence(v, dx=1.0):
    """calculate_divergence: interior nodes sum (-W.x + E.x) + (-S.y + N.y); nodes on a wall add the four terms to 0.0f one
    after the other, a missing neighbour's term being the node's own component with the sign of a ghost that is minus it."""
    vx, vy = v[..., 0], v[..., 1]
    dim_y, dim_x = vx.shape
    with np.errstate(all="ignore"):
        wx, ex, _, _ = _neighbours(vx, -vx)    # ghost velocity is negative: -W.x = own.x, E.x = -own.x
        _, _, sy, ny = _neighbours(vy, -vy)
        fast = (-wx + ex) + (-sy + ny)
        safe = np.zeros_like(vx)
        for term in (-wx, ex, -sy, ny):
            safe = safe + term
        j, i = np.mgrid[0:dim_y, 0:dim_x]
        interior = (i > 0) & (i < dim_x - 1) & (j > 0) & (j < dim_y - 1)
        return (np.where(interior, fast, safe) * two_dx_inv(dx)).astype(F)


def vorticity(v, dx=1.0):
    """((E - W) - (N - S)) * k for every node: E, W = vy at (i +- 1, j), N, S = vx at (i, j +- 1); a neighbour outside the
    domain is minus the node's own component."""
    vx, vy = v[..., 0], v[..., 1]
    with np.errstate(all="ignore"):
        w, e, _, _ = _neighbours(vy, -vy)
        _, _, s, n = _neighbours(vx, -vx)
        return (((e - w) - (n - s)) * two_dx_inv(dx)).astype(F)


def speed(v):
    vx, vy = v[..., 0], v[..., 1]
    with np.errstate(all="ignore"):
        return np.sqrt(vx * vx + vy * vy).astype(F)


def scalar(what, v, p, dx=1.0):
    """The scalar field of view `what` of one member: float32[dim_y, dim_x]."""
    if what == SPEED:
        return speed(v)
    if what == VORTICITY:
        return vorticity(v, dx)
    if what == PRESSURE:
        return p.astype(F, copy=True)
    if what == DIVERGENCE:
        return divergence(v, dx)
    raise ValueError(what)


def lerp_floats(s, lo, hi, palette):
    """The float every channel's narrowing is handed, float32[..., 3], and where the texel is nan_colour instead."""
    palette = np.asarray(palette, np.uint32)
    stops = palette.shape[0]
    s = np.asarray(s, F)
    with np.errstate(all="ignore"):
        r = F(1.0) / (F(hi) - F(lo))
        t = (s - F(lo)) * r
        nan = np.isnan(s) | np.isnan(t)
        t = np.where(nan, F(0.0), t)
        t = np.where(t < F(0.0), F(0.0), np.where(t > F(1.0), F(1.0), t)).astype(F)
        x = t * F(stops - 1)
        n = np.minimum(x.astype(np.int32), stops - 2)
        f = x - n.astype(F)
        a, b = palette[n].astype(F), palette[n + 1].astype(F)
        return (a + (b - a) * f[..., None]).astype(F), nan


def narrow(x):
    """uq_narrow: (uint32_t)(x + 0.5f), for x + 0.5f inside [0, 2^32)."""
    return (np.asarray(x, F) + F(0.5)).astype(np.int64).astype(np.uint32)


def texels(s, lo, hi, palette, nan_colour):
    """Scalar -> texel: uint32[..., 3]."""
    val, nan = lerp_floats(s, lo, hi, palette)
    out = narrow(val)
    out[nan] = np.asarray(nan_colour, np.uint32)
    return out


def view_texels(what, v, p, dx, lo, hi, palette, nan_colour):
    return texels(scalar(what, v, p, dx), lo, hi, palette, nan_colour)


def draw_floats(colour, scaling):
    """The draw task's chains (csrc/render_math.h) on a dye colour[dim_y, dim_x, 3]: the float handed to the narrowing of
    every channel of every pixel, float32[scaling * (dim_x - 1), scaling * (dim_y - 1), 3]."""
    t = np.asarray(colour, np.uint32).astype(F).transpose(1, 0, 2)   # [i, j, channel]
    inv = F(1.0) / F(scaling)
    t11, t21, t12, t22 = t[:-1, :-1], t[1:, :-1], t[:-1, 1:], t[1:, 1:]
    nx, ny = t11.shape[:2]
    out = np.empty((nx, scaling, ny, scaling, 3), F)
    left, right = t11.copy(), t12.copy()
    dl, dr = (t21 - t11) * inv, (t22 - t12) * inv
    for ii in range(scaling):
        x, d = left.copy(), (right - left) * inv
        for jj in range(scaling):
            out[:, ii, :, jj] = x
            x = x + d
        left, right = left + dl, right + dr
    return out.reshape(nx * scaling, ny * scaling, 3)


def pack_rgb565(channels, byteswap=True):
    """RGB565 of narrowed channels uint32[..., 3] (csrc/render_math.h render_pack)."""
    c = np.asarray(channels, np.uint32)
    px = (((c[..., 0] & 0xF8000000) >> 16) | ((c[..., 1] & 0xFC000000) >> 21) | ((c[..., 2] & 0xF8000000) >> 27)).astype(np.uint16)
    return px.byteswap() if byteswap else px


def render(colour, scaling, byteswap=True):
    return pack_rgb565(narrow(draw_floats(colour, scaling)), byteswap)
