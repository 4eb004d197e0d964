"""The tracers' definition in numpy (include/sfl.h "TRACERS"), for the tests: sample() of sfl/advect.h (advect.h:24-72) at
arbitrary positions and the advance rule, operation for operation in float32 -- every product and sum rounded on its own,
the dye narrowed to UQ32 exactly where the header narrows.  tests/test_tracers.py pins it to the bits of the golden
fixtures, which the reference's own advect.h left; tests/test_tracers_gpu.py then applies it to downloaded fields."""
import numpy as np

F = np.float32


def _lerp(t, a, b):
    """a * (1 - t) + b * t: two rounded products, one rounded sum (advect.h:13-16)."""
    return a * (F(1) - t) + b * t


def _narrow(a):
    """UQ32(float): + 0.5f, truncate (uq32.h:13)."""
    return (a + F(0.5)).astype(np.int64).astype(np.uint32)


def sample(field, x, y, no_slip):
    """sample<T>(field, x, y, dim_x, dim_y, no_slip) at every position: field float32[dim_y, dim_x] or [dim_y, dim_x, 2],
    or the dye uint32[dim_y, dim_x, 3]; x, y float32[n].  A position with a NaN coordinate reads NaN (the dye: 0)."""
    field, x, y = np.asarray(field), np.asarray(x, F), np.asarray(y, F)
    dye = field.dtype == np.uint32
    scalar = field.ndim == 2
    p = (field[..., None] if scalar else field).astype(F)   # (widening a UQ32 rounds to nearest even, uq32.h:15)
    dim_y, dim_x = p.shape[:2]
    skip = np.isnan(x) | np.isnan(y)
    x, y = np.where(skip, F(0), x), np.where(skip, F(0), y)
    lx, ly = F(dim_x - 1), F(dim_y - 1)
    with np.errstate(invalid="ignore", over="ignore"):
        x_under, y_under = x < 0, y < 0
        x_out, y_out = x_under | (x >= lx), y_under | (y >= ly)
        fi, fj = np.floor(x), np.floor(y)
        di, dj = (x - fi)[:, None], (y - fj)[:, None]
        ci = np.where(x_out, np.where(x_under, 0, dim_x - 1), np.where(x_out, F(0), fi).astype(np.int64))
        cj = np.where(y_out, np.where(y_under, 0, dim_y - 1), np.where(y_out, F(0), fj).astype(np.int64))
        ci1, cj1 = np.minimum(ci + 1, dim_x - 1), np.minimum(cj + 1, dim_y - 1)
        p11, p12, p21, p22 = p[cj, ci], p[cj1, ci], p[cj, ci1], p[cj1, ci1]
        inside = _lerp(di, _lerp(dj, p11, p12), _lerp(dj, p21, p22))
        along_x_wall, along_y_wall = _lerp(dj, p11, p12), _lerp(di, p11, p21)
        corner, x_wall, outside = (x_out & y_out)[:, None], x_out[:, None], (x_out | y_out)[:, None]
        weight = None
        if no_slip:
            beyond_x, beyond_y = np.where(x_under, -x, x - lx), np.where(y_under, -y, y - ly)
            wx = np.where(beyond_x < 0.5, F(1) - F(2) * beyond_x, F(0)).astype(F)
            wy = np.where(beyond_y < 0.5, F(1) - F(2) * beyond_y, F(0)).astype(F)
            weight = np.where(x_out, F(1) * wx, F(1)).astype(F)
            weight = np.where(y_out, weight * wy, weight).astype(F)[:, None]
        if dye:   # "T p_edge": the corner texel as stored, a wall value narrowed once; scaled, it is widened and narrowed again
            raw = field[cj, ci]
            on_wall = np.where(corner, raw, np.where(x_wall, _narrow(along_x_wall), _narrow(along_y_wall)))
            if no_slip:
                on_wall = _narrow(weight * on_wall.astype(F))
            out = np.where(outside, on_wall, _narrow(inside))
            return np.where(skip[:, None], np.uint32(0), out).astype(np.uint32)
        on_wall = np.where(corner, p11, np.where(x_wall, along_x_wall, along_y_wall))
        if no_slip:
            on_wall = weight * on_wall
        out = np.where(outside, on_wall, inside).astype(F)
    out = np.where(skip[:, None], F(np.nan), out).astype(F)
    return out[:, 0] if scalar else out


def advance(velocity, xy, dt):
    """One advance of the positions xy float32[n, 2] by dt on velocity float32[dim_y, dim_x, 2]."""
    xy = np.asarray(xy, F)
    x, y = xy[:, 0], xy[:, 1]
    skip = np.isnan(x) | np.isnan(y)
    u = sample(velocity, x, y, True)
    with np.errstate(invalid="ignore", over="ignore"):
        moved = np.stack([x + u[:, 0] * F(dt), y + u[:, 1] * F(dt)], axis=1).astype(F)
    return np.where(skip[:, None], xy, moved)


def same_bits(got, want):
    """Bit for bit, with any NaN equal to any NaN (which NaN an operation leaves is the hardware's)."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    if got.shape != want.shape or got.dtype != want.dtype:
        return False
    if got.dtype != np.float32:
        return bool(np.array_equal(got, want))
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]))
