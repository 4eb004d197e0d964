"""The rule of the averages (include/sfl.h "AVERAGES") restated in numpy: per-cell sums over time of the fields held, one
IEEE-754 double addition per plane, cell and sample, in sample order; 64-bit integer sums of the raw UQ32 dye.  The tests hold
the device's planes to this BIT FOR BIT; there is no tolerance anywhere.

numpy's float64 arithmetic is IEEE on every platform this suite runs on: `a.astype(float64)` is exact for a float32
(denormals included), the product of two such values is exact (48 <= 53 bits), and `+=` rounds once."""
import numpy as np

VELOCITY, STRESS, PRESSURE, DYE, ALL = 1, 2, 4, 8, 15
U, V, UU, VV, UV, P, PP, R, G, B = range(10)
PLANES = 10
NAMES = ("U", "V", "UU", "VV", "UV", "P", "PP", "R", "G", "B")
GROUP_OF = (VELOCITY, VELOCITY, STRESS, STRESS, STRESS, PRESSURE, PRESSURE, DYE, DYE, DYE)


def planes_of(what):
    """The ids of the planes that exist under the mask `what`, in order."""
    return [k for k in range(PLANES) if what & GROUP_OF[k]]


def dtype_of(plane):
    return np.uint64 if GROUP_OF[plane] == DYE else np.float64


def start(what, shape):
    """Every plane of `what` at its start value: +0.0, or 0 for the dye planes.  shape: (..., dim_y, dim_x)."""
    return {k: np.zeros(shape, dtype_of(k)) for k in planes_of(what)}


def terms(what, v, p, dye):
    """What ONE sample adds per plane: v of shape (..., 2) float32, p (...) float32, dye (..., 3) uint32."""
    out = {}
    if what & (VELOCITY | STRESS):
        assert v.dtype == np.float32
        x, y = v[..., 0].astype(np.float64), v[..., 1].astype(np.float64)
    if what & VELOCITY:
        out[U], out[V] = x, y
    if what & STRESS:
        out[UU], out[VV], out[UV] = x * x, y * y, x * y
    if what & PRESSURE:
        assert p.dtype == np.float32
        q = p.astype(np.float64)
        out[P], out[PP] = q, q * q
    if what & DYE:
        assert dye.dtype == np.uint32
        out[R], out[G], out[B] = (dye[..., c].astype(np.uint64) for c in range(3))
    return out


def add(sums, what, v, p, dye):
    """One sample into `sums` (of start()), in place: one rounded addition per plane and cell."""
    with np.errstate(all="ignore"):   # (Inf - Inf and Inf * 0 are NaN by IEEE: that is the rule, not an accident)
        for k, t in terms(what, v, p, dye).items():
            sums[k] += t   # uint64: wraps modulo 2^64, which 2^32 samples of values below 2^32 cannot reach
    return sums


def sums(what, samples):
    """The planes after the samples [(v, p, dye), ...] in order."""
    out = None
    for v, p, dye in samples:
        if out is None:
            out = start(what, v.shape[:-1] if v is not None else p.shape if p is not None else dye.shape[:-1])
        add(out, what, v, p, dye)
    return out


def means(s, n):
    """sum / samples of every plane, float64."""
    return {k: a.astype(np.float64) / np.float64(n) for k, a in s.items()}


def reynolds_stress(s, n):
    """The central moments <u'u'>, <v'v'>, <u'v'> and the turbulent kinetic energy from the sums, float64."""
    m = means(s, n)
    uu, vv, uv = m[UU] - m[U] * m[U], m[VV] - m[V] * m[V], m[UV] - m[U] * m[V]
    return {"uu": uu, "vv": vv, "uv": uv, "tke": 0.5 * (uu + vv)}
