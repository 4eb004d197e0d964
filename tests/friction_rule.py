"""The friction's rule of include/sfl.h ("FRICTION") restated in numpy, on the conventions and on the pieces of
tests/load_rule.py: the wet faces, the exponent and the terms are that module's, so that the two rules cannot drift apart.
`v` is float32[dim_y, dim_x, 2] with node (i, j) at [j, i] and (x, y) last, `solid` is bool[dim_y, dim_x], `labels`
uint8[dim_y, dim_x] or None (every solid cell is body 1).  What tests/test_friction.py checks the sanity of and what
tests/test_friction_gpu.py holds the samplers of csrc/friction.hip to, bit for bit.  The sums are Python integers, so an
overflow would show instead of wrapping.  Not part of the product."""
import numpy as np

import load_rule
from load_rule import MAX_BODIES, W, E, S, N   # noqa: F401  (the directions index `faces`, as in the loads)

# struct sfl_body_friction, 48 bytes: the offsets of sfl_body_load
DTYPE = np.dtype([("fx", "<i8"), ("fy", "<i8"), ("exp2", "<i4"), ("max_abs_t", "<f4"), ("faces", "<u4", (4,)),
                  ("nonfinite", "<u4"), ("reserved", "<u4")])
# the tangential component of a face by direction: the fluid cell W or E of the solid one slides along y, S or N along x
TANGENT = {W: 1, E: 1, S: 0, N: 0}


def friction(v, solid, labels=None, bodies=1):
    """The `bodies` records of one grid: DTYPE[bodies]."""
    v = np.asarray(v, np.float32)
    assert 1 <= bodies <= MAX_BODIES and v.shape == np.asarray(solid).shape + (2,)
    faces = load_rule.wet_faces(solid, labels)
    out = np.zeros(bodies, DTYPE)
    for b in range(1, bodies + 1):
        per_dir = [v[j[body == b], i[body == b], TANGENT[d]] for d, (j, i, body) in enumerate(faces)]
        finite = [x[np.isfinite(x)] for x in per_dir]   # (the normal component is not looked at)
        every = np.concatenate(finite)
        rec = out[b - 1]
        rec["faces"] = [len(x) for x in per_dir]
        rec["nonfinite"] = sum(len(x) for x in per_dir) - len(every)
        if len(every):   # the maximum over the bit patterns of |v_t|
            rec["max_abs_t"] = (np.ascontiguousarray(every).view(np.uint32) & np.uint32(0x7FFFFFFF)).max().view(np.float32)
        q = load_rule.exponent(rec["max_abs_t"])   # ONE q for fx and fy
        sums = [sum(load_rule.terms(x, q)) for x in finite]
        fx, fy = sums[S] + sums[N], sums[W] + sums[E]   # plain signs: the fluid drags the body along
        assert -2 ** 63 <= fx < 2 ** 63 and -2 ** 63 <= fy < 2 ** 63
        rec["fx"], rec["fy"], rec["exp2"] = fx, fy, q
    return out


def friction_xy(rec, nu):
    """nu * fx * 2^exp2, nu * fy * 2^exp2 as float64[..., 2]: the force per unit depth and density -- no factor dx.  nu
    broadcasts against the records' shape."""
    scale = np.ldexp(1.0, rec["exp2"].astype(np.int64)) * np.asarray(nu, np.float64)
    return np.stack([rec["fx"].astype(np.float64) * scale, rec["fy"].astype(np.float64) * scale], axis=-1)
