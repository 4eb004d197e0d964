"""The loads' rule of include/sfl.h ("LOADS") restated in numpy, on the conventions of tests/solid_rule.py: scalars are
float32[dim_y, dim_x] with node (i, j) at [j, i], `solid` is bool[dim_y, dim_x], `labels` uint8[dim_y, dim_x] or None (every
solid cell is body 1).  What tests/test_loads.py checks the sanity of and what tests/test_loads_gpu.py holds the samplers of
csrc/loads.hip to, bit for bit.  The terms are formed as the header states them -- trunc(ldexp((double)p, -q)) -- and summed
as Python integers, so an overflow would show instead of wrapping.  Not part of the product."""
import numpy as np

MAX_BODIES = 16
# struct sfl_body_load, 48 bytes
DTYPE = np.dtype([("fx", "<i8"), ("fy", "<i8"), ("exp2", "<i4"), ("max_abs_p", "<f4"), ("faces", "<u4", (4,)),
                  ("nonfinite", "<u4"), ("reserved", "<u4")])
W, E, S, N = 0, 1, 2, 3   # where the FLUID cell of a face lies of its solid cell: the index into `faces`


def wet_faces(solid, labels=None):
    """The wet faces, one entry per direction W, E, S, N: (j, i of the fluid cells, body of the solid cells).  A face needs its
    solid cell inside the domain -- the slices below never leave it -- and in a body: label 0 is none."""
    solid = np.asarray(solid, bool)
    lab = np.ones(solid.shape, np.uint8) if labels is None else np.asarray(labels, np.uint8)
    assert lab.shape == solid.shape
    fluid = ~solid
    out = []
    # (fluid cells' slice, solid cells' slice): the solid cell is the fluid cell's E, W, N, S neighbour
    for f, s in ((np.s_[:, :-1], np.s_[:, 1:]), (np.s_[:, 1:], np.s_[:, :-1]), (np.s_[:-1, :], np.s_[1:, :]), (np.s_[1:, :], np.s_[:-1, :])):
        face = fluid[f] & solid[s] & (lab[s] > 0)
        j, i = np.nonzero(face)
        j0, i0 = (sl.start or 0 for sl in f)
        out.append((j + j0, i + i0, lab[s][face].astype(int)))
    return out


def exponent(max_abs_p):
    """q = floor(log2(max_abs_p)) - 32, denormals included; 0 for 0.0f."""
    m = float(np.float32(max_abs_p))
    return 0 if m == 0.0 else int(np.frexp(m)[1]) - 1 - 32


def terms(p, q):
    """t = (int64) trunc(ldexp((double) p, -q)) of finite pressures, as Python integers."""
    t = np.trunc(np.ldexp(np.asarray(p, np.float32).astype(np.float64), -q))
    assert (np.abs(t) < 2.0 ** 33).all()
    return [int(x) for x in t]


def loads(p, solid, labels=None, bodies=1):
    """The `bodies` records of one grid: DTYPE[bodies]."""
    p = np.asarray(p, np.float32)
    assert 1 <= bodies <= MAX_BODIES and p.shape == np.asarray(solid).shape
    faces = wet_faces(solid, labels)
    out = np.zeros(bodies, DTYPE)
    for b in range(1, bodies + 1):
        per_dir = [p[j[body == b], i[body == b]] for j, i, body in faces]
        finite = [x[np.isfinite(x)] for x in per_dir]
        every = np.concatenate(finite)
        rec = out[b - 1]
        rec["faces"] = [len(x) for x in per_dir]
        rec["nonfinite"] = sum(len(x) for x in per_dir) - len(every)
        if len(every):   # the maximum over the bit patterns of |p|
            rec["max_abs_p"] = (np.ascontiguousarray(every).view(np.uint32) & np.uint32(0x7FFFFFFF)).max().view(np.float32)
        q = exponent(rec["max_abs_p"])
        sums = [sum(terms(x, q)) for x in finite]
        fx, fy = sums[W] - sums[E], sums[S] - sums[N]
        assert -2 ** 63 <= fx < 2 ** 63 and -2 ** 63 <= fy < 2 ** 63
        rec["fx"], rec["fy"], rec["exp2"] = fx, fy, q
    return out


def loads_xy(rec):
    """fx * 2^exp2, fy * 2^exp2 as float64[..., 2]."""
    scale = np.ldexp(1.0, rec["exp2"].astype(np.int64))
    return np.stack([rec["fx"].astype(np.float64) * scale, rec["fy"].astype(np.float64) * scale], axis=-1)
