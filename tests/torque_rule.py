"""The torque's rule of include/sfl.h ("TORQUE") restated in numpy, on the conventions and on the pieces of
tests/load_rule.py and tests/friction_rule.py: the wet faces, the exponents q and the terms are those modules', so that the
three rules cannot drift apart.  `p` is float32[dim_y, dim_x], `v` float32[dim_y, dim_x, 2] with node (i, j) at [j, i] and
(x, y) last, `solid` bool[dim_y, dim_x], `labels` uint8[dim_y, dim_x] or None (every solid cell is body 1), `pivot2`
int32[bodies, 2] in HALF cells or None (every pivot (0, 0)).  What tests/test_torque.py checks the sanity of and what
tests/test_torque_gpu.py holds the samplers of csrc/torque.hip to, bit for bit.  The sums are Python integers, and the rule
asserts the header's bound |sum| < 2^63 instead of wrapping.  Not part of the product."""
import numpy as np

import load_rule
from friction_rule import TANGENT
from load_rule import MAX_BODIES, W, E, S, N   # noqa: F401

MAX_PIVOT2 = 1 << 24
# struct sfl_body_torque, 64 bytes
DTYPE = np.dtype([("mp", "<i8"), ("mf", "<i8"), ("exp2_p", "<i4"), ("exp2_f", "<i4"), ("max_abs_p", "<f4"), ("max_abs_t", "<f4"),
                  ("faces", "<u4"), ("max_arm2", "<u4"), ("nonfinite_p", "<u4"), ("nonfinite_t", "<u4"), ("pivot2", "<i4", (2,)),
                  ("reserved", "<u4", (2,))])
# the solid cell of a face from its fluid cell, (di, dj) by direction: the fluid cell lies W, E, S, N of the solid one
SOLID_OF = {W: (1, 0), E: (-1, 0), S: (0, 1), N: (0, -1)}


def bit_length(x):
    """L(x): 0 for 0."""
    return int(x).bit_length()


def shift(faces, max_arm2):
    """s = max(0, L(faces) + L(max_arm2) - 30)."""
    return max(0, bit_length(faces) + bit_length(max_arm2) - 30)


def pressure_product(d, rx2, ry2, tp):
    """What a face adds to mp: -ry2*tp, +ry2*tp, +rx2*tp, -rx2*tp for d = W, E, S, N."""
    return (-ry2 * tp, ry2 * tp, rx2 * tp, -rx2 * tp)[d]


def friction_product(d, rx2, ry2, tf):
    """What a face adds to mf: +rx2*tf for W and E (tf from v.y), -ry2*tf for S and N (tf from v.x)."""
    return rx2 * tf if d in (W, E) else -ry2 * tf


def max_bits(x):
    """The maximum of |x| over the finite values, by the bit patterns; 0.0f when there is none."""
    x = np.asarray(x, np.float32)
    x = x[np.isfinite(x)]
    if not len(x):
        return np.float32(0)
    return (np.ascontiguousarray(x).view(np.uint32) & np.uint32(0x7FFFFFFF)).max().view(np.float32)


def face_list(p, v, solid, labels, b, px2, py2):
    """The wet faces of body b: (d, rx2, ry2, p, v_t) per face, the arms as Python integers."""
    out = []
    for d, (j, i, body) in enumerate(load_rule.wet_faces(solid, labels)):
        di, dj = SOLID_OF[d]
        for jj, ii in zip(j[body == b].tolist(), i[body == b].tolist()):
            out.append((d, 2 * (ii + di) - px2, 2 * (jj + dj) - py2, p[jj, ii], v[jj, ii, TANGENT[d]]))
    return out


def torque(p, v, solid, labels=None, bodies=1, pivot2=None):
    """The `bodies` records of one grid: DTYPE[bodies]."""
    p, v = np.asarray(p, np.float32), np.asarray(v, np.float32)
    assert 1 <= bodies <= MAX_BODIES and p.shape == np.asarray(solid).shape and v.shape == p.shape + (2,)
    piv = np.zeros((bodies, 2), np.int64) if pivot2 is None else np.asarray(pivot2, np.int64)
    assert piv.shape == (bodies, 2) and (np.abs(piv) <= MAX_PIVOT2).all()
    out = np.zeros(bodies, DTYPE)
    for b in range(1, bodies + 1):
        rec = out[b - 1]
        px2, py2 = int(piv[b - 1, 0]), int(piv[b - 1, 1])
        rec["pivot2"] = (px2, py2)
        faces = face_list(p, v, solid, labels, b, px2, py2)
        if not faces:
            continue   # all zeros but the pivot
        rec["faces"] = len(faces)
        rec["max_arm2"] = max(max(abs(rx2), abs(ry2)) for _, rx2, ry2, _, _ in faces)
        rec["max_abs_p"] = max_bits([f[3] for f in faces])
        rec["max_abs_t"] = max_bits([f[4] for f in faces])
        s = shift(rec["faces"], rec["max_arm2"])
        q_p, q_f = load_rule.exponent(rec["max_abs_p"]) + s, load_rule.exponent(rec["max_abs_t"]) + s
        mp = mf = 0
        bound = 2 ** (33 - s + bit_length(rec["max_arm2"]) + bit_length(rec["faces"]))
        assert bound <= 2 ** 63
        for d, rx2, ry2, pf, vt in faces:
            if np.isfinite(pf):
                tp = load_rule.terms([pf], q_p)[0]
                assert abs(tp) < 2 ** (33 - s)
                mp += pressure_product(d, rx2, ry2, tp)
            else:
                rec["nonfinite_p"] += 1
            if np.isfinite(vt):
                tf = load_rule.terms([vt], q_f)[0]
                assert abs(tf) < 2 ** (33 - s)
                mf += friction_product(d, rx2, ry2, tf)
            else:
                rec["nonfinite_t"] += 1
        assert abs(mp) < bound and abs(mf) < bound, "the header's bound: |sum| < 2^(33 - s + L(max_arm2) + L(faces)) <= 2^63"
        rec["mp"], rec["mf"], rec["exp2_p"], rec["exp2_f"] = mp, mf, q_p, q_f
    return out


def torque_xy(rec, dx=1.0, rho=1.0, nu=1.0):
    """float64[..., 2]: the pressure torque mp * 2^(exp2_p - 1) * dx^2 and the friction torque per unit depth
    rho * nu * mf * 2^(exp2_f - 1) * dx.  nu broadcasts against the records' shape."""
    mp = rec["mp"].astype(np.float64) * np.ldexp(1.0, rec["exp2_p"].astype(np.int64) - 1) * (float(dx) * float(dx))
    mf = rec["mf"].astype(np.float64) * np.ldexp(1.0, rec["exp2_f"].astype(np.int64) - 1) * np.asarray(nu, np.float64) * (float(rho) * float(dx))
    return np.stack([mp, mf], axis=-1)
