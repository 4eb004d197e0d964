"""Ensembles on the GPU: the distance between two sets of fields (sfl_distance, sfl_batch_distance) and the per-cell envelope of
the dye over the members of a batch (sfl_batch_envelope*).

The contract under test (include/sfl.h): every figure is, bit for bit, what numpy gives on the downloaded (or uploaded)
fields -- maxima of bit patterns, integer maxima, counts and exact integer sums do not depend on the order of reduction, so
there is no tolerance anywhere; a NaN is matched by any NaN.  The yardsticks are `yardstick` (np.max(np.abs(a - b)) in
float32, which propagates NaN; int64 differences for the dye; bitwise inequality per cell) and `envelope_yardstick` (min, max,
sum(uint64) // count over axis 0).  tests/test_ensemble.py has the CPU side."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_bit_equal, random_fields
from test_batch_params import assert_report_equal

SHAPES = [(2, 2), (3, 3), (61, 81), (130, 70), (96, 65), (257, 130), (1030, 67), (2, 4000)]
V, D, P = 1, 2, 4          # SFL_DIST_VELOCITY, SFL_DIST_DYE, SFL_DIST_PRESSURE
FV, FC, FDIV, FP = 0, 1, 2, 3       # SFL_FIELD_VELOCITY, SFL_FIELD_COLOR, SFL_FIELD_DIVERGENCE, SFL_FIELD_PRESSURE
ZERO = {"velocity_cells_differ": 0, "dye_cells_differ": 0, "pressure_cells_differ": 0}


# ---- the yardsticks -----------------------------------------------------------------------------------
def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def yardstick(a, b, what=V | D | P):
    """The record of fields a = (v, c, p) against b, as numpy has it; the parts not asked for are zero."""
    w = {"max_abs_dvx": np.float32(0), "max_abs_dvy": np.float32(0), "max_abs_dp": np.float32(0), "what": what,
         "velocity_cells_differ": 0, "dye_cells_differ": 0, "pressure_cells_differ": 0, "max_abs_ddye": [0, 0, 0], "sum_abs_ddye": [0, 0, 0]}
    with np.errstate(all="ignore"):
        if what & V:
            d = a[0] - b[0]
            assert d.dtype == np.float32
            w["max_abs_dvx"], w["max_abs_dvy"] = np.max(np.abs(d[..., 0])), np.max(np.abs(d[..., 1]))
            w["velocity_cells_differ"] = int(np.count_nonzero((u32(a[0]) != u32(b[0])).any(axis=-1)))
        if what & D:
            d = np.abs(a[1].astype(np.int64) - b[1].astype(np.int64)).reshape(-1, 3)
            w["max_abs_ddye"] = [int(x) for x in d.max(axis=0)]
            w["sum_abs_ddye"] = [int(x) for x in d.sum(axis=0)]
            w["dye_cells_differ"] = int(np.count_nonzero((a[1] != b[1]).any(axis=-1)))
        if what & P:
            d = a[2] - b[2]
            assert d.dtype == np.float32
            w["max_abs_dp"] = np.max(np.abs(d))
            w["pressure_cells_differ"] = int(np.count_nonzero(u32(a[2]) != u32(b[2])))
    return w


def assert_distance(got, want, what):
    """One record against the yardstick's: bit for bit (a NaN by any NaN), the parts not asked for zero."""
    print(f"{what}: got {got}, want {want}")
    assert int(got["what"]) == want["what"], what
    for name in ("max_abs_dvx", "max_abs_dvy", "max_abs_dp"):
        assert_report_equal(got[name], want[name], f"{what}: {name}")
    for name in ZERO:
        assert int(got[name]) == want[name], f"{what}: {name} {int(got[name])}, want {want[name]}"
    assert got["sum_abs_ddye"].dtype == np.uint64 and got["max_abs_ddye"].dtype == np.uint32
    assert [int(x) for x in got["max_abs_ddye"]] == want["max_abs_ddye"], f"{what}: max_abs_ddye"
    assert [int(x) for x in got["sum_abs_ddye"]] == want["sum_abs_ddye"], f"{what}: sum_abs_ddye"


def flags(bits):
    return dict(velocity=bool(bits & V), dye=bool(bits & D), pressure=bool(bits & P))


@functools.lru_cache(maxsize=None)
def fields(dim_x, dim_y, seed=0):
    """(v, c, p): a random velocity (|v| <= 100), a dye drawn over the whole UQ32 range, a pressure.  Shared: never written to."""
    v, _, p = random_fields(dim_x, dim_y, 300 + dim_x + seed)
    c = np.random.default_rng(11 + dim_x + seed).integers(0, 2 ** 32, (dim_y, dim_x, 3), dtype=np.uint32)
    for a in (v, c, p):
        a.setflags(write=False)
    return v, c, p


@functools.lru_cache(maxsize=None)
def fields_nearby(dim_x, dim_y, seed=0):
    """fields() with about a third of the cells of each field replaced: the counts are neither 0 nor all cells."""
    a, other = fields(dim_x, dim_y, seed), fields(dim_x, dim_y, seed + 5000)
    rng = np.random.default_rng(23 + dim_x + seed)
    out = []
    for x, y in zip(a, other):
        mask = rng.random((dim_y, dim_x)) < 0.3
        z = x.copy()
        z[mask] = y[mask]
        z.setflags(write=False)
        out.append(z)
    return tuple(out)


def upload(s, f, first=None):
    for field, a in zip((FV, FC, FP), f):
        if first is None:
            s.upload(field, a)
        else:
            s.upload(field, a, first)


def boundary_cells(sfl, lane_cells, cells):
    """The first and the last cell, and the cells on both sides of every kind of internal boundary of a distance pass whose
    lanes hold `lane_cells` cells: between two lanes, two waves, two loads of the workgroup, two items, and between the
    last whole lane and the cells read one at a time behind it.  The constants are the library's own (solver.py, from
    csrc/ensemble_kernels.h)."""
    assert (sfl.DIST_THREADS, sfl.DIST_ITEM_LOADS) == (256, 8)
    row = sfl.DIST_THREADS * lane_cells
    edges = [lane_cells, 64 * lane_cells, row, 2 * row, row * sfl.DIST_ITEM_LOADS, 2 * row * sfl.DIST_ITEM_LOADS, cells - cells % lane_cells]
    out = {0, cells - 1}
    for e in edges:
        out |= {c for c in (e - 1, e) if 0 <= c < cells}
    return sorted(out)


KINDS = [  # (bit, field index in (v, c, p), words per cell, lane cells name)
    (V, 0, 2, "DIST_VELOCITY_LANE_CELLS"), (D, 1, 3, "DIST_DYE_LANE_CELLS"), (P, 2, 1, "DIST_PRESSURE_LANE_CELLS")]


def changed_word(x, cell, word, words):
    """A copy of field x with one word of one cell changed (flat cell index), and the word's old and new value."""
    q = x.copy()
    flat = q.reshape(-1, words)
    old = flat[cell, word]
    flat[cell, word] = old ^ np.uint32(0x00ABCDEF) if q.dtype == np.uint32 else np.float32(old + np.float32(1000.5))
    return q, old, flat[cell, word]


def want_one_word(bit, word, old, new):
    """The record when exactly one word differs, worked out by hand: one cell, max and sum exact."""
    w = yardstick(None, None, 0)
    w["what"] = bit
    with np.errstate(all="ignore"):
        if bit == V:
            w["velocity_cells_differ"] = 1
            w["max_abs_dvx" if word == 0 else "max_abs_dvy"] = np.abs(np.float32(new) - np.float32(old))
        elif bit == P:
            w["pressure_cells_differ"] = 1
            w["max_abs_dp"] = np.abs(np.float32(new) - np.float32(old))
        else:
            w["dye_cells_differ"] = 1
            w["max_abs_ddye"][word] = w["sum_abs_ddye"][word] = abs(int(new) - int(old))
    return w


# ---- contexts -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_random_fields_each_part_alone_and_all_three(sfl, dim_x, dim_y):
    fa, fb = fields(dim_x, dim_y), fields_nearby(dim_x, dim_y)
    tag = f"{dim_x} x {dim_y}"
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        assert_distance(a.distance(b), yardstick(fa, fa), f"{tag}: two fresh contexts")
        upload(a, fa)
        upload(b, fb)
        full = yardstick(fa, fb)
        assert 0 < full["velocity_cells_differ"] < dim_x * dim_y or dim_x * dim_y < 10
        for bits in (V, D, P, V | D, V | P, D | P, V | D | P):
            assert_distance(a.distance(b, **flags(bits)), yardstick(fa, fb, bits), f"{tag}: what {bits}")
        assert_distance(b.distance(a), yardstick(fb, fa), f"{tag}: b against a")
        assert_distance(a.distance(a), yardstick(fa, fa), f"{tag}: a against itself")
        for s, f in ((a, fa), (b, fb)):     # the call reads only
            for field, x in zip((FV, FC, FP), f):
                assert_bit_equal(s.download(field), x, f"{tag}: field {field} after distance()")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (130, 70), (2, 4000)])
def test_a_single_differing_word_is_found_wherever_it_sits(sfl, dim_x, dim_y):
    f = fields(dim_x, dim_y)
    cells = dim_x * dim_y
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        upload(a, f)
        upload(b, f)
        for bit, k, words, lane_name in KINDS:
            field = (FV, FC, FP)[k]
            for cell in boundary_cells(sfl, getattr(sfl, lane_name), cells):
                for word in range(words):
                    q, old, new = changed_word(f[k], cell, word, words)
                    b.upload(field, q)
                    tag = f"{dim_x} x {dim_y}: bit {bit}, word {word} of cell {cell}"
                    assert_distance(b.distance(a, **flags(bit)), want_one_word(bit, word, new, old), tag)
                    assert_distance(a.distance(b), want_one_word(bit, word, old, new) | {"what": 7}, tag + ", all three parts")
            b.upload(field, f[k])
        assert_distance(a.distance(b), yardstick(f, f), "everything put back")


@pytest.mark.gpu
def test_the_largest_dye_differences(sfl):
    dim_x, dim_y = 61, 81
    ca, cb = np.zeros((dim_y, dim_x, 3), np.uint32), np.zeros((dim_y, dim_x, 3), np.uint32)
    ca[0, 0, 0], cb[0, 0, 0] = 0xFFFFFFFF, 0             # 2^32 - 1
    ca[40, 30, 1], cb[40, 30, 1] = 0, 0xFFFFFFFF          # ... the other way round
    ca[-1, -1, 2], cb[-1, -1, 2] = 2 ** 31, 2 ** 31 - 1   # across the sign bit of an int32: 1
    ca[-1, -2, 2], cb[-1, -2, 2] = 2 ** 31 - 1, 2 ** 31
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        a.upload(FC, ca)
        b.upload(FC, cb)
        got = a.distance(b, velocity=False, pressure=False)
    want = yardstick((None, ca, None), (None, cb, None), D)
    assert want["max_abs_ddye"] == [2 ** 32 - 1, 2 ** 32 - 1, 1] and want["sum_abs_ddye"] == [2 ** 32 - 1, 2 ** 32 - 1, 2] and want["dye_cells_differ"] == 4
    assert_distance(got, want, "0xFFFFFFFF against 0, 2^31 against 2^31 - 1")
    # every cell at the largest difference: the sums pass 2^32 by far
    ca, cb = np.full((dim_y, dim_x, 3), 0xFFFFFFFF, np.uint32), np.zeros((dim_y, dim_x, 3), np.uint32)
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        a.upload(FC, ca)
        got = b.distance(a, velocity=False, pressure=False)
    want = yardstick((None, cb, None), (None, ca, None), D)
    assert want["sum_abs_ddye"] == [dim_x * dim_y * 0xFFFFFFFF] * 3
    assert_distance(got, want, "every value at 2^32 - 1")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (130, 70)])
def test_non_finite_values_and_signed_zeros(sfl, dim_x, dim_y):
    f = fields(dim_x, dim_y)
    j, i = dim_y // 2, dim_x // 3
    payload = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        upload(a, f)
        upload(b, f)

        def put(va, vb):
            """va / vb into one word of a's / b's velocity (component 1) and pressure; both records."""
            qa, qb, pa, pb = f[0].copy(), f[0].copy(), f[2].copy(), f[2].copy()
            qa[j, i, 1], qb[j, i, 1], pa[j, i], pb[j, i] = va, vb, va, vb
            a.upload(FV, qa), b.upload(FV, qb), a.upload(FP, pa), b.upload(FP, pb)
            got, want = a.distance(b), yardstick((qa, f[1], pa), (qb, f[1], pb))
            assert_distance(got, want, f"{dim_x} x {dim_y}: {va!r} against {vb!r}")
            return got

        got = put(np.float32(np.nan), f[0][j, i, 1])          # a NaN on one side
        assert np.isnan(got["max_abs_dvy"]) and np.isnan(got["max_abs_dp"]) and got["max_abs_dvx"] == 0
        assert got["velocity_cells_differ"] == 1 and got["pressure_cells_differ"] == 1
        for inf in (np.float32(np.inf), np.float32(-np.inf)):  # the same inf on both sides: inf - inf is a NaN, the bits are equal
            got = put(inf, inf)
            assert np.isnan(got["max_abs_dvy"]) and np.isnan(got["max_abs_dp"])
            assert got["velocity_cells_differ"] == 0 and got["pressure_cells_differ"] == 0
        got = put(np.float32(np.inf), np.float32(-np.inf))
        assert np.isposinf(got["max_abs_dvy"]) and got["velocity_cells_differ"] == 1
        got = put(np.float32(0.0), np.float32(-0.0))           # |+0 - -0| = +0.0f, and the cell differs
        assert got["max_abs_dvy"].view(np.uint32) == 0 and got["max_abs_dp"].view(np.uint32) == 0
        assert got["velocity_cells_differ"] == 1 and got["pressure_cells_differ"] == 1
        got = put(np.float32(-0.0), np.float32(0.0))
        assert got["max_abs_dvy"].view(np.uint32) == 0 and got["velocity_cells_differ"] == 1
        got = put(payload, payload)                             # the same NaN payload on both sides: the cell is equal
        assert np.isnan(got["max_abs_dvy"]) and got["velocity_cells_differ"] == 0 and got["pressure_cells_differ"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (130, 70)])
def test_step_n_against_single_steps_is_the_same_bits_in_one_call(sfl, dim_x, dim_y):
    """The library's own contract: sfl_step_n(3) with a queued drag leaves what three sfl_step calls leave."""
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        for s in (a, b):
            s.setup_sketch_fields()
            s.queue_drags([(40, 20, 30.0, -12.0), (41, 20, 8.0, 25.0)])
        a.step_n(3, 0.05, 1.0, 20, 1.9)
        for _ in range(3):
            b.step(0.05, 1.0, 20, 1.9)
        got = a.distance(b)
        fa, fb = [a.download(k) for k in (FV, FC, FP)], [b.download(k) for k in (FV, FC, FP)]
    assert_distance(got, yardstick(fa, fb), f"{dim_x} x {dim_y}: step_n(3) against three steps")
    assert {k: int(got[k]) for k in ZERO} == ZERO
    assert np.abs(fa[0]).max() > 0 and np.abs(fa[2]).max() > 0, "the flow must have moved"


@pytest.mark.gpu
def test_a_folded_twin_is_as_far_away_as_numpy_says(sfl):
    """SFL_OPT_SOR_FOLD = 1 on a quiescent start with one drag: whatever the distance is, it is numpy's on the downloads."""
    dim_x, dim_y = 257, 130
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        b.set_option(sfl.capi.OPT_SOR_FOLD, 1)
        for s in (a, b):
            s.setup_sketch_fields()
            s.queue_drags([(40, 20, 30.0, -12.0)])
            s.step_n(3, 0.05, 1.0, 20, 1.9)
        got = a.distance(b)
        fa, fb = [a.download(k) for k in (FV, FC, FP)], [b.download(k) for k in (FV, FC, FP)]
    assert_distance(got, yardstick(fa, fb), "exact against folded")


@pytest.mark.gpu
def test_contexts_that_do_not_match_are_refused(sfl):
    with sfl.Solver(130, 70) as a, sfl.Solver(130, 71) as b, sfl.Solver(130, 70, rank=0, nranks=2) as slab:
        for other, code, message in ((b, sfl.capi.ERR_INVALID, "shapes must be the same"), (slab, sfl.capi.ERR_STATE, "whole-domain contexts only")):
            with pytest.raises(sfl.SflError) as e:
                a.distance(other)
            assert e.value.code == code and message in str(e.value), str(e.value)


@pytest.mark.gpu
def test_more_items_than_workgroups(sfl):
    """3001 x 2900 = 8.7 million cells: the velocity and the dye have more items than the capped grid has workgroups (they
    stride), the cell count is odd, and single differing words sit in the last cell and in a cell of the last items."""
    dim_x, dim_y = 3001, 2900
    rng = np.random.default_rng(3001)
    v = rng.random((dim_y, dim_x, 2), dtype=np.float32)
    c = rng.integers(0, 2 ** 32, (dim_y, dim_x, 3), dtype=np.uint32)
    v2, c2 = v.copy(), c.copy()
    v2[-1, -1, 1] += np.float32(3.0)
    v2[-3, 5, 0] -= np.float32(7.0)
    c2[-1, -1, 2] ^= np.uint32(0x80000000)
    c2[17, 2000, 0] ^= np.uint32(1)
    with sfl.Solver(dim_x, dim_y) as a, sfl.Solver(dim_x, dim_y) as b:
        a.upload(FV, v), a.upload(FC, c), b.upload(FV, v2), b.upload(FC, c2)
        got = a.distance(b, pressure=False)
    want = yardstick((v, c, None), (v2, c2, None), V | D)
    assert want["velocity_cells_differ"] == 2 and want["dye_cells_differ"] == 2 and want["max_abs_ddye"] == [1, 0, 2 ** 31]
    assert_distance(got, want, "3001 x 2900")


# ---- batches ------------------------------------------------------------------------------------------
BATCHES = [(61, 81, 5, False), (8, 6, 7, False), (96, 96, 3, True)]   # 61 x 81: member bases that are not 16-byte aligned


@functools.lru_cache(maxsize=None)
def batch_fields(dim_x, dim_y, batch):
    """Member 0 = fields(); member m = member 0 with about a third of its cells replaced, differently for each m."""
    base, per = fields(dim_x, dim_y), []
    for m in range(batch):
        other = fields(dim_x, dim_y, 77 * (m + 1))
        mask = np.random.default_rng(m).random((dim_y, dim_x)) < (0.3 if m else 0.0)
        per.append(tuple(np.where(mask[..., None] if x.ndim == 3 else mask, y, x) for x, y in zip(base, other)))
    out = tuple(np.stack([p[k] for p in per]) for k in range(3))
    for a in out:
        a.setflags(write=False)
    return out


def member(f, m):
    return tuple(x[m] for x in f)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,batch,large", BATCHES)
def test_every_member_against_a_reference_member(sfl, dim_x, dim_y, batch, large):
    f = batch_fields(dim_x, dim_y, batch)
    tag = f"{dim_x} x {dim_y} x {batch}"
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        b.upload(FV, f[0])
        b.upload(FC, f[1])
        b.upload(FDIV, f[2])
        b.poisson_solve_each(1.0, 3, 1.9)          # a pressure of each member's own, and a valid residual report
        f = (f[0], f[1], b.download(FP))
        assert np.abs(f[2]).max() > 0
        residual = b.residual()
        for ref in (0, 2, batch - 1):
            got = b.distance(ref_member=ref)
            assert got.dtype == sfl.FIELD_DISTANCE_DTYPE and got.shape == (batch,)
            for m in range(batch):
                assert_distance(got[m], yardstick(member(f, m), member(f, ref)), f"{tag}: member {m} against member {ref}")
            assert {k: int(got[ref][k]) for k in ZERO} == ZERO
            assert b.distance(b, ref_member=ref).tobytes() == got.tobytes(), f"{tag}: ref = the batch itself"
        full = b.distance(ref_member=2)
        count = min(3, batch - 1)
        part = b.distance(ref_member=2, first=1, count=count)
        assert part.tobytes() == full[1:1 + count].tobytes(), f"{tag}: members [1, 1 + {count})"
        for bits in (V, D, P):
            for m, rec in enumerate(b.distance(ref_member=0, first=1, count=count, **flags(bits))):
                assert_distance(rec, yardstick(member(f, 1 + m), member(f, 0), bits), f"{tag}: member {1 + m}, part {bits}")
        pair = b.distance()      # pairwise against itself
        for m in range(batch):
            assert_distance(pair[m], yardstick(member(f, m), member(f, m)), f"{tag}: member {m} against itself")
        assert b.distance(count=0).shape == (0,)
        # what is refused, with a batch at hand
        with pytest.raises(sfl.SflError, match="not inside the batch"):
            b.distance(ref_member=0, first=1, count=batch)
        with pytest.raises(sfl.SflError, match="ref_member"):
            b.distance(ref_member=batch)
        # the call reads only: the fields and the residual report are as they were
        assert_bit_equal(b.residual(), residual, f"{tag}: residual() after distance()")
        for field, x in zip((FV, FC, FP), f):
            assert_bit_equal(b.download(field), x, f"{tag}: field {field} after distance()")
    # a member's record is the record of two contexts holding those fields
    with sfl.Solver(dim_x, dim_y) as sa, sfl.Solver(dim_x, dim_y) as sb:
        upload(sb, member(f, 2))
        for m in range(batch):
            upload(sa, member(f, m))
            assert sa.distance(sb).tobytes() == full[m].tobytes(), f"{tag}: member {m} against two contexts"


@pytest.mark.gpu
def test_a_single_differing_word_in_a_member_whose_base_is_not_aligned(sfl):
    """61 x 81 = 4941 cells: member 1 starts 4941 * 8 (velocity), * 12 (dye), * 4 (pressure) bytes into the field, none a
    multiple of 16.  One word of member 1 changed at its unaligned head, at its tail and at the kernel's boundaries."""
    dim_x, dim_y, batch = 61, 81, 3
    f = fields(dim_x, dim_y)
    cells = dim_x * dim_y
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        for m in range(batch):
            upload(b, tuple(x[None] for x in f), m)
        for bit, k, words, lane_name in KINDS:
            field = (FV, FC, FP)[k]
            for cell in boundary_cells(sfl, getattr(sfl, lane_name), cells):
                for word in (0, words - 1):
                    q, old, new = changed_word(f[k], cell, word, words)
                    b.upload(field, q[None], 1)
                    tag = f"bit {bit}, word {word} of cell {cell} of member 1"
                    got = b.distance(ref_member=0, **flags(bit))
                    assert_distance(got[1], want_one_word(bit, word, new, old), tag)
                    for m in (0, 2):
                        assert_distance(got[m], yardstick(None, None, 0) | {"what": bit}, tag + f": member {m}")
                    got = b.distance(ref_member=1, **flags(bit))     # ... and with the changed member as the fixed reference
                    for m in (0, 2):
                        assert_distance(got[m], want_one_word(bit, word, old, new), tag + f": member {m} against it")
            b.upload(field, f[k][None], 1)


@pytest.mark.gpu
def test_more_members_than_workgroups(sfl):
    """2100 members of 8 x 6: one item per member and more items than the capped grid has workgroups, so a workgroup strides
    from member to member and leaves each one's figures before it takes the next."""
    dim_x, dim_y, batch = 8, 6, 2100
    rng = np.random.default_rng(2100)
    f = ((rng.standard_normal((batch, dim_y, dim_x, 2)) * (rng.random((batch, 1, 1, 1)) < 0.5)).astype(np.float32),
         rng.integers(0, 2 ** 32, (batch, dim_y, dim_x, 3), dtype=np.uint32) >> rng.integers(0, 32, (batch, 1, 1, 1), dtype=np.uint32),
         rng.standard_normal((batch, dim_y, dim_x)).astype(np.float32))
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        upload(b, f, 0)
        fixed, pair = b.distance(ref_member=1234), b.distance()
    for m in range(batch):
        assert_distance(fixed[m], yardstick(member(f, m), member(f, 1234)), f"member {m} of {batch}")
    assert not pair.view(np.uint8).reshape(batch, 64)[:, :12].any() and not pair.view(np.uint8).reshape(batch, 64)[:, 16:].any()


FORCES = ([0, 2, 1], [(20, 40), (30, 10), (5, 5)], [(-12.0, 30.0), (9.0, -25.0), (3.0, 4.0)])


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,batch,large", [(61, 81, 3, False), (96, 96, 3, True)])
def test_twins_pairwise(sfl, dim_x, dim_y, batch, large):
    """A batch against a twin of the other kind (61 x 81), or of its own (96 x 96 does not fit the small kind), after
    step_n_each(3) with forces: all counts zero.  Then one force more on the twin: the record is numpy's."""
    iters = [10, 20, 15]
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b, sfl.BatchSolver(dim_x, dim_y, batch, large=True) as twin:
        for x in (b, twin):
            x.setup_sketch_fields()
            x.queue_forces(*FORCES)
            x.queue_forces([1], [(7, 9)], [(5.0, -6.0)], step=2)
            x.step_n_each(3, 0.05, 1.0, iters, 1.9)
        got = b.distance(twin)
        for m in range(batch):
            assert {k: int(got[m][k]) for k in ZERO} == ZERO, f"member {m}"
            assert got[m]["max_abs_dvx"] == 0 and got[m]["max_abs_dp"] == 0 and not got[m]["sum_abs_ddye"].any()
        twin.queue_forces([1], [(30, 30)], [(40.0, 2.0)])
        for x in (b, twin):
            x.step_n_each(2, 0.05, 1.0, iters, 1.9)
        residual = b.residual()
        got = b.distance(twin)
        assert_bit_equal(b.residual(), residual, "residual() after distance()")
        fb, ft = [b.download(k) for k in (FV, FC, FP)], [twin.download(k) for k in (FV, FC, FP)]
        for m in range(batch):
            assert_distance(got[m], yardstick(member(fb, m), member(ft, m)), f"member {m} against its twin")
        assert got[1]["velocity_cells_differ"] > 0 and {k: int(got[0][k]) for k in ZERO} == ZERO
        with sfl.BatchSolver(dim_x, dim_y + 1, batch, large=True) as other:
            with pytest.raises(sfl.SflError, match="shapes must be the same"):
                b.distance(other)
        with sfl.BatchSolver(dim_x, dim_y, batch - 1, large=True) as few:
            with pytest.raises(sfl.SflError, match="pairwise"):
                b.distance(few)
            assert b.distance(few, count=batch - 1).shape == (batch - 1,)


# ---- the envelope -------------------------------------------------------------------------------------
def envelope_yardstick(c):
    """mean, min, max, spread over axis 0 of uint32[count, ...]."""
    lo, hi = c.min(axis=0), c.max(axis=0)
    mean = c.astype(np.uint64).sum(axis=0) // np.uint64(c.shape[0])
    assert mean.max() < 2 ** 32
    return [mean.astype(np.uint32), lo, hi, hi - lo]


def assert_envelope(sfl, b, c, first, count, what):
    assert b.envelope_info() == (first, count), what
    for which, want in enumerate(envelope_yardstick(c[first:first + count])):
        assert_bit_equal(b.envelope_field(which), want, f"{what}: field {which} of members [{first}, {first} + {count})")


@functools.lru_cache(maxsize=None)
def ensemble_dye(sfl, dim_x, dim_y, batch):
    """Random dye, with: cell 0 alternating between 0 and 2^32 - 1 from member to member (a 32-bit sum would wrap); cell 1 the
    same in every member; and single outliers -- a high one in channel 0 and a low one in channel 1 of a cell of its own --
    in the first and last member of the batch and of every member group."""
    group = sfl.ENV_GROUP_MEMBERS
    rng = np.random.default_rng(dim_x + batch)
    c = rng.integers(2 ** 20, 2 ** 31, (batch, dim_y, dim_x, 3), dtype=np.uint32)
    flat = c.reshape(batch, -1, 3)
    flat[0::2, 0, :], flat[1::2, 0, :] = 0, 0xFFFFFFFF
    flat[:, 1, :] = flat[0, 1, :]
    outliers = sorted({0, batch - 1} | {m for g in range(0, batch, group) for m in (g - 1, g) if 0 <= m < batch})
    for k, m in enumerate(outliers):
        flat[m, (2 + k) % flat.shape[1], 0], flat[m, (2 + k) % flat.shape[1], 1] = 0xFFFFFFF0 + k, k
    c.setflags(write=False)
    return c


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,batch,large", [(61, 81, 1, False), (61, 81, 2, False), (61, 81, 5, False), (8, 6, 37, False),
                                                     (61, 81, 70, False), (96, 96, 3, True)])
def test_the_envelope_is_numpys(sfl, dim_x, dim_y, batch, large):
    group = sfl.ENV_GROUP_MEMBERS
    assert group == 32 and (batch <= group or batch % group), "37 and 70: more than one group, no multiple of it"
    c = ensemble_dye(sfl, dim_x, dim_y, batch)
    tag = f"{dim_x} x {dim_y} x {batch}"
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        assert b.envelope_info() == (0, 0)
        with pytest.raises(sfl.SflError) as e:
            b.envelope_field(0)
        assert e.value.code == sfl.capi.ERR_STATE
        b.upload(FC, c)
        b.envelope()
        assert_envelope(sfl, b, c, 0, batch, tag)
        ranges = {(0, 1), (batch - 1, 1), (batch // 2, batch - batch // 2), (0, max(batch - 1, 1))}
        if batch > group:     # ranges that end and begin on both sides of a group boundary, and groups counted from `first`
            ranges |= {(0, group), (0, group + 1), (1, group), (1, group + 1), (group - 1, 2), (3, batch - 3)}
        for first, count in sorted(ranges):
            b.envelope(first, count)
            assert_envelope(sfl, b, c, first, count, tag)
        assert_bit_equal(b.download(FC), c, f"{tag}: the members' dye after envelope()")
        for bad in ((0, 0), (1, batch), (-1, 1)):
            with pytest.raises(sfl.SflError):
                b.envelope(*bad)
        assert b.envelope_info() == (first, count), "a refused call leaves the snapshot"


@pytest.mark.gpu
def test_equal_members_have_no_spread(sfl):
    dim_x, dim_y, batch = 61, 81, 40
    one = fields(dim_x, dim_y)[1]
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        for m in range(batch):
            b.upload(FC, one[None], m)
        b.envelope()
        assert not b.envelope_field(sfl.capi.ENV_SPREAD).any()
        for which in (sfl.capi.ENV_MEAN, sfl.capi.ENV_MIN, sfl.capi.ENV_MAX):
            assert_bit_equal(b.envelope_field(which), one, f"field {which} of {batch} equal members")


@pytest.mark.gpu
def test_the_envelopes_pictures_and_the_snapshot(sfl):
    """envelope_render is Solver.render_rgb565 of a context that got the downloaded field as its dye; the snapshot is kept
    through later steps and replaced by the next envelope()."""
    dim_x, dim_y, batch = 61, 81, 5
    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.Solver(dim_x, dim_y) as s:
        b.setup_sketch_fields()
        b.queue_forces(*FORCES)
        b.step_n_each(4, 0.05, 1.0, [5, 10, 20, 30, 40], 1.9)
        b.envelope(1, 4)
        c = b.download(FC)
        assert_envelope(sfl, b, c, 1, 4, "after four steps")
        kept = [b.envelope_field(which) for which in range(4)]
        assert kept[sfl.capi.ENV_SPREAD].any(), "the members must disagree somewhere"
        for which in range(4):
            s.upload(FC, kept[which])
            for scaling in (1, 4):
                for byteswap in (True, False):
                    img = b.envelope_render(which, scaling, byteswap)
                    assert img.shape == (scaling * (dim_x - 1), scaling * (dim_y - 1)) and img.dtype == np.uint16
                    assert np.array_equal(img, s.render_rgb565(scaling, byteswap)), f"field {which} at scaling {scaling}"
        b.queue_forces([3], [(30, 30)], [(20.0, 20.0)])
        b.step_n(2, 0.05, 1.0, 10, 1.9)
        assert not np.array_equal(b.download(FC), c), "the dye must have moved on"
        for which in range(4):
            assert_bit_equal(b.envelope_field(which), kept[which], f"field {which} after two more steps")
        assert b.envelope_info() == (1, 4)
        b.envelope()
        assert_envelope(sfl, b, b.download(FC), 0, batch, "the next envelope")
        lib, img = sfl.capi.lib(), np.zeros(4, np.uint16)
        assert lib.sfl_batch_envelope_render(b._h, 0, 1, 1, img.ctypes.data_as(C.POINTER(C.c_uint16)), 8) == sfl.capi.ERR_INVALID
        assert "9600 bytes" in lib.sfl_last_error().decode()
