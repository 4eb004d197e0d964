"""The fused SOR kernel after its interior trip went on a diet (profiles/sor_trip_diet.txt): the priority turn is picked by two bit
tests inside one asm statement, and the relaxation's product by omega passes through an empty asm statement that keeps it a plain
multiplication (Lane2::scalar_only).  Neither touches the arithmetic, so every solve here is compared with the oracle BIT FOR BIT,
on the smallest shapes at which every path of the kernel runs:

  416 x 640, 418 x 300   even width: 8-byte accesses, five strips of which three are inner ones (interior tiles in both stream
                         directions need r0 - NS - RING > 0 and r1 + NS + RING < dim_y: RING = 18 at NS = 16, 12 at NS = 10)
  417 x 640              odd width: 4-byte accesses
  rows per tile 40, 23   several chunks per strip, both stream directions, and a last, partial trip of every length class
                         (40 + 32 and 23 + 32 input rows are no multiples of 18; 23 + 20 and 40 + 20 none of 12)
  iters 8 / 24           one launch from zero / three launches at NS = 16 (from zero, then both sweep directions); 2 / 5 at NS = 10
  dx 1 / 0.5, exact and folded arithmetic: the four instantiations of the relaxation
  two virtual ranks      lrows < dim_y and ghost rows: clamped loads beside the cuts

The shapes were chosen for a larger change (row offsets by cursors, stores dropped by the buffer's range check: both measured and
removed again, see the note); what they guard in the tree as it stands is relax() and next_turn() on every path, as regression tests.
"""
import numpy as np
import pytest

from conftest import assert_bit_equal

pytestmark = pytest.mark.gpu

OMEGA = np.float32(1.96)
SHAPES = [(416, 640), (418, 300), (417, 640)]
_RHS, _WANT = {}, {}


def rhs(kind, dim_x, dim_y):
    """dense: a Gaussian sample; sparse: three touch dipoles on an exact zero (the sketch's own start)."""
    key = (kind, dim_x, dim_y)
    if key not in _RHS:
        if kind == "dense":
            d = np.random.default_rng(dim_x * 1000 + dim_y).standard_normal((dim_y, dim_x)).astype(np.float32)
        else:
            d = np.zeros((dim_y, dim_x), np.float32)
            for fx, fy in ((0.5, 0.5), (0.12, 0.8), (0.9, 0.07)):
                i, j = int(dim_x * fx), int(dim_y * fy)
                d[j, i - 1] += np.float32(10.0)
                d[j, i + 1] -= np.float32(10.0)
                d[j - 1, i] += np.float32(5.0)
                d[j + 1, i] -= np.float32(5.0)
        d.setflags(write=False)
        _RHS[key] = d
    return _RHS[key]


def want(oracle, kind, dim_x, dim_y, dx, iters):
    """One oracle solve per (right-hand side, dx, iters), shared by every configuration that must reproduce it."""
    key = (kind, dim_x, dim_y, dx, iters)
    if key not in _WANT:
        w = oracle.poisson_solve(rhs(kind, dim_x, dim_y), dx, iters, OMEGA)
        w.setflags(write=False)
        _WANT[key] = w
    return _WANT[key]


@pytest.mark.parametrize("fuse", [16, 10])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_dense_right_hand_side_bit_exact(sfl, oracle, dim_x, dim_y, fuse):
    d = rhs("dense", dim_x, dim_y)
    for rows in (40, 23):
        for iters in (8, 24):
            for dx in (1.0, 0.5):
                for fold in (0, 1):
                    hp = sfl.HostPath(sor_kernel=2, sor_fuse=fuse, sor_rows=rows, sor_fold=fold)
                    assert_bit_equal(hp.poisson_solve(d, dx, iters, OMEGA), want(oracle, "dense", dim_x, dim_y, dx, iters),
                                     f"{dim_x}x{dim_y} fuse {fuse} rows {rows} iters {iters} dx {dx} fold {fold}")


@pytest.mark.parametrize("fuse", [16, 10])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_sparse_right_hand_side_bit_exact(sfl, oracle, dim_x, dim_y, fuse):
    """Three dipoles on zero: most tiles relax exact zeros, signed ones included, through the same products.  (24 iterations:
    the solution's front is still far above the denormals, where the folded product is the reference's bits too --
    sor_stream_core.h relax.)"""
    d = rhs("sparse", dim_x, dim_y)
    for rows in (40, 23):
        for iters in (8, 24):
            for dx in (1.0, 0.5):
                for fold in (0, 1):
                    hp = sfl.HostPath(sor_kernel=2, sor_fuse=fuse, sor_rows=rows, sor_fold=fold)
                    assert_bit_equal(hp.poisson_solve(d, dx, iters, OMEGA), want(oracle, "sparse", dim_x, dim_y, dx, iters),
                                     f"{dim_x}x{dim_y} fuse {fuse} rows {rows} iters {iters} dx {dx} fold {fold}")


@pytest.mark.parametrize("fuse,halo", [(16, 32), (10, 20)])
def test_two_virtual_ranks_bit_exact(sfl, oracle, fuse, halo):
    """416 x 640 as two slabs of 320 rows + `halo` ghost rows: supersteps of two launches, cut-adjacent tiles that read clamped
    rows beyond the local arrays."""
    dim_x, dim_y, iters = 416, 640, 24
    d = rhs("dense", dim_x, dim_y)
    for rows in (40, 23):
        slabs = [sfl.Solver(dim_x, dim_y, 0, r, 2) for r in range(2)]
        try:
            sfl.Solver.link_group(slabs)
            for s in slabs:
                s.set_option(sfl.capi.OPT_SOR_KERNEL, 2)
                s.set_option(sfl.capi.OPT_SOR_FUSE, fuse)
                s.set_option(sfl.capi.OPT_SOR_HALO, halo)
                s.set_option(sfl.capi.OPT_SOR_ROWS, rows)
                s.upload(sfl.capi.FIELD_DIVERGENCE, d[s.row_begin:s.row_end])
            slabs[0].poisson_solve(1.0, iters, OMEGA)
            slabs[0].synchronize()
            info = slabs[0].last_solve_info()
            got = np.concatenate([s.download(sfl.capi.FIELD_PRESSURE) for s in slabs], axis=0)
        finally:
            for s in slabs:
                s.close()
        assert info["fuse"] == fuse and info["halo"] == halo, info
        assert_bit_equal(got, want(oracle, "dense", dim_x, dim_y, 1.0, iters), f"two slabs, fuse {fuse} halo {halo} rows {rows}")
