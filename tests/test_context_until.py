"""Whole-domain contexts: the update norm of the pressure they hold (sfl_residual), a solve continued from that pressure
(sfl_poisson_continue) and a solve stopped at a tolerance (sfl_poisson_solve_until).

The contract under test is the batches' (include/sfl.h, sfl_batch_residual and sfl_member_stop), carried to contexts of any
size: residual() is, bit for bit, the numpy restatement `update_norm` of test_batch_params.py on the p and d a download
hands out; poisson_solve(a) + poisson_continue(b) leaves the reference's poisson_solve(a + b); poisson_solve_until stops at
the k the numpy `rule` of test_batch_until.py finds, leaves the reference's poisson_solve(k) and reports u_k.  Both yardsticks
are pinned against the oracle by CPU tests of their own files.  All comparisons are bit for bit; a NaN matches any NaN.

Shapes: the one-workgroup path (at most 6144 cells) and the general kernels; widths that are no multiple of 4 (rows that are
not 16-byte aligned), of 256 (a partly filled strip of the norm kernel) and beyond 256 (more than one strip); heights that
are no multiple of the norm kernel's 8-row tiles; two columns, three rows."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_batch_params import assert_report_equal, update_norm
from test_batch_until import classify, rule, sor_iteration, zero_mean

SYMBOLS = ["sfl_residual", "sfl_poisson_continue", "sfl_poisson_solve_until"]
SMALL_SHAPES = [(2, 2), (3, 3), (61, 81)]
GENERAL_SHAPES = [(130, 70), (96, 65), (257, 130), (512, 96), (1030, 67), (2, 4000), (3073, 3)]
ALL_SHAPES = SMALL_SHAPES + GENERAL_SHAPES
# option sets: name -> {option name: value}
AUTO, K1, K2F16 = {}, {"OPT_SOR_KERNEL": 1}, {"OPT_SOR_KERNEL": 2, "OPT_SOR_FUSE": 16}
KERNELS = {"auto": AUTO, "kernel1": K1, "kernel2-fuse2": {"OPT_SOR_KERNEL": 2, "OPT_SOR_FUSE": 2},
           "kernel2-fuse8": {"OPT_SOR_KERNEL": 2, "OPT_SOR_FUSE": 8}, "kernel2-fuse16": K2F16,
           "no-small-grid": {"OPT_SMALL_GRID": 0}}


def context(sfl, dim_x, dim_y, options=AUTO):
    s = sfl.Solver(dim_x, dim_y)
    for name, value in options.items():
        s.set_option(getattr(sfl.capi, name), value)
    return s


def fields(dim_x, dim_y, seed):
    """A random right-hand side and a random pressure that is no solve's output."""
    rng = np.random.default_rng(seed)
    return rng.standard_normal((dim_y, dim_x)).astype(np.float32), rng.standard_normal((dim_y, dim_x)).astype(np.float32)


def load(sfl, s, d, p=None):
    s.upload(sfl.capi.FIELD_DIVERGENCE, d)
    if p is not None:
        s.upload(sfl.capi.FIELD_PRESSURE, p)


@functools.lru_cache(maxsize=None)
def yardstick(dim_x, dim_y, cap, omega, tol, every):
    """The rule on zero_mean(dim_x, dim_y, 3 + dim_x), dx = 1: (d, k, p_k, u_k), evaluated once per parameter point."""
    d = zero_mean(dim_x, dim_y, 3 + dim_x)
    k, p, u = rule(d, 1.0, cap, omega, tol, every)
    return d, k, p, u


def assert_until(sfl, oracle, dim_x, dim_y, options, cap, omega, tol, every, want_k, want_class, what):
    d, k, p, u = yardstick(dim_x, dim_y, cap, omega, tol, every)
    assert classify(k, cap, u) == want_class and (want_k is None or k == want_k), (what, "the yardstick itself", k, u)
    with context(sfl, dim_x, dim_y, options) as s:
        load(sfl, s, d)
        got_k, got_u = s.poisson_solve_until(1.0, cap, omega, tol=tol, every=every)
        got_p = s.download(sfl.capi.FIELD_PRESSURE)
        info = s.last_solve_info()
    print(f"{what}: k {got_k} (want {k}), norm {got_u!r} (want {u!r}), launches {info['launches']}")
    assert got_k == k, (what, got_k, k)
    with np.errstate(all="ignore"):
        assert_bit_equal(got_p, oracle.poisson_solve(d, np.float32(1.0), k, np.float32(omega)), f"{what}: pressure at k = {k}")
    assert_report_equal(got_u, u, f"{what}: norm")
    assert_report_equal(got_u, update_norm(got_p, d, 1.0), f"{what}: norm of the pressure handed out")
    return k, info


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    for name in ("residual", "poisson_continue", "poisson_solve_until"):
        assert hasattr(sfl.Solver, name), name
    assert lib.sfl_abi_version() == 1


def test_a_null_context_is_refused_by_all_three(sfl):
    lib = sfl.capi.lib()
    u, k = C.c_float(), C.c_int32()
    for call in (lambda: lib.sfl_residual(None, 1.0, C.byref(u)),
                 lambda: lib.sfl_poisson_continue(None, 1.0, 3, 1.9),
                 lambda: lib.sfl_poisson_solve_until(None, 1.0, 10, 1.9, 1e-3, 8, C.byref(k), C.byref(u))):
        assert call() == sfl.capi.ERR_INVALID
        assert "NULL" in lib.sfl_last_error().decode()


def test_the_python_until_needs_a_tolerance(sfl):
    with pytest.raises(ValueError):
        sfl.Solver.poisson_solve_until(object(), 1.0, 10, 1.9)


# ---- GPU: what is refused -----------------------------------------------------------------------------
@pytest.mark.gpu
def test_bad_arguments_are_refused_and_leave_the_pressure_alone(sfl):
    d, p = fields(130, 70, 5)
    with context(sfl, 130, 70) as s:
        load(sfl, s, d, p)
        for call in (lambda: s.poisson_solve_until(1.0, 10, 1.9, tol=1e-3, every=0),
                     lambda: s.poisson_solve_until(1.0, 10, 1.9, tol=float("nan"), every=8),
                     lambda: s.poisson_solve_until(1.0, -1, 1.9, tol=1e-3, every=8),
                     lambda: s.poisson_continue(1.0, -1, 1.9)):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == sfl.capi.ERR_INVALID, str(e.value)
        assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), p, "pressure after refused calls")
        lib, k = sfl.capi.lib(), C.c_int32()       # either out pointer may be NULL
        assert lib.sfl_poisson_solve_until(s._h, 1.0, 4, 1.9, -1.0, 8, None, None) == sfl.capi.OK
        assert lib.sfl_poisson_solve_until(s._h, 1.0, 4, 1.9, -1.0, 8, C.byref(k), None) == sfl.capi.OK and k.value == 4


@pytest.mark.gpu
def test_slabs_are_refused_by_all_three(sfl):
    with sfl.Solver(130, 70, rank=0, nranks=2) as s:
        for call in (lambda: s.residual(1.0), lambda: s.poisson_continue(1.0, 3, 1.9),
                     lambda: s.poisson_solve_until(1.0, 10, 1.9, tol=1e-3, every=8)):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == sfl.capi.ERR_STATE, str(e.value)
            assert "whole-domain contexts only" in str(e.value)


# ---- GPU: the residual --------------------------------------------------------------------------------
def spike_cells(dim_x, dim_y):
    """The four corners, the middle of each edge, and an interior cell beside a boundary of the norm kernel's tiles: column
    256 (the first of the second strip) where the grid has one, row 8 (the first of the second 8-row tile)."""
    mx, my = dim_x // 2, dim_y // 2
    cells = [(0, 0), (dim_x - 1, 0), (0, dim_y - 1), (dim_x - 1, dim_y - 1), (mx, 0), (mx, dim_y - 1), (0, my), (dim_x - 1, my)]
    if dim_x > 2 and dim_y > 2:
        cells.append((256 if dim_x > 257 else mx if mx < dim_x - 1 else 1, 8 if dim_y > 9 else 1))
        cells.append((255 if dim_x > 257 else 1, 7 if dim_y > 9 else 1))
    return sorted(set(cells))


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", ALL_SHAPES)
def test_the_residual_is_numpys_update_norm_wherever_the_maximum_sits(sfl, dim_x, dim_y):
    d, p = fields(dim_x, dim_y, 11 + dim_x)
    with context(sfl, dim_x, dim_y) as s:
        load(sfl, s, d, p)
        for dx in (1.0, 0.5):
            assert_report_equal(s.residual(dx), update_norm(p, d, dx), f"{dim_x} x {dim_y}, dx {dx}")
        plain = update_norm(p, d, 1.0)
        for (i, j) in spike_cells(dim_x, dim_y):
            q = p.copy()
            q[j, i] = np.float32(1000.0)
            want = update_norm(q, d, 1.0)
            assert want > 100 * plain, "the spike must be what sets the maximum"
            s.upload(sfl.capi.FIELD_PRESSURE, q)
            assert_report_equal(s.residual(1.0), want, f"{dim_x} x {dim_y}, spike at ({i}, {j})")
        for value in (np.nan, np.inf, -np.inf):
            q = p.copy()
            q[dim_y // 2, dim_x // 3] = np.float32(value)
            s.upload(sfl.capi.FIELD_PRESSURE, q)
            assert_report_equal(s.residual(1.0), update_norm(q, d, 1.0), f"{dim_x} x {dim_y}, one {value}")
        assert np.isnan(update_norm(q, d, 1.0)) or np.isinf(update_norm(q, d, 1.0))
        s.upload(sfl.capi.FIELD_PRESSURE, p)                  # the call reads, it never writes
        s.residual(1.0)
        assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), p, "pressure after residual()")
        assert_bit_equal(s.download(sfl.capi.FIELD_DIVERGENCE), d, "divergence after residual()")


@pytest.mark.gpu
def test_the_residual_of_61_x_81_without_the_small_grid_path(sfl):
    d, p = fields(61, 81, 72)
    with context(sfl, 61, 81, KERNELS["no-small-grid"]) as s:
        load(sfl, s, d, p)
        assert_report_equal(s.residual(0.5), update_norm(p, d, 0.5), "61 x 81, small grid off")


@pytest.mark.gpu
def test_the_residual_of_seventeen_million_cells(sfl):
    """4099 x 4100: more than 2^24 cells, more tiles than the capped grid has waves (the waves stride), rows that are not
    16-byte aligned.  One numpy evaluation; the spike sits in the last tile handed out."""
    dim_x, dim_y = 4099, 4100
    d, p = fields(dim_x, dim_y, 4099)
    p[dim_y - 2, dim_x - 3] = np.float32(50.0)
    with context(sfl, dim_x, dim_y) as s:
        load(sfl, s, d, p)
        got = s.residual(1.0)
    want = update_norm(p, d, 1.0)
    assert want > 10
    assert_report_equal(got, want, "4099 x 4100")


# ---- GPU: continue ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["kernel1", "kernel2-fuse2", "kernel2-fuse8", "kernel2-fuse16"])
@pytest.mark.parametrize("dim_x,dim_y", GENERAL_SHAPES)
def test_solve_7_then_continue_5_is_the_oracles_solve_12(sfl, oracle, dim_x, dim_y, kernel):
    d, _ = fields(dim_x, dim_y, 21 + dim_x)
    dx, omega = np.float32(0.5), np.float32(1.9)
    with context(sfl, dim_x, dim_y, KERNELS[kernel]) as s:
        load(sfl, s, d)
        s.poisson_solve(dx, 7, omega)
        s.poisson_continue(dx, 5, omega)
        got = s.download(sfl.capi.FIELD_PRESSURE)
    assert_bit_equal(got, oracle.poisson_solve(d, dx, 12, omega), f"{dim_x} x {dim_y}, {kernel}: 7 + 5 iterations")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,kernel", [(x, y, "auto") for x, y in SMALL_SHAPES] + [(61, 81, "no-small-grid")])
def test_solve_7_then_continue_5_on_the_small_shapes(sfl, oracle, dim_x, dim_y, kernel):
    d, _ = fields(dim_x, dim_y, 21 + dim_x)
    dx, omega = np.float32(1.0), np.float32(1.96)
    with context(sfl, dim_x, dim_y, KERNELS[kernel]) as s:
        load(sfl, s, d)
        s.poisson_solve(dx, 7, omega)
        s.poisson_continue(dx, 5, omega)
        got = s.download(sfl.capi.FIELD_PRESSURE)
        launches = s.last_solve_info()["launches"]
    assert_bit_equal(got, oracle.poisson_solve(d, dx, 12, omega), f"{dim_x} x {dim_y}, {kernel}: 7 + 5 iterations")
    if kernel == "auto":
        assert launches == 1, "the small-grid path continues in one launch"


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,kernel", [(61, 81, "auto"), (3, 3, "auto"), (130, 70, "auto"), (130, 70, "kernel1"),
                                                (257, 130, "kernel2-fuse16"), (1030, 67, "kernel2-fuse8"), (2, 4000, "auto")])
def test_continue_iterates_from_an_uploaded_pressure_and_zero_iterations_touch_nothing(sfl, dim_x, dim_y, kernel):
    d, p = fields(dim_x, dim_y, 31 + dim_x)
    dx, omega = 0.5, 1.5
    with context(sfl, dim_x, dim_y, KERNELS[kernel]) as s:
        load(sfl, s, d, p)
        s.poisson_continue(dx, 0, omega)
        assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), p, f"{dim_x} x {dim_y}, {kernel}: zero iterations")
        s.poisson_continue(dx, 3, omega)
        got = s.download(sfl.capi.FIELD_PRESSURE)
    want = p
    for _ in range(3):
        want = sor_iteration(want, d, dx, omega)
    assert_bit_equal(got, want, f"{dim_x} x {dim_y}, {kernel}: three iterations from a random pressure")


# ---- GPU: until ---------------------------------------------------------------------------------------
EARLY = [  # dim_x, dim_y, omega, tol, every, cap, k
    (130, 70, 1.9, 1e-2, 8, 400, 128), (130, 70, 1.9, 1e-3, 5, 400, 215), (130, 70, 1.9, 0.1, 3, 200, 48),
    (96, 65, 1.9, 1e-2, 8, 400, 88), (61, 81, 1.9, 1e-2, 8, 400, 96), (61, 81, 1.96, 1e-2, 1, 400, 128),
    (257, 130, 1.9, 0.5, 8, 120, 24), (257, 130, 1.9, 0.1, 3, 200, 63), (512, 96, 1.7, 0.2, 5, 120, 20)]


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["auto", "kernel1", "kernel2-fuse16"])
@pytest.mark.parametrize("dim_x,dim_y,omega,tol,every,cap,k", EARLY)
def test_a_solve_that_stops_early_stops_where_the_rule_stops(sfl, oracle, dim_x, dim_y, omega, tol, every, cap, k, kernel):
    what = f"{dim_x} x {dim_y}, omega {omega}, tol {tol}, every {every}, cap {cap}, {kernel}"
    k, info = assert_until(sfl, oracle, dim_x, dim_y, KERNELS[kernel], cap, omega, tol, every, k, "early", what)
    # the SOR launches of all segments, the norm launches not among them
    if kernel == "kernel1":
        assert info["launches"] == 2 * k, (what, info)
    if kernel == "kernel2-fuse16" and every == 8:
        assert info["launches"] == k // 8, (what, info)
    if kernel == "auto" and (dim_x, dim_y) == (61, 81):
        assert info["launches"] == 1, (what, info)


@pytest.mark.gpu
def test_61_x_81_stops_early_without_the_small_grid_path(sfl, oracle):
    assert_until(sfl, oracle, 61, 81, KERNELS["no-small-grid"], 400, 1.9, 1e-2, 8, 96, "early", "61 x 81, small grid off")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", ALL_SHAPES)
def test_plain_gauss_seidel_runs_to_its_cap(sfl, oracle, dim_x, dim_y):
    """omega = 1, tol 1e-3, every 8, cap 48: every shape of more than a handful of cells is still far from 1e-3 at the cap.
    The two tiny shapes are not: by the yardstick 2 x 2 and 3 x 3 have converged at the check in front of iteration 8 (u_8 =
    0 and 5.5e-5), so for them the same parameters are one more early stop."""
    want_k, want_class = (8, "early") if dim_x * dim_y <= 9 else (48, "cap")
    assert_until(sfl, oracle, dim_x, dim_y, AUTO, 48, 1.0, 1e-3, 8, want_k, want_class, f"{dim_x} x {dim_y}, omega 1, cap 48")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(2, 4000), (3073, 3)])
def test_the_thin_shapes_run_to_their_cap(sfl, oracle, dim_x, dim_y):
    assert_until(sfl, oracle, dim_x, dim_y, AUTO, 120, 1.9, 0.5, 8, 120, "cap", f"{dim_x} x {dim_y}, cap 120")


@pytest.mark.gpu
@pytest.mark.parametrize("kernel", ["auto", "kernel1", "kernel2-fuse16"])
def test_a_diverging_solve_stops_at_its_first_nan_checkpoint(sfl, oracle, kernel):
    assert_until(sfl, oracle, 130, 70, KERNELS[kernel], 400, 2.5, 1e-3, 8, 112, "nan", f"130 x 70, omega 2.5, {kernel}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,kernel", [(61, 81, "auto"), (130, 70, "auto"), (130, 70, "kernel1"), (257, 130, "kernel2-fuse16")])
def test_the_corners_of_the_rule(sfl, oracle, dim_x, dim_y, kernel):
    opts, what = KERNELS[kernel], f"{dim_x} x {dim_y}, {kernel}"
    d = zero_mean(dim_x, dim_y, 3 + dim_x)
    _, junk = fields(dim_x, dim_y, 9)
    # tol = +inf stops at k = 0 and leaves p = 0, whatever the context held; so does a cap of 0
    for cap, tol in ((40, np.inf), (0, 1e-2), (0, -1.0)):
        with context(sfl, dim_x, dim_y, opts) as s:
            load(sfl, s, d, junk)
            k, u = s.poisson_solve_until(1.0, cap, 1.9, tol=tol, every=8)
            assert k == 0, (what, cap, tol, k)
            assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), np.zeros_like(d), f"{what}: cap {cap}, tol {tol}")
            assert_report_equal(u, update_norm(np.zeros_like(d), d, 1.0), f"{what}: u_0")
    # tol = -1: poisson_solve(cap), count = cap, the norm reported -- also at a cap that is no multiple of `every`
    with context(sfl, dim_x, dim_y, opts) as s:
        load(sfl, s, d, junk)
        k, u = s.poisson_solve_until(1.0, 37, 1.9, tol=-1.0, every=8)
        got = s.download(sfl.capi.FIELD_PRESSURE)
        assert k == 37
        assert_bit_equal(got, oracle.poisson_solve(d, np.float32(1.0), 37, np.float32(1.9)), f"{what}: tol -1")
        assert_report_equal(u, update_norm(got, d, 1.0), f"{what}: tol -1, norm")
        s.poisson_solve(1.0, 37, 1.9)
        assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), got, f"{what}: tol -1 is poisson_solve")
    # a cap that is no multiple of `every`, reached: the last segment is shortened
    assert_until(sfl, oracle, dim_x, dim_y, opts, 43, 1.9, 1e-6, 8, 43, "cap", f"{what}: cap 43, every 8")
    # ... and a stop at the last checkpoint below such a cap
    _, k2, _, _ = yardstick(dim_x, dim_y, 400, 1.9, 0.5, 8)
    assert_until(sfl, oracle, dim_x, dim_y, opts, k2 + 3, 1.9, 0.5, 8, k2, "early", f"{what}: cap {k2 + 3}, stops at {k2}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,kernel", [(130, 70, "auto"), (257, 130, "kernel2-fuse16")])
def test_with_the_folded_quarter_the_until_is_the_contexts_own_solve(sfl, dim_x, dim_y, kernel):
    d = zero_mean(dim_x, dim_y, 3 + dim_x)
    with context(sfl, dim_x, dim_y, dict(KERNELS[kernel], OPT_SOR_FOLD=1)) as s:
        load(sfl, s, d)
        k, u = s.poisson_solve_until(1.0, 200, 1.9, tol=0.1, every=3)
        got = s.download(sfl.capi.FIELD_PRESSURE)
        assert 0 < k < 200 and k % 3 == 0, k
        assert_report_equal(u, update_norm(got, d, 1.0), "folded: norm of the pressure handed out")
        s.poisson_solve(1.0, k, 1.9)
        assert_bit_equal(got, s.download(sfl.capi.FIELD_PRESSURE), f"{dim_x} x {dim_y}, {kernel}, folded: until vs solve({k})")


@pytest.mark.gpu
def test_a_batch_of_one_and_a_context_agree(sfl):
    dim_x, dim_y, cap, omega, tol, every = 61, 81, 400, 1.9, 1e-2, 8
    d = zero_mean(dim_x, dim_y, 3 + dim_x)
    with sfl.BatchSolver(dim_x, dim_y, 1) as b:
        b.upload(sfl.capi.FIELD_DIVERGENCE, d[None])
        b.poisson_solve_until(1.0, cap, omega, tol=tol, every=every)
        bp, bu, bk = b.download(sfl.capi.FIELD_PRESSURE)[0], b.residual()[0], int(b.iterations()[0, 0])
    for kernel in ("auto", "no-small-grid"):
        with context(sfl, dim_x, dim_y, KERNELS[kernel]) as s:
            load(sfl, s, d)
            k, u = s.poisson_solve_until(1.0, cap, omega, tol=tol, every=every)
            assert k == bk and 0 < k < cap, (kernel, k, bk)
            assert_bit_equal(s.download(sfl.capi.FIELD_PRESSURE), bp, f"context ({kernel}) vs batch of one: pressure")
            assert_report_equal(u, bu, f"context ({kernel}) vs batch of one: norm")
            assert_report_equal(s.residual(1.0), bu, f"context ({kernel}): residual() after the until")
