"""Every kernel that multiplies by the grid spacing, at spacings where none of its products is exact (tests/dx_cases.py).

Three products depend on dx: the right-hand side dx * d of every relaxation and update norm (poisson.cpp:89,109), the
reciprocal 1 / (2 dx) formed on the host, and the scaled differences flow_sum * two_dx_inv, u - (pe - pw) * two_dx_inv
(finitediff.cpp:22,30,56,70).  With a power-of-two dx all three are exact, and a fused multiply-add, a division by 2 dx or a
hoisted factor leave the reference's bits; at the spacings used here each of them changes a few per cent of the cells after
one operator.  So each family below takes one kind of kernel through its dx-dependent sites at the smallest shapes that
reach every path of it, bit for bit against the oracle (which tests/test_oracle_vs_reference.py and the dxn_ fixtures pin
to the reference at the same spacings) or against the numpy yardsticks of test_batch_params.py / test_batch_until.py.
"""
import os
import struct
import subprocess

import numpy as np
import pytest

import test_batch_params as bp
from conftest import ROOT, assert_bit_equal, random_fields
from dx_cases import DX_A, DX_B, DX_C, DX_CASES, dx_id
from test_batch_params import FIELDS, assert_report_equal, update_norm
from test_batch_until import classify, rule, yardstick_step, zero_mean
from test_flow_stats import assert_stats
from test_flow_stats import yardstick as stats_yardstick
from test_force_timeline import oracle_steps
from test_gpu_parity import _smooth_velocity

pytestmark = pytest.mark.gpu

DT = np.float32(1 / 30.0)
OMEGA = np.float32(1.96)
F = (0, 2, 3, 1)   # velocity, divergence, pressure, colour: the order of FIELDS


def context(sfl, dim_x, dim_y, **options):
    s = sfl.Solver(dim_x, dim_y)
    for name, value in options.items():
        s.set_option(getattr(sfl.capi, name), value)
    return s


def solve(sfl, s, d, dx, iters, omega=OMEGA):
    s.upload(sfl.capi.FIELD_DIVERGENCE, d)
    s.poisson_solve(dx, iters, omega)
    s.synchronize()
    return s.download(sfl.capi.FIELD_PRESSURE)


def step_fields(sfl, s, v, c, call):
    s.upload(sfl.capi.FIELD_VELOCITY, v)
    s.upload(sfl.capi.FIELD_COLOR, c)
    call(s)
    s.synchronize()
    return [s.download(f) for f in F]


def assert_fields(got, want, what):
    for name, a, b in zip(FIELDS, got, want):
        assert_bit_equal(a, b, f"{what}: {name}")


# ---- SOR, one pass per launch (stencil_kernels.hip: -0.25f * (dx * d - sum) inside, k * (dx * d - sum) at the walls) ------
@pytest.mark.parametrize("dx", DX_CASES, ids=dx_id)
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (33, 17), (130, 70)])
def test_sor_one_pass_per_launch(sfl, oracle, dim_x, dim_y, dx):
    _, _, d = random_fields(dim_x, dim_y, 300 + dim_x)
    with context(sfl, dim_x, dim_y, OPT_SOR_KERNEL=1, OPT_SMALL_GRID=0) as s:
        assert s.get_option(sfl.capi.OPT_SOR_KERNEL) == 1 and s.get_option(sfl.capi.OPT_SMALL_GRID) == 0
        got = solve(sfl, s, d, dx, 5)
    assert_bit_equal(got, oracle.poisson_solve(d, dx, 5, OMEGA), f"{dim_x} x {dim_y}, dx {dx!r}")


# ---- SOR, the fused kernel: edge tiles (4 x 5), flipped tiles, the k * (...) wall path, both arithmetic parts ------------
@pytest.mark.parametrize("fold", [0, 1])
@pytest.mark.parametrize("fuse", [2, 8, 16])
@pytest.mark.parametrize("dim_x,dim_y", [(4, 5), (127, 33), (300, 41), (512, 96)])
def test_sor_fused(sfl, oracle, dim_x, dim_y, fuse, fold):
    """fold = 1 multiplies once by -0.25f * omega; on a dense Gaussian right-hand side no quarter underflows, so it leaves
    the reference's bits too (test_folded_quarter_omega_at_the_edges_of_float asserts the same for dense fields)."""
    _, _, d = random_fields(dim_x, dim_y, 400 + dim_x + fuse)
    iters = fuse + fuse // 2
    with context(sfl, dim_x, dim_y, OPT_SOR_KERNEL=2, OPT_SOR_FUSE=fuse, OPT_SOR_FOLD=fold) as s:
        for dx in DX_CASES:
            got = solve(sfl, s, d, dx, iters)
            assert_bit_equal(got, oracle.poisson_solve(d, dx, iters, OMEGA), f"{dim_x} x {dim_y}, fuse {fuse}, fold {fold}, dx {dx!r}")


# ---- the small grid in one launch (small_grid_core.h: dx * d kept per thread, and its update norm) -------------------------
SMALL = [(2, 2), (61, 81), (3, 2048), (128, 48)]     # 3 x 2048: 6144 cells, but too many of one colour per thread -- the general kernels


def one_workgroup(dim_x, dim_y):
    return dim_x * dim_y <= 6144 and dim_y * ((dim_x + 1) // 2) <= 3072


@pytest.mark.parametrize("dx", [DX_A, DX_B], ids=dx_id)
@pytest.mark.parametrize("dim_x,dim_y", SMALL)
def test_small_grid_solve_step_and_residual(sfl, oracle, dim_x, dim_y, dx):
    v, c, d = random_fields(dim_x, dim_y, 500 + dim_x, 90.0)
    with context(sfl, dim_x, dim_y) as s:
        assert s.get_option(sfl.capi.OPT_SMALL_GRID) == 1
        got = solve(sfl, s, d, dx, 9)
        assert (s.last_solve_info()["launches"] == 1) == one_workgroup(dim_x, dim_y)
        assert_bit_equal(got, oracle.poisson_solve(d, dx, 9, OMEGA), f"solve, dx {dx!r}")
        assert_report_equal(s.residual(dx), update_norm(got, d, dx), f"update norm of the solve, dx {dx!r}")
        got = step_fields(sfl, s, v, c, lambda s: s.step(DT, dx, 5, OMEGA))
        assert_fields(got, oracle.step(v, c, DT, dx, 5, OMEGA), f"step, dx {dx!r}")
        assert_report_equal(s.residual(dx), update_norm(got[2], got[1], dx), f"update norm of the step, dx {dx!r}")


def assert_until(sfl, oracle, s, d, dx, cap, omega, tol, every, what):
    """poisson_solve_until by the rule of test_context_until.py: the k the numpy rule finds, the oracle's pressure of k
    iterations, the rule's norm, which is also numpy's update norm of the pressure handed out."""
    k, _, u = rule(d, dx, cap, omega, tol, every)
    s.upload(sfl.capi.FIELD_DIVERGENCE, d)
    got_k, got_u = s.poisson_solve_until(dx, cap, omega, tol=tol, every=every)
    got_p = s.download(sfl.capi.FIELD_PRESSURE)
    print(f"{what}: k {got_k} (want {k}, {classify(k, cap, u)}), norm {got_u!r} (want {u!r})")
    assert got_k == k, (what, got_k, k)
    assert_bit_equal(got_p, oracle.poisson_solve(d, dx, k, np.float32(omega)), f"{what}: pressure at k = {k}")
    assert_report_equal(got_u, u, f"{what}: norm")
    assert_report_equal(got_u, update_norm(got_p, d, dx), f"{what}: norm of the pressure handed out")
    return k


@pytest.mark.parametrize("dim_x,dim_y", SMALL)
def test_small_grid_solve_until(sfl, oracle, dim_x, dim_y):
    d = zero_mean(dim_x, dim_y, 510 + dim_x)
    with context(sfl, dim_x, dim_y) as s:
        k = assert_until(sfl, oracle, s, d, DX_A, 64, 1.9, 0.05, 4, f"{dim_x} x {dim_y}, dx 0.37")
    if (dim_x, dim_y) in ((2, 2), (61, 81)):
        assert 0 < k < 64, "these two stop early on the yardstick: the stop is decided by a norm of an inexact dx * d"


# ---- the streaming update norm of the general contexts (update_norm.hip) ----------------------------------------------------
@pytest.mark.parametrize("dx", [DX_A, DX_C], ids=dx_id)
@pytest.mark.parametrize("dim_x,dim_y", [(130, 70), (300, 141)])
def test_streaming_update_norm_continue_and_until(sfl, oracle, dim_x, dim_y, dx):
    assert dim_x * dim_y > 6144
    rng = np.random.default_rng(600 + dim_x)
    d, p = (rng.standard_normal((dim_y, dim_x)).astype(np.float32) for _ in range(2))
    with context(sfl, dim_x, dim_y) as s:
        s.upload(sfl.capi.FIELD_DIVERGENCE, d)
        s.upload(sfl.capi.FIELD_PRESSURE, p)
        assert_report_equal(s.residual(dx), update_norm(p, d, dx), f"a random pressure, dx {dx!r}")
        s.poisson_solve(dx, 7, OMEGA)
        s.poisson_continue(dx, 5, OMEGA)
        got = s.download(sfl.capi.FIELD_PRESSURE)
        assert_bit_equal(got, oracle.poisson_solve(d, dx, 12, OMEGA), f"7 + 5 iterations, dx {dx!r}")
        assert_report_equal(s.residual(dx), update_norm(got, d, dx), f"after 12 iterations, dx {dx!r}")
        assert_until(sfl, oracle, s, zero_mean(dim_x, dim_y, 610 + dim_x), dx, 40, 1.9, 0.2, 8, f"{dim_x} x {dim_y}, dx {dx!r}")


# ---- the step kernels of a context -------------------------------------------------------------------------------------------
STEP_SHAPES = [(130, 70), (160, 128)]      # below and above kAdvectTiledMinCells (16384 cells)


def step_inputs(dim_x, dim_y):
    _, c, _ = random_fields(dim_x, dim_y, 700 + dim_x)
    return c, [("noise", random_fields(dim_x, dim_y, 701 + dim_x, 100.0)[0]), ("smooth", _smooth_velocity(dim_x, dim_y, 110.0))]


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("dim_x,dim_y", STEP_SHAPES)
def test_one_step_under_every_fusion(sfl, oracle, dim_x, dim_y, kernel):
    c, fields = step_inputs(dim_x, dim_y)
    with context(sfl, dim_x, dim_y, OPT_ADVECT_KERNEL=kernel) as s:
        for dx in (DX_A, DX_C):
            for name, v in fields:
                want = oracle.step(v, c, DT, dx, 3, OMEGA)
                for projection in (0, 1):
                    for divergence in (0, 1):
                        s.set_option(sfl.capi.OPT_FUSE_PROJECTION, projection)
                        s.set_option(sfl.capi.OPT_FUSE_DIVERGENCE, divergence)
                        got = step_fields(sfl, s, v, c, lambda s: s.step(DT, dx, 3, OMEGA))
                        assert_fields(got, want, f"{name}, dx {dx!r}, fused projection {projection}, fused divergence {divergence}")


@pytest.mark.parametrize("seams", [1, 0])
@pytest.mark.parametrize("dx", [DX_A, DX_C], ids=dx_id)
@pytest.mark.parametrize("dim_x,dim_y", STEP_SHAPES)
def test_three_steps_in_one_call(sfl, oracle, dim_x, dim_y, dx, seams):
    """step_n joins its steps by the seam kernel (advect_seam.h), which projects and differences on its own."""
    c, fields = step_inputs(dim_x, dim_y)
    with context(sfl, dim_x, dim_y, OPT_STEP_SEAMS=seams) as s:
        for name, v in fields:
            got = step_fields(sfl, s, v, c, lambda s: s.step_n(3, DT, dx, 3, OMEGA))
            want = (v, None, None, c)
            for _ in range(3):
                want = oracle.step(want[0], want[3], DT, dx, 3, OMEGA)
            assert_fields(got, want, f"{name}, dx {dx!r}, seams {seams}")


@pytest.mark.parametrize("kernel", [1, 2])
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (61, 81), (160, 128)])
def test_divergence_and_gradient_alone(sfl, oracle, dim_x, dim_y, kernel):
    v, _, p = random_fields(dim_x, dim_y, 800 + dim_x, 100.0)
    with context(sfl, dim_x, dim_y, OPT_ADVECT_KERNEL=kernel) as s:
        for dx in DX_CASES:
            s.upload(sfl.capi.FIELD_VELOCITY, v)
            s.upload(sfl.capi.FIELD_PRESSURE, p)
            s.calculate_divergence(dx)
            s.subtract_gradient(dx)
            s.synchronize()
            assert_bit_equal(s.download(sfl.capi.FIELD_DIVERGENCE), oracle.divergence(v, dx), f"divergence, dx {dx!r}")
            assert_bit_equal(s.download(sfl.capi.FIELD_VELOCITY), oracle.subtract_gradient(v, p, dx), f"gradient, dx {dx!r}")


# ---- virtual slabs -----------------------------------------------------------------------------------------------------------
def slab_group(sfl, dim_x, dim_y, nranks, **options):
    slabs = [sfl.Solver(dim_x, dim_y, 0, r, nranks) for r in range(nranks)]
    sfl.Solver.link_group(slabs)
    for s in slabs:
        for name, value in options.items():
            s.set_option(getattr(sfl.capi, name), value)
    return slabs


def slab_io(slabs):
    def upload(field, a):
        for s in slabs:
            s.upload(field, a[s.row_begin:s.row_end])
    return upload, lambda f: np.concatenate([s.download(f) for s in slabs], axis=0)


@pytest.mark.parametrize("nranks", [2, 3])
def test_slabs_step_and_solve(sfl, oracle, nranks):
    dim_x, dim_y = 200, 131
    v, c, d = random_fields(dim_x, dim_y, 900 + nranks, 60.0)
    slabs = slab_group(sfl, dim_x, dim_y, nranks, OPT_SOR_FUSE=8, OPT_SOR_HALO=0)
    try:
        upload, cat = slab_io(slabs)
        upload(sfl.capi.FIELD_VELOCITY, v)
        upload(sfl.capi.FIELD_COLOR, c)
        slabs[0].step(DT, DX_A, 4, OMEGA)
        slabs[0].synchronize()
        assert_fields([cat(f) for f in F], oracle.step(v, c, DT, DX_A, 4, OMEGA), f"{nranks} slabs: step at dx 0.37")
        upload(sfl.capi.FIELD_DIVERGENCE, d)
        slabs[0].poisson_solve(DX_B, 9, OMEGA)
        slabs[0].synchronize()
        assert_bit_equal(cat(sfl.capi.FIELD_PRESSURE), oracle.poisson_solve(d, DX_B, 9, OMEGA), f"{nranks} slabs: solve at dx 1.37")
    finally:
        for s in slabs:
            s.close()


def test_slabs_with_a_deep_halo(sfl, oracle):
    """test_virtual_slabs_match_single_context's (kernel 2, fuse 8, halo 32) on three ranks, at dx = 0.37."""
    dim_x, dim_y, iters, nranks = 96, 160, 7, 3
    v, c, _ = random_fields(dim_x, dim_y, 21, 60.0)
    slabs = slab_group(sfl, dim_x, dim_y, nranks, OPT_SOR_KERNEL=2, OPT_SOR_FUSE=8, OPT_SOR_HALO=32)
    try:
        upload, cat = slab_io(slabs)
        upload(sfl.capi.FIELD_VELOCITY, v)
        upload(sfl.capi.FIELD_COLOR, c)
        slabs[0].step(DT, DX_A, iters, OMEGA)
        slabs[0].synchronize()
        got = [cat(f) for f in F]
    finally:
        for s in slabs:
            s.close()
    assert_fields(got, oracle.step(v, c, DT, DX_A, iters, OMEGA), "three slabs, halo 32, dx 0.37")


# ---- batches (batch_grid.hip, batch_large.hip, batch_play.hip) ---------------------------------------------------------------
BATCHES = [pytest.param(61, 81, 5, False, id="61x81x5"), pytest.param(96, 96, 3, True, id="96x96x3-large")]


def batch_params(sfl, batch, seed, shift=0, iters=None):
    """dt, iters and omega as test_batch_params.py draws them; member m's dx is spacing (m + shift) mod 5."""
    prm = bp.draw_params(sfl, batch, seed)
    prm["dx"] = [DX_CASES[(m + shift) % len(DX_CASES)] for m in range(batch)]
    if iters is not None:
        prm["iters"] = iters
    return prm


@pytest.mark.parametrize("dim_x,dim_y,batch,large", BATCHES)
def test_batch_members_with_a_spacing_each(sfl, oracle, dim_x, dim_y, batch, large):
    fields = [bp.member_fields(dim_x, dim_y, 1000 + 7 * m + dim_x) for m in range(batch)]
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b, sfl.Solver(dim_x, dim_y) as s:
        prm = batch_params(sfl, batch, 31 + dim_x, shift=2, iters=[5, 9, 1, 20, 6][:batch])
        bp.upload_members(b, fields)
        b.poisson_solve_each(prm)
        p = b.download(3)
        for m, (_, _, d) in enumerate(fields):
            assert_bit_equal(p[m], oracle.poisson_solve(d, prm["dx"][m], int(prm["iters"][m]), prm["omega"][m]), f"solve, member {m} ({prm[m]})")
        bp.assert_reports(b, b.download(2), p, prm, "after poisson_solve_each")
        prm = batch_params(sfl, batch, 32 + dim_x, iters=[5, 9, 1, 20, 6][:batch])
        b.step_n_each(2, prm)
        got = bp.download_all(b)
        for m, (v, c, _) in enumerate(fields):
            want = bp.context_run(s, v, c, prm[m], steps=2)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} ({prm[m]}) against a context's step_n")
            if m == 0:      # ... and the context itself against the oracle
                state = (v, None, None, c)
                for _ in range(2):
                    state = oracle.step(state[0], state[3], prm["dt"][m], prm["dx"][m], int(prm["iters"][m]), prm["omega"][m])
                assert_fields(want, state, f"the context of member {m} against the oracle")
        bp.assert_reports(b, got[1], got[2], prm, "after step_n_each")


@pytest.mark.parametrize("dim_x,dim_y,batch,large", BATCHES)
def test_batch_solves_stopped_at_a_tolerance(sfl, oracle, dim_x, dim_y, batch, large):
    """test_batch_until.py's rule: member m stops at the k the numpy rule finds on ITS divergence and ITS dx, and holds the
    oracle's step of k iterations."""
    fields = [bp.member_fields(dim_x, dim_y, 1100 + 7 * m + dim_x, 40.0) for m in range(batch)]
    prm = batch_params(sfl, batch, 41 + dim_x, iters=24)
    prm["omega"] = 1.9
    stops = sfl.member_stops(batch, [9.0, 4.5, -1.0, 6.0, 3.0][:batch], 4)
    steps = [yardstick_step(oracle, v, c, prm[m], stops[m]) for m, (v, c, _) in enumerate(fields)]
    ks = [k for k, _, _ in steps]
    print("k of every member:", ks)
    assert any(0 < k < 24 for k in ks) and any(k == 24 for k in ks), "the yardstick must stop some member early and run some to the cap"
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        bp.upload_members(b, fields)
        b.step_n_until(1, prm, tol=stops)
        got = bp.download_all(b)
        its, res = b.iterations(), b.residual()
    for m, (k, _, state) in enumerate(steps):
        assert tuple(its[m]) == (k, k), f"member {m} ({prm[m]}, {stops[m]}): iterations {its[m]}, the yardstick's {k}"
        for f, name in enumerate(FIELDS):
            assert_bit_equal(got[f][m], state[f], f"{name}, member {m} ({prm[m]}, {stops[m]}) at k = {k}")
        assert_report_equal(res[m], update_norm(got[2][m], got[1][m], prm["dx"][m]), f"member {m} ({prm[m]})")


def test_batch_replay_in_one_launch(sfl, oracle):
    """step_n(3) with a record at step 1 and no following tracer set: batch_play.hip, its own divergence and projection."""
    dim_x, dim_y, batch = 61, 81, 5
    fields = [bp.member_fields(dim_x, dim_y, 1200 + m, 40.0) for m in range(batch)]
    records = {1: [(1, (30, 40), (55.0, -35.0)), (4, (0, 0), (3.0, 4.0)), (4, (60, 80), (-20.0, 10.0))]}
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        bp.upload_members(b, fields)
        b.queue_forces(*zip(*records[1]), step=1)
        b.step_n(3, DT, DX_A, 4, OMEGA)
        got = bp.download_all(b)
    for m, (v, c, _) in enumerate(fields):
        mine = {k: [(cell, vel) for mm, cell, vel in r if mm == m] for k, r in records.items()}
        want = oracle_steps(oracle, v, c, mine, 3, DT, DX_A, 4, OMEGA)
        for name, a, w in zip(FIELDS, got, want):
            assert_bit_equal(a[m], w, f"{name}, member {m} after three steps in one launch")


# ---- flow statistics (flow_stats.hip: divergence_sum * two_dx_inv, never stored) ------------------------------------------
@pytest.mark.parametrize("dx", [DX_A, DX_C], ids=dx_id)
def test_flow_stats_of_a_context(sfl, oracle, dx):
    v, c, _ = random_fields(130, 70, 1300)
    with context(sfl, 130, 70) as s:
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
        assert_stats(s.flow_stats(dx), stats_yardstick(oracle, v, c, dx), f"130 x 70, dx {dx!r}")


@pytest.mark.parametrize("dim_x,dim_y,batch,large", BATCHES)
def test_flow_stats_of_a_batch(sfl, oracle, dim_x, dim_y, batch, large):
    fields = [bp.member_fields(dim_x, dim_y, 1400 + 7 * m + dim_x) for m in range(batch)]
    each = [DX_CASES[m % len(DX_CASES)] for m in range(batch)]
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        bp.upload_members(b, fields)
        for dx in (DX_A, DX_C):
            got = b.flow_stats(dx)
            for m, (v, c, _) in enumerate(fields):
                assert_stats(got[m], stats_yardstick(oracle, v, c, dx), f"member {m}, dx {dx!r}")
        got = b.flow_stats(each)
        for m, (v, c, _) in enumerate(fields):
            assert_stats(got[m], stats_yardstick(oracle, v, c, each[m]), f"member {m}, its own dx {each[m]!r}")


# ---- the C++ drop-in headers ---------------------------------------------------------------------------------------------
def test_reference_style_caller_at_an_inexact_spacing(tmp_path, oracle):
    """tests/cpp/dropin_loop.cpp with a spacing argument: one calculate_divergence, poisson_solve and subtract_gradient at
    dx = 0.37f through include/sfl/finitediff.h and poisson.h."""
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", os.path.join(ROOT, "esp32-fluid-simulation_amd", "host")], check=True, stdout=subprocess.DEVNULL)
    subprocess.run(["make", "-C", cpp, "dropin"], check=True, stdout=subprocess.DEVNULL)
    dim_x, dim_y, iters = 61, 81, 6
    v, c = oracle.lcg_fields(dim_x, dim_y, 4321, 90.0)
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(struct.pack("3i", dim_x, dim_y, iters))
        f.write(v.tobytes())
        f.write(c.tobytes())
    subprocess.run([os.path.join(cpp, "dropin_loop"), str(fin), "1", str(fout), "0.37"], check=True)
    raw = open(fout, "rb").read()
    n = dim_x * dim_y
    got = [np.frombuffer(raw, np.float32, 2 * n, 0).reshape(dim_y, dim_x, 2), np.frombuffer(raw, np.float32, n, 8 * n).reshape(dim_y, dim_x),
           np.frombuffer(raw, np.float32, n, 12 * n).reshape(dim_y, dim_x), np.frombuffer(raw, np.uint32, 3 * n, 16 * n).reshape(dim_y, dim_x, 3)]
    assert_fields(got, oracle.step(v, c, DT, DX_A, iters, OMEGA), "drop-in caller at dx 0.37")
