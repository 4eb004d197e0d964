"""Batches of large members (sfl_batch_create_large, sfl_batch_is_large): up to 20224 cells per member with 8 B of LDS
per cell -- the advected velocity first, the divergence and the pressure afterwards in the same bytes.

The contract under test is the batches' own, unchanged: after any sequence of batch calls member m holds, bit for bit,
what a whole-domain context of the same shape holds after the same calls made with member m's data, forces and
parameters; residual() is the update norm of include/sfl.h and iterations() the k of its stopping rule.  The yardsticks
are the oracle, single contexts, a batch of sfl_batch_create at a shape both kinds take, and the numpy restatement of
the update norm of test_batch_params.py.  A batch made by sfl_batch_create_large runs the large-member kernels whatever
its shape, so the smallest shapes test them too.  The CPU tests need no GPU: the limits are checked before any device
is touched.  All comparisons are bit for bit; a NaN is matched by any NaN."""
import ctypes as C
import functools

import numpy as np
import pytest

import test_batch_params as bp
import test_batch_until as bu
import test_flow_stats as tf
from conftest import assert_bit_equal
from test_batch_params import FIELDS, assert_report_equal, update_norm

DT = np.float32(1 / 30.0)
OMEGA = np.float32(1.96)
LARGE_SYMBOLS = ["sfl_batch_create_large", "sfl_batch_is_large"]
# the smallest shapes the kernels accept; member bases not 16-byte aligned; 6162 cells, just past the old limit; the
# target sizes; 20164 cells, near the new limit; an odd width; narrow and tall; 20005 cells, 10005 of one colour
LARGE_SHAPES = [(2, 2), (3, 3), (5, 7), (61, 81), (79, 78), (128, 128), (160, 120), (142, 142), (257, 63), (2, 5000), (4001, 5)]


# ---- CPU ----------------------------------------------------------------------------------------------
def test_both_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in LARGE_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    assert sfl.capi.SIGNATURES["sfl_batch_create_large"] == sfl.capi.SIGNATURES["sfl_batch_create"]
    assert sfl.capi.BATCH_LARGE_MAX_CELLS == 20224 >= 160 * 120
    assert isinstance(sfl.BatchSolver.large, property)


@pytest.mark.parametrize("dims,limit", [
    ((1, 81, 4), "dim_x and dim_y must be >= 2"),
    ((61, 1, 4), "dim_x and dim_y must be >= 2"),
    ((61, 81, 0), "batch must be >= 1"),
    ((4045, 5, 1), "at most 20224 cells"),                 # 20225 cells
    ((3, 6741, 1), "at most 10240 cells of one colour"),   # 20223 cells, 13482 of one colour
    ((64, 64, 524288), "2^31 - 1"),                        # batch x cells = 2^31
])
def test_create_large_refuses_what_does_not_fit_before_touching_a_gpu(sfl, dims, limit):
    lib = sfl.capi.lib()
    h = C.c_void_p()
    assert lib.sfl_batch_create_large(C.byref(h), 0, *dims) == sfl.capi.ERR_INVALID
    assert limit in lib.sfl_last_error().decode()
    assert not h.value


def test_null_pointers_are_refused(sfl):
    lib = sfl.capi.lib()
    assert lib.sfl_batch_create_large(None, 0, 128, 128, 4) == sfl.capi.ERR_INVALID
    assert "NULL" in lib.sfl_last_error().decode()
    flag = C.c_int(7)
    assert lib.sfl_batch_is_large(None, C.byref(flag)) == sfl.capi.ERR_INVALID
    assert "NULL" in lib.sfl_last_error().decode() and flag.value == 7


def test_a_valid_large_batch_without_a_device_fails_loudly(sfl):
    if sfl.device_count() > 0:
        pytest.skip("a GPU is present: the create succeeds (the GPU tests below use it)")
    for dims in ((128, 128, 4), (160, 120, 1), (2, 2, 1), (4001, 5, 2)):
        with pytest.raises(sfl.SflError) as e:
            sfl.BatchSolver(*dims, large=True)
        assert e.value.code == sfl.capi.ERR_HIP   # the limits passed; no CPU fallback


# ---- GPU ----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def members(dim_x, dim_y, batch, seed, vamp=90.0):
    """`batch` members' distinct seeded fields (velocity, dye over [0, 0xFF000000), a scalar).  Shared: never written to."""
    fields = [bp.member_fields(dim_x, dim_y, seed + 7 * m, vamp) for m in range(batch)]
    for f in fields:
        for a in f:
            a.setflags(write=False)
    return fields


def forces_for(dim_x, dim_y):
    """Forces on members 0 and 2: member 0 has two records on the same cell (the last one wins) and one outside."""
    mid = (dim_x // 2, dim_y // 2)
    return {0: [(mid, (55.0, -35.0)), (mid, (-8.0, 6.0)), ((dim_x, 0), (99.0, 99.0))],
            2: [((dim_x - 1, dim_y - 1), (-20.0, 10.0)), ((0, 0), (3.0, 4.0))]}


def queue(b, forces):
    records = [(m, cell, vel) for m in sorted(forces) for cell, vel in forces[m]]
    b.queue_forces([r[0] for r in records], [r[1] for r in records], [r[2] for r in records])


def oracle_steps(oracle, v, c, prm, forces, steps):
    """`steps` steps of the oracle with one member's parameters, the forces in the first."""
    state = (v, None, None, c)
    for k in range(steps):
        state = bu.oracle_step(oracle, state[0], state[3], prm["dt"], prm["dx"], int(prm["iters"]), prm["omega"],
                               forces if k == 0 else ())
    return state


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", LARGE_SHAPES)
def test_three_steps_of_every_member_equal_the_oracle(sfl, oracle, dim_x, dim_y):
    batch, steps = 3, 3
    fields = members(dim_x, dim_y, batch, 100 + dim_x)
    forces = forces_for(dim_x, dim_y)
    prm = sfl.member_params(batch, DT, 1.0, 5, OMEGA)
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        assert b.shape == (dim_x, dim_y, batch) and b.large
        bp.upload_members(b, fields)
        queue(b, forces)
        b.step_n(steps, DT, 1.0, 5, OMEGA)
        b.synchronize()
        got = bp.download_all(b)
    for m, (v, c, _) in enumerate(fields):
        want = oracle_steps(oracle, v, c, prm[m], forces.get(m, ()), steps)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(got[k][m], want[k], f"{name}, member {m}")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", LARGE_SHAPES)
def test_the_solve_of_every_member_equals_the_oracle(sfl, oracle, dim_x, dim_y):
    batch = 3
    fields = members(dim_x, dim_y, batch, 100 + dim_x)
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        bp.upload_members(b, fields)
        for iters, dx in ((7, 1.0), (1, 0.5), (0, 1.0)):
            b.poisson_solve(dx, iters, OMEGA)
            b.synchronize()
            p = b.download(3)
            for m, (_, _, d) in enumerate(fields):
                assert_bit_equal(p[m], oracle.poisson_solve(d, dx, iters, OMEGA), f"member {m}, {iters} iterations, dx {dx}")
            if iters == 0:
                assert not np.any(p), "no iterations: the zero fill"


@pytest.mark.gpu
def test_a_member_equals_a_context_on_the_general_kernels(sfl):
    dim_x, dim_y, batch, steps, iters = 128, 128, 2, 3, 9
    fields = members(dim_x, dim_y, batch, 4000, 40.0)
    forces = {1: [((64, 64), (55.0, -35.0)), ((64, 64), (-8.0, 6.0)), ((127, 0), (3.0, 4.0))]}
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        bp.upload_members(b, fields)
        queue(b, forces)
        b.step_n(steps, DT, 0.5, iters, OMEGA)
        b.synchronize()
        got = bp.download_all(b)
    prm = sfl.member_params(1, DT, 0.5, iters, OMEGA)[0]
    with sfl.Solver(dim_x, dim_y) as s:
        for m, (v, c, _) in enumerate(fields):
            want = bp.context_run(s, v, c, prm, forces.get(m, ()), steps=steps)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} against a context")


@pytest.mark.gpu
def test_both_kinds_of_batch_agree_where_both_apply(sfl):
    dim_x, dim_y, batch = 61, 81, 5
    fields = members(dim_x, dim_y, batch, 7000, 40.0)
    forces = forces_for(dim_x, dim_y)
    prm = sfl.member_params(batch, [1 / 30.0, 1 / 60.0, 0.1, 1 / 30.0, 1 / 60.0], [1.0, 0.5, 2.0, 1.0, 0.5], [9, 0, 20, 33, 5],
                            [1.96, 1.5, 1.9, 1.0, 1.96])
    cap = sfl.member_params(batch, prm["dt"], prm["dx"], [60, 33, 0, 120, 17], [1.9, 1.96, 1.5, 1.0, 1.9])
    stops = sfl.member_stops(batch, [0.1, 1e-2, 1e-3, -1.0, np.inf], [4, 1, 7, 4, 1])
    lib, flag = sfl.capi.lib(), C.c_int(-1)
    with sfl.BatchSolver(dim_x, dim_y, batch) as small, sfl.BatchSolver(dim_x, dim_y, batch, large=True) as large:
        for b, want in ((small, 0), (large, 1)):
            assert lib.sfl_batch_is_large(b._h, C.byref(flag)) == sfl.capi.OK and flag.value == want
            assert b.large == bool(want)
            bp.upload_members(b, fields)
            queue(b, forces)
            b.step_n_each(2, prm)
        for k, (g, w) in enumerate(zip(bp.download_all(large), bp.download_all(small))):
            assert_bit_equal(g, w, f"{FIELDS[k]} after step_n_each")
        assert_bit_equal(large.residual(), small.residual(), "the update norm after step_n_each")
        for b in (small, large):
            queue(b, {3: [((7, 9), (4.0, 4.0))]})
            b.step_n_until(2, cap, tol=stops)
        for k, (g, w) in enumerate(zip(bp.download_all(large), bp.download_all(small))):
            assert_bit_equal(g, w, f"{FIELDS[k]} after step_n_until")
        assert_bit_equal(large.residual(), small.residual(), "the update norm after step_n_until")
        print("iterations:", small.iterations().tolist())
        assert large.iterations().tolist() == small.iterations().tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(5, 7), (61, 81), (79, 78), (128, 128), (4001, 5)])
def test_each_member_with_its_own_parameters_and_its_update_norm(sfl, oracle, dim_x, dim_y):
    batch = 4
    fields = members(dim_x, dim_y, batch, 2000 + dim_x)
    prm = sfl.member_params(batch, [1 / 30.0, 1 / 60.0, 0.1, 1 / 30.0], [1.0, 0.5, 2.0, 1.0], [9, 0, 20, 3], [1.96, 1.5, 1.9, 1.0])
    forces = forces_for(dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        bp.upload_members(b, fields)
        b.poisson_solve_each(prm)
        p = b.download(3)
        for m, (_, _, d) in enumerate(fields):
            assert_bit_equal(p[m], oracle.poisson_solve(d, prm["dx"][m], int(prm["iters"][m]), prm["omega"][m]),
                             f"solve, member {m} ({prm[m]})")
        bp.assert_reports(b, b.download(2), p, prm, "after poisson_solve_each")
        queue(b, forces)
        b.step_n_each(2, prm)
        got = bp.download_all(b)
        for m, (v, c, _) in enumerate(fields):
            want = oracle_steps(oracle, v, c, prm[m], forces.get(m, ()), 2)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} ({prm[m]})")
        bp.assert_reports(b, got[1], got[2], prm, "after step_n_each")


@pytest.mark.gpu
def test_a_nan_in_one_members_divergence_is_that_members_alone(sfl):
    dim_x, dim_y, batch = 128, 128, 3
    d = np.stack([f[2] for f in members(dim_x, dim_y, batch, 2500)]).copy()
    d[1, 77, 31] = np.nan
    prm = sfl.member_params(batch, 0.0, 1.0, 2, 1.9)   # two iterations: the NaN has reached a few cells, not all
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        b.upload(2, d)
        b.poisson_solve_each(prm)
        p, res = b.download(3), b.residual()
    print("update norms:", res)
    assert np.isnan(res[1]) and np.isnan(update_norm(p[1], d[1], 1.0)) and not np.all(np.isnan(p[1]))
    for m in (0, 2):
        assert np.isfinite(res[m]) and np.all(np.isfinite(p[m]))
        assert_report_equal(res[m], update_norm(p[m], d[m], 1.0), f"member {m}")


# ---- stopping at a tolerance ------------------------------------------------------------------------------
def smooth_divergence(oracle, dim_x, dim_y, member, dx):
    """The divergence of a smooth velocity that vanishes on the walls: zero mean, so the solve converges -- within tens
    of iterations, the velocity having eight to thirteen half waves across the grid."""
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    x, y = i / (dim_x - 1.0), j / (dim_y - 1.0)
    kx, ky = 8 + 2 * (member % 3), 8 + member % 2
    v = np.stack([np.sin(kx * np.pi * x) * np.sin(ky * np.pi * y) * (20.0 + member),
                  np.sin((kx + 1) * np.pi * x) * np.sin(ky * np.pi * y) * (15.0 - member)], axis=-1).astype(np.float32)
    return oracle.divergence(v, np.float32(dx))


def expected_stop(oracle, d, dx, cap, omega, tol, every):
    """The rule of include/sfl.h (sfl_member_stop) by the oracle's solve: -> (k, u_k, the pressure of k iterations)."""
    k = 0
    while True:
        p = oracle.poisson_solve(d, np.float32(dx), k, np.float32(omega))
        u = np.float32(update_norm(p, d, dx))
        if k >= cap or (tol >= 0 and (u <= np.float32(tol) or np.isnan(u))):
            return k, u, p
        k = min(k + every, cap)


# (dx, cap, omega, tol, every) of the six members
UNTIL_MEMBERS = [(1.0, 80, 1.8, 0.05, 4), (1.0, 25, 1.0, 1e-4, 7), (1.0, 30, 1.9, np.inf, 4), (0.5, 17, 1.96, -1.0, 3),
                 (1.0, 90, 1.9, 0.02, 1), (2.0, 60, 1.5, 0.2, 5)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (128, 128)])
def test_every_member_stops_where_the_rule_stops_it(sfl, oracle, dim_x, dim_y):
    batch = len(UNTIL_MEMBERS)
    d = np.stack([smooth_divergence(oracle, dim_x, dim_y, m, q[0]) for m, q in enumerate(UNTIL_MEMBERS)])
    want = [expected_stop(oracle, d[m], *q) for m, q in enumerate(UNTIL_MEMBERS)]
    ks, caps = [w[0] for w in want], [q[1] for q in UNTIL_MEMBERS]
    print(f"{dim_x} x {dim_y}: k = {ks} of {caps}, norms {[float(w[1]) for w in want]}")
    # the members are what the test is about (on the yardstick alone): one stops at 0, one in between, one at its cap
    assert any(k == 0 for k in ks) and any(0 < k < c for k, c in zip(ks, caps)) and any(k == c for k, c in zip(ks, caps))
    prm = sfl.member_params(batch, 0.0, [q[0] for q in UNTIL_MEMBERS], caps, [q[2] for q in UNTIL_MEMBERS])
    stops = sfl.member_stops(batch, [q[3] for q in UNTIL_MEMBERS], [q[4] for q in UNTIL_MEMBERS])
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        b.upload(2, d)
        b.poisson_solve_until(prm, tol=stops)
        its, res, p = b.iterations(), b.residual(), b.download(3)
        assert its.tolist() == [[k, k] for k in ks]
        for m, (k, u, wp) in enumerate(want):
            assert_report_equal(res[m], u, f"member {m} {UNTIL_MEMBERS[m]}")
            assert_bit_equal(p[m], wp, f"pressure, member {m} {UNTIL_MEMBERS[m]} at k = {k}")
        # the staleness rules, as on small batches
        b.step_n(1, DT, 1.0, 2, OMEGA)
        for report in (b.iterations, b.residual):
            with pytest.raises(sfl.SflError) as e:
                report()
            assert e.value.code == sfl.capi.ERR_STATE
        b.upload(2, d)
        b.poisson_solve_until(prm, tol=stops)
        assert b.iterations().tolist() == its.tolist()
        assert_bit_equal(b.residual(), res, "the update norm of the same solve again")
        b.upload(3, np.zeros((1, dim_y, dim_x), np.float32), first=1)   # an upload of the pressure
        for report in (b.iterations, b.residual):
            with pytest.raises(sfl.SflError) as e:
                report()
            assert e.value.code == sfl.capi.ERR_STATE


# ---- more members than workgroup slots ----------------------------------------------------------------------
@pytest.mark.gpu
def test_520_members_on_256_compute_units(sfl, oracle):
    """One member per CU: members 256 .. 519 follow others on a CU whose LDS still holds their pressure and divergence."""
    dim_x, dim_y, batch, steps, iters = 128, 128, 520, 2, 3
    rng = np.random.default_rng(520)
    v = (rng.uniform(-1, 1, (batch, dim_y, dim_x, 2)) * 40.0).astype(np.float32)
    c = rng.integers(0, 0xFF000000, (batch, dim_y, dim_x, 3), dtype=np.uint32)
    prm = sfl.member_params(1, DT, 1.0, iters, OMEGA)[0]
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b:
        b.upload(0, v)
        b.upload(1, c)
        b.step_n(steps, DT, 1.0, iters, OMEGA)
        b.synchronize()
        got = {m: [b.download(f, m, 1)[0] for f in (0, 2, 3, 1)] for m in (0, 255, 256, 519)}
    for m, fields in got.items():
        want = oracle_steps(oracle, v[m], c[m], prm, (), steps)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(fields[k], want[k], f"{name}, member {m}")


# ---- the calls whose kernels do not depend on the member size -----------------------------------------------
@pytest.mark.gpu
def test_flow_stats_setup_and_render_of_a_large_batch(sfl, oracle):
    dim_x, dim_y, batch = 128, 128, 4
    fields = members(dim_x, dim_y, batch, 900)
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b, sfl.Solver(dim_x, dim_y) as s:
        bp.upload_members(b, fields)
        stats = b.flow_stats(0.5)
        for m, (v, c, _) in enumerate(fields):
            tf.assert_stats(stats[m], tf.yardstick(oracle, v, c, 0.5), f"member {m}")
        each = b.flow_stats([1.0, 0.5, 2.0, 0.25], first=1, count=2, dye=False)
        for k, m in enumerate((1, 2)):
            tf.assert_stats(each[k], tf.yardstick(oracle, fields[m][0], None, (1.0, 0.5, 2.0, 0.25)[m]), f"member {m}, its own dx", dye=False)
        for scaling, byteswap in ((2, True), (1, False)):
            s.upload(1, fields[2][1])
            assert_bit_equal(b.render_rgb565(2, scaling, byteswap), s.render_rgb565(scaling, byteswap), "the render of member 2")
        b.setup_sketch_fields()
        s.setup_sketch_fields()
        for f, name in ((0, "velocity"), (1, "colour")):
            assert_bit_equal(b.download(f, 3, 1)[0], s.download(f), f"{name} of member 3 after setup_sketch_fields")
