"""Batches with parameters of each member's own (sfl_batch_step_n_each, sfl_batch_poisson_solve_each) and the update
norm they leave (sfl_batch_residual): one float per member, max |p_gs - p| on the member's final pressure.

The contract under test: member m ends up, bit for bit, where a context of the same shape ends up after the same calls
made with member m's data, forces AND parameters; and residual()[m] equals, bit for bit, the numpy restatement below
evaluated on the divergence and pressure a download hands out (NaN <-> any NaN).  The numpy restatement itself is pinned
against the oracle by a CPU test.  All comparisons are bit for bit."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import assert_bit_equal
from dx_cases import DX_A, DX_C, widened

FIELDS = ("velocity", "divergence", "pressure", "colour")
EACH_SYMBOLS = ["sfl_batch_step_n_each", "sfl_batch_poisson_solve_each", "sfl_batch_residual"]
BATCH_SHAPES = [(2, 2), (3, 3), (61, 81), (80, 60), (78, 78), (128, 48), (257, 23), (2047, 3), (2, 3072)]
# the parameter points of the GPU tests are drawn from these with a fixed seed
DTS, DXS = (1 / 30.0, 1 / 60.0, 0.1), (1.0, 0.5, widened(DX_A), widened(DX_C))    # (the last two: no product with dx is exact)
ITERS, OMEGAS = (0, 1, 5, 9, 20, 33), (1.0, 1.5, 1.9, 1.96)


# ---- the yardstick: numpy restatement of the update norm ----------------------------------------------
def gs_target(p, d, dx):                       # p, d: float32[dim_y, dim_x]
    """p_gs of every cell (poisson.cpp:67-89 on the perimeter, :107-109 inside): float32, every operation on its own."""
    f = np.float32
    s = np.zeros_like(p); n = np.zeros(p.shape, np.int32)
    s[:, 1:]  = s[:, 1:]  + p[:, :-1]; n[:, 1:]  += 1     # W
    s[:, :-1] = s[:, :-1] + p[:, 1:];  n[:, :-1] += 1     # E
    s[1:, :]  = s[1:, :]  + p[:-1, :]; n[1:, :]  += 1     # S
    s[:-1, :] = s[:-1, :] + p[1:, :];  n[:-1, :] += 1     # N
    k = np.array([0, 0, f(-1.0 / 2.0), f(-1.0 / 3.0), f(-0.25)], np.float32)[n]
    return k * (f(dx) * d - s)


def update_norm(p, d, dx):
    with np.errstate(all="ignore"):
        return np.max(np.abs(gs_target(p, d, dx) - p))    # np.max propagates NaN


def numpy_sor(d, dx, iters, omega):
    """Red-black SOR from zero built on gs_target: poisson_solve (poisson.cpp:114-125)."""
    f = np.float32
    p = np.zeros_like(d)
    jj, ii = np.indices(d.shape)
    with np.errstate(all="ignore"):
        for _ in range(iters):
            for colour in (0, 1):
                g = gs_target(p, d, dx)
                p = np.where(((ii + jj) & 1) == colour, (f(1) - f(omega)) * p + f(omega) * g, p).astype(np.float32)
    return p


def assert_report_equal(got, want, what):
    """Bit for bit; the one relaxation: a NaN is matched by any NaN."""
    got, want = np.float32(got), np.float32(want)
    if np.isnan(want):
        assert np.isnan(got), f"{what}: the update norm is a NaN, the batch reports {got!r}"
    else:
        assert got.view(np.uint32) == want.view(np.uint32), \
            f"{what}: update norm {got!r} (0x{int(got.view(np.uint32)):08x}), want {want!r} (0x{int(want.view(np.uint32)):08x})"


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in EACH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    mp = sfl.capi.MemberParams
    assert C.sizeof(mp) == 16
    assert [(n, getattr(mp, n).offset) for n, _ in mp._fields_] == [("dt", 0), ("dx", 4), ("omega", 8), ("iters", 12)]
    for name in ("step_n_each", "poisson_solve_each", "residual"):
        assert hasattr(sfl.BatchSolver, name), name


def test_a_null_batch_is_refused_by_all_three(sfl):
    lib = sfl.capi.lib()
    prm = (sfl.capi.MemberParams * 2)()
    out = (C.c_float * 2)()
    for call in (lambda: lib.sfl_batch_step_n_each(None, 1, prm),
                 lambda: lib.sfl_batch_poisson_solve_each(None, prm),
                 lambda: lib.sfl_batch_residual(None, 0, 2, out, 8)):
        assert call() == sfl.capi.ERR_INVALID
        assert "NULL" in lib.sfl_last_error().decode()


def test_member_params_broadcasts_into_the_c_layout(sfl):
    want = np.dtype([("dt", "<f4"), ("dx", "<f4"), ("omega", "<f4"), ("iters", "<i4")])
    a = sfl.member_params(5, 0.1)                                    # scalars (and the defaults) broadcast
    assert a.dtype == want and a.dtype.itemsize == 16 and a.shape == (5,) and a.flags["C_CONTIGUOUS"]
    assert [a.dtype.fields[n][1] for n in ("dt", "dx", "omega", "iters")] == [0, 4, 8, 12]
    assert np.all(a["dt"] == np.float32(0.1)) and np.all(a["dx"] == 1) and np.all(a["iters"] == 10)
    assert np.all(a["omega"] == np.float32(1.96))
    b = sfl.member_params(3, [0.1, 0.2, 0.3], [1, 2, 3], [4, 5, 6], [1.0, 1.5, 1.9])   # sequences kept
    assert_bit_equal(b["dt"], np.array([0.1, 0.2, 0.3], np.float32))
    assert_bit_equal(b["dx"], np.array([1, 2, 3], np.float32))
    assert_bit_equal(b["omega"], np.array([1.0, 1.5, 1.9], np.float32))
    assert b["iters"].tolist() == [4, 5, 6]
    c = sfl.member_params(4, 1 / 30.0, iters=np.arange(4), omega=(1.0, 1.2, 1.4, 1.6))  # mixed
    assert np.all(c["dt"] == np.float32(1 / 30.0)) and c["iters"].tolist() == [0, 1, 2, 3] and np.all(c["dx"] == 1)
    assert_bit_equal(c["omega"], np.array([1.0, 1.2, 1.4, 1.6], np.float32))
    assert c.tobytes() == b"".join(bytes(sfl.capi.MemberParams(r["dt"], r["dx"], r["omega"], r["iters"])) for r in c)
    for bad in (dict(dt=[0.1, 0.2]), dict(dt=0.1, iters=[1, 2, 3, 4, 5]), dict(dt=0.1, omega=[]),
                dict(dt=0.1, dx=np.ones((3, 1)))):
        with pytest.raises(ValueError):
            sfl.member_params(3, **bad)


@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (3, 3), (61, 81), (257, 23)])
@pytest.mark.parametrize("dx,iters,omega", [(1.0, 9, 1.96), (0.5, 20, 1.5), (2.0, 3, 1.0), (widened(DX_A), 9, 1.96), (3.0, 5, 1.5)])
def test_the_yardstick_is_the_oracles_gauss_seidel_target(oracle, dim_x, dim_y, dx, iters, omega):
    """A red-black SOR built on gs_target IS the oracle's poisson_solve, bit for bit: g is its p_gs, not an estimate."""
    d = np.random.default_rng(3 + dim_x).standard_normal((dim_y, dim_x)).astype(np.float32)
    assert_bit_equal(numpy_sor(d, dx, iters, omega), oracle.poisson_solve(d, dx, iters, np.float32(omega)),
                     f"numpy SOR on gs_target, {dim_x} x {dim_y}, dx {dx}, {iters} iterations, omega {omega}")


# ---- GPU ----------------------------------------------------------------------------------------------
def member_fields(dim_x, dim_y, seed, vamp=90.0):
    """Distinct seeded fields of one member; dye over all of [0, 0xFF000000) (both halves of UQ32)."""
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (dim_y, dim_x, 2)) * vamp).astype(np.float32)
    c = rng.integers(0, 0xFF000000, (dim_y, dim_x, 3), dtype=np.uint32)
    d = rng.standard_normal((dim_y, dim_x)).astype(np.float32)
    return v, c, d


def upload_members(b, fields):
    b.upload(0, np.stack([f[0] for f in fields]))
    b.upload(1, np.stack([f[1] for f in fields]))
    b.upload(2, np.stack([f[2] for f in fields]))


def download_all(b, first=0, count=None):
    return [b.download(f, first, count) for f in (0, 2, 3, 1)]   # velocity, divergence, pressure, colour


def draw_params(sfl, batch, seed):
    rng = np.random.default_rng(seed)
    pick = lambda values: [values[k] for k in rng.integers(0, len(values), batch)]
    return sfl.member_params(batch, pick(DTS), pick(DXS), pick(ITERS), pick(OMEGAS))


def context_run(s, v, c, prm, forces=(), steps=1):
    """A single context's answer with ONE member's parameters: upload, queue forces, step_n."""
    s.upload(0, v)
    s.upload(1, c)
    if forces:
        cells, vel = zip(*forces)
        s.queue_forces(np.array(cells, np.int32), np.array(vel, np.float32))
    s.step_n(steps, prm["dt"], prm["dx"], int(prm["iters"]), prm["omega"])
    s.synchronize()
    return [s.download(f) for f in (0, 2, 3, 1)]


def assert_reports(b, got_d, got_p, prm, what):
    res = b.residual()
    assert res.dtype == np.float32 and res.shape == (len(prm),)
    for m in range(len(prm)):
        assert_report_equal(res[m], update_norm(got_p[m], got_d[m], prm["dx"][m]), f"{what}, member {m} ({prm[m]})")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", BATCH_SHAPES)
@pytest.mark.parametrize("batch", [1, 3, 37])
def test_every_member_equals_the_oracle_with_its_own_parameters(sfl, oracle, dim_x, dim_y, batch):
    fields = [member_fields(dim_x, dim_y, 2000 * batch + 11 * m + dim_x) for m in range(batch)]
    prm = draw_params(sfl, batch, 100 * batch + dim_x)
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        upload_members(b, fields)
        b.poisson_solve_each(prm["dx"], prm["iters"], prm["omega"])
        p = b.download(3)
        for m, (_, _, d) in enumerate(fields):
            assert_bit_equal(p[m], oracle.poisson_solve(d, prm["dx"][m], int(prm["iters"][m]), prm["omega"][m]),
                             f"solve, member {m} ({prm[m]})")
        assert_reports(b, b.download(2), p, prm, "after poisson_solve_each")
        b.step_n_each(1, prm)                        # a ready-made array
        got = download_all(b)
        for m, (v, c, _) in enumerate(fields):
            want = oracle.step(v, c, prm["dt"][m], prm["dx"][m], int(prm["iters"][m]), prm["omega"][m])
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} ({prm[m]})")
        assert_reports(b, got[1], got[2], prm, "after step_n_each")


FORCES_257 = {
    0: [((30, 40), (55.0, -35.0)), ((30, 40), (-8.0, 6.0)), ((0, 0), (3.0, 4.0))],   # the same cell twice: last wins
    128: [((61, 5), (99.0, 99.0)), ((60, 80), (-20.0, 10.0))],                      # (dim_x, 5) lies outside: skipped
    256: [((10, 70), (12.0, -7.0)), ((11, 70), (1.5, 2.5))],
}


def queue_257(b):
    records = [(m, cell, vel) for m in (0, 128, 256) for cell, vel in FORCES_257[m]]
    for part in (records[:4], records[4:]):   # queued in two calls, interleaved members
        b.queue_forces([r[0] for r in part], [r[1] for r in part], [r[2] for r in part])


@pytest.mark.gpu
def test_257_members_with_forces_and_parameters_equal_single_contexts(sfl):
    dim_x, dim_y, batch = 61, 81, 257
    fields = [member_fields(dim_x, dim_y, 5000 + m, 40.0) for m in range(batch)]
    prm = draw_params(sfl, batch, 257)
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        upload_members(b, fields)
        queue_257(b)
        b.step_n_each(3, prm["dt"], prm["dx"], prm["iters"], prm["omega"])
        got = download_all(b)
        assert_reports(b, got[1], got[2], prm, "after three steps")
    with sfl.Solver(dim_x, dim_y) as s:
        for m, (v, c, _) in enumerate(fields):
            want = context_run(s, v, c, prm[m], FORCES_257.get(m, ()), steps=3)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} ({prm[m]})")


@pytest.mark.gpu
def test_the_same_parameters_for_every_member_is_step_n(sfl):
    dim_x, dim_y, batch = 61, 81, 19
    fields = [member_fields(dim_x, dim_y, 7000 + m, 40.0) for m in range(batch)]
    forces = ([0, 7, 7, 18], [(30, 40), (5, 5), (5, 5), (60, 80)], [(55.0, -35.0), (1.0, 2.0), (-3.0, 4.0), (9.0, 9.0)])
    with sfl.BatchSolver(dim_x, dim_y, batch) as each, sfl.BatchSolver(dim_x, dim_y, batch) as uniform:
        for b in (each, uniform):
            upload_members(b, fields)
            b.queue_forces(*forces)
        each.step_n_each(3, 1 / 60.0, 0.5, 9, 1.9)
        uniform.step_n(3, 1 / 60.0, 0.5, 9, 1.9)
        got, want = download_all(each), download_all(uniform)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(got[k], want[k], f"{name}: step_n_each with one parameter set against step_n")
        assert_reports(each, got[1], got[2], sfl.member_params(batch, 1 / 60.0, 0.5, 9, 1.9), "uniform parameters")


@pytest.mark.gpu
def test_diverged_members_report_what_numpy_reports_and_leave_their_neighbours_alone(sfl, oracle):
    """Through poisson_solve_each only: the solve is arithmetic on fixed LDS indices whatever the values are."""
    dim_x, dim_y = 61, 81
    rng = np.random.default_rng(8)
    spike = np.zeros((dim_y, dim_x), np.float32)
    spike[40, 30] = 1.0
    # (dx, iters, omega, rhs) -- members 0, 2, 5, 8 are the healthy neighbours
    healthy = (1.0, 20, 1.96, None)
    cases = [healthy, (1.0, 200, 2.5, None), (0.5, 33, 1.5, None), (1.0, 80, 2.5, None), (1.0, 200, 2.05, None),
             healthy, (2.0, 0, 1.96, None), (1.0, 200, 1.96, spike), (1.0, 9, 1.9, None),
             (1.0, 20, 1.0, spike * np.float32(1e-30))]
    batch = len(cases)
    d = np.stack([rng.standard_normal((dim_y, dim_x)).astype(np.float32) if c[3] is None else c[3] for c in cases])
    prm = sfl.member_params(batch, 0.0, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    with np.errstate(all="ignore"):
        want_p = [oracle.poisson_solve(d[m], *cases[m][:2], np.float32(cases[m][2])) for m in range(batch)]
    # the cases are what they claim to be (so none can go vacuous)
    assert np.isnan(update_norm(want_p[1], d[1], 1.0)), "omega 2.5 x 200: the yardstick must be a NaN"
    for m in (3, 4):
        assert np.all(np.isfinite(want_p[m])) and np.isfinite(update_norm(want_p[m], d[m], 1.0))
        assert update_norm(want_p[m], d[m], 1.0) > 1e5, "huge but finite"
    assert not np.any(want_p[6])
    # (the unit spike fills the grid with normal numbers within 40 iterations; scaled to 1e-30 its front is denormal)
    assert np.all(want_p[7] != 0)
    front = np.abs(want_p[9][want_p[9] != 0])
    assert np.any(front < np.finfo(np.float32).tiny), "the scaled single-cell right-hand side must leave denormals in p"
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.upload(2, d)
        b.poisson_solve_each(prm)
        p, res = b.download(3), b.residual()
    print("update norms:", res)
    for m in range(batch):
        if np.all(np.isfinite(want_p[m])):   # every member but the one that reaches inf / NaN
            assert_bit_equal(p[m], want_p[m], f"pressure, member {m} {cases[m][:3]}")
        assert_report_equal(res[m], update_norm(p[m], d[m], cases[m][0]), f"member {m} {cases[m][:3]}")
    assert np.isnan(res[1]) and np.isnan(update_norm(p[1], d[1], 1.0))
    k = np.array([0, 0, -1.0 / 2.0, -1.0 / 3.0, -0.25], np.float32)[gs_neighbours(dim_x, dim_y)]
    assert_report_equal(res[6], np.max(np.abs(k * (np.float32(2.0) * d[6]))), "iters = 0: max |k dx d|")


def gs_neighbours(dim_x, dim_y):
    n = np.full((dim_y, dim_x), 4, np.int32)
    n[0, :] -= 1; n[-1, :] -= 1; n[:, 0] -= 1; n[:, -1] -= 1
    return n


@pytest.mark.gpu
def test_when_a_report_is_valid_and_what_is_refused(sfl):
    dim_x, dim_y, batch = 61, 81, 8
    fields = [member_fields(dim_x, dim_y, 9000 + m, 40.0) for m in range(batch)]
    prm = draw_params(sfl, batch, 9)
    lib, cap = sfl.capi.lib(), sfl.capi

    def stale(b):
        with pytest.raises(sfl.SflError) as e:
            b.residual()
        assert e.value.code == cap.ERR_STATE
        assert "_each" in str(e.value)       # the message says which call to make

    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.Solver(dim_x, dim_y) as s:
        stale(b)                                                   # a fresh batch
        upload_members(b, fields)
        b.step_n_each(0, prm)                                      # n == 0 launches nothing: still no report
        stale(b)
        b.step_n_each(1, prm)
        first = b.residual()
        assert_reports(b, b.download(2), b.download(3), prm, "first report")
        b.step_n_each(0, prm)                                      # ... and leaves a report as it was
        assert_bit_equal(b.residual(), first, "report after n == 0")
        b.step_n(1, 1 / 30.0, 1.0, 5, 1.96)
        stale(b)
        b.poisson_solve_each(prm)
        assert_reports(b, b.download(2), b.download(3), prm, "after poisson_solve_each")
        b.poisson_solve(1.0, 5, 1.96)
        stale(b)
        b.step_n_each(1, prm)
        b.residual()
        b.upload(3, np.zeros((1, dim_y, dim_x), np.float32), first=2)   # an upload of the pressure
        stale(b)
        b.poisson_solve_each(prm)
        b.upload(2, fields[0][2][None])                            # ... or of the divergence
        stale(b)
        b.poisson_solve_each(prm)
        b.upload(0, fields[0][0][None])                            # velocity and dye are not what the report is about
        res = b.residual()
        # ranges and byte counts as download
        assert_bit_equal(b.residual(3, 2), res[3:5], "members 3..4")
        assert b.residual(batch, 0).shape == (0,)
        out = (C.c_float * batch)()
        h = b._h
        for args in ((-1, 1, 4), (0, batch + 1, 4 * (batch + 1)), (batch - 1, 2, 8), (0, -1, 0), (0, 2, 4), (0, 2, 12)):
            assert lib.sfl_batch_residual(h, args[0], args[1], out, args[2]) == cap.ERR_INVALID, args
        assert lib.sfl_batch_residual(h, 0, 2, None, 8) == cap.ERR_INVALID
        assert lib.sfl_batch_step_n_each(h, 1, None) == cap.ERR_INVALID and "NULL" in lib.sfl_last_error().decode()
        assert lib.sfl_batch_poisson_solve_each(h, None) == cap.ERR_INVALID
        assert lib.sfl_batch_step_n_each(h, -1, prm.ctypes.data_as(C.POINTER(cap.MemberParams))) == cap.ERR_INVALID
        assert_bit_equal(b.residual(), res, "the report survives refused calls")
        # iters = -1 in member 5: refused, naming it; the force queue and every field untouched
        upload_members(b, fields)
        b.queue_forces([5, 2], [(30, 40), (7, 9)], [(50.0, -20.0), (4.0, 4.0)])
        before = download_all(b)
        bad = prm.copy()
        bad["iters"][5] = -1
        bad["iters"][6] = -7
        for call in (lambda: b.step_n_each(1, bad), lambda: b.poisson_solve_each(bad), lambda: b.step_n_each(0, bad)):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == cap.ERR_INVALID and re.search(r"member 5\b", str(e.value)), str(e.value)
        after = download_all(b)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(after[k], before[k], f"{name} after refused calls")
        b.step_n_each(1, prm)                                      # looks unforced, applies the forces queued before
        got = download_all(b)
        forces = {5: [((30, 40), (50.0, -20.0))], 2: [((7, 9), (4.0, 4.0))]}
        for m in range(batch):
            want = context_run(s, before[0][m], before[3][m], prm[m], forces.get(m, ()))
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} after a refused call")
        with pytest.raises(ValueError):
            b.step_n_each(1, prm[:4])                              # a ready-made array of another batch's length


@pytest.mark.gpu
def test_parameters_and_reports_of_members_beyond_four_gigabytes_of_one_field(sfl):
    """61 x 81 x 73000 members: the dye alone is 4.33 GB (> 2^32 bytes).  Members 0 and B - 1 get parameters of their own."""
    dim_x, dim_y, batch = 61, 81, 73000
    assert batch * dim_x * dim_y * 12 > 2 ** 32
    forces = {0: [((30, 40), (40.0, -25.0))], batch - 1: [((12, 70), (-33.0, 18.0)), ((13, 70), (5.0, 5.0))]}
    prm = sfl.member_params(batch, 1 / 30.0, 1.0, 20, 1.96)
    for m, (dt, dx, iters, omega) in ((0, (1 / 60.0, 0.5, 33, 1.5)), (batch - 1, (0.1, 2.0, 9, 1.9))):
        prm["dt"][m], prm["dx"][m], prm["iters"][m], prm["omega"][m] = dt, dx, iters, omega
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.setup_sketch_fields()
        for m, fs in forces.items():
            b.queue_forces([m] * len(fs), [f[0] for f in fs], [f[1] for f in fs])
        b.step_n_each(1, prm)
        got = {m: [b.download(f, m, 1)[0] for f in (0, 2, 3, 1)] for m in (0, 1, batch - 2, batch - 1)}
        tail = b.residual(batch - 2, 2)
        head = b.residual(0, 2)
    for k, m in enumerate((batch - 2, batch - 1)):
        assert_report_equal(tail[k], update_norm(got[m][2], got[m][1], prm["dx"][m]), f"member {m}")
    for k, m in enumerate((0, 1)):
        assert_report_equal(head[k], update_norm(got[m][2], got[m][1], prm["dx"][m]), f"member {m}")
    assert tail[1] > 0 and head[0] > 0                # the forced members have something to report
    with sfl.Solver(dim_x, dim_y) as s:
        for m, fields in got.items():
            s.setup_sketch_fields()
            if m in forces:
                s.queue_forces(np.array([f[0] for f in forces[m]], np.int32), np.array([f[1] for f in forces[m]], np.float32))
            s.step_n(1, prm["dt"][m], prm["dx"][m], int(prm["iters"][m]), prm["omega"][m])
            s.synchronize()
            for k, name in enumerate(FIELDS):
                assert_bit_equal(fields[k], s.download((0, 2, 3, 1)[k]), f"{name}, member {m}")
