"""Batches (include/sfl.h group 4, sfl_batch_*): many independent small grids of one shape stepped by one launch.

The contract under test: after any sequence of batch calls member m holds, bit for bit, what a whole-domain context of
the same shape holds after the same calls made with member m's data and forces -- checked against the oracle and
against single contexts.  The CPU tests need no GPU: argument checks run before any device is touched."""
import ctypes as C
import re

import numpy as np
import pytest

from conftest import assert_bit_equal

DT = np.float32(1 / 30.0)
OMEGA = np.float32(1.96)
FIELDS = ("velocity", "divergence", "pressure", "colour")
BATCH_SYMBOLS = ["sfl_batch_create", "sfl_batch_destroy", "sfl_batch_shape", "sfl_batch_upload", "sfl_batch_download",
                 "sfl_batch_field_device_ptr", "sfl_batch_queue_forces", "sfl_batch_step_n", "sfl_batch_poisson_solve",
                 "sfl_batch_setup_sketch_fields", "sfl_batch_render_rgb565", "sfl_batch_synchronize"]
# the shapes of test_gpu_parity.SMALL_SHAPES that a batch member may take (6144 cells, 3072 of one colour)
BATCH_SHAPES = [(2, 2), (3, 3), (61, 81), (80, 60), (78, 78), (128, 48), (257, 23), (2047, 3), (2, 3072)]


# ---- CPU ----------------------------------------------------------------------------------------------
def test_every_batch_symbol_is_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in BATCH_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    assert hasattr(sfl, "BatchSolver")


@pytest.mark.parametrize("dims,limit", [
    ((1, 81, 4), "dim_x and dim_y must be >= 2"),
    ((61, 1, 4), "dim_x and dim_y must be >= 2"),
    ((61, 81, 0), "batch must be >= 1"),
    ((1229, 5, 1), "at most 6144 cells"),                # 6145 cells
    ((3, 2048, 1), "at most 3072 cells of one colour"),  # 6144 cells, 4096 of one colour
    ((64, 64, 524288), "2^31 - 1"),                      # batch x cells = 2^31
])
def test_create_refuses_what_does_not_fit_before_touching_a_gpu(sfl, dims, limit):
    lib = sfl.capi.lib()
    h = C.c_void_p()
    assert lib.sfl_batch_create(C.byref(h), 0, *dims) == sfl.capi.ERR_INVALID
    assert limit in lib.sfl_last_error().decode()
    assert not h.value


def test_null_handles_and_pointers_are_refused(sfl):
    lib = sfl.capi.lib()
    assert lib.sfl_batch_create(None, 0, 61, 81, 4) == sfl.capi.ERR_INVALID
    assert "NULL" in lib.sfl_last_error().decode()
    buf = (C.c_uint8 * 64)()
    i, img = C.c_int(), (C.c_uint16 * 4)()
    calls = [
        lambda: lib.sfl_batch_destroy(None),
        lambda: lib.sfl_batch_shape(None, C.byref(i), C.byref(i), C.byref(i)),
        lambda: lib.sfl_batch_upload(None, 0, 0, 1, buf, 64),
        lambda: lib.sfl_batch_download(None, 0, 0, 1, buf, 64),
        lambda: lib.sfl_batch_field_device_ptr(None, 0, C.byref(C.c_void_p())),
        lambda: lib.sfl_batch_queue_forces(None, None, None, None, 0),
        lambda: lib.sfl_batch_step_n(None, 1, 0.1, 1.0, 5, 1.9),
        lambda: lib.sfl_batch_poisson_solve(None, 1.0, 5, 1.9),
        lambda: lib.sfl_batch_setup_sketch_fields(None),
        lambda: lib.sfl_batch_render_rgb565(None, 0, 1, 1, img, 8),
        lambda: lib.sfl_batch_synchronize(None),
    ]
    assert len(calls) == len(BATCH_SYMBOLS) - 1
    for call in calls:
        assert call() == sfl.capi.ERR_INVALID


def test_a_valid_batch_without_a_device_fails_loudly(sfl):
    if sfl.device_count() > 0:
        pytest.skip("a GPU is present: the create succeeds (the GPU tests below use it)")
    with pytest.raises(sfl.SflError) as e:
        sfl.BatchSolver(61, 81, 4)
    assert e.value.code == sfl.capi.ERR_HIP   # no CPU fallback


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


def solver_run(s, v, c, forces=(), steps=1, iters=5, dx=1.0, drags=None):
    """A single context's answer: upload, queue forces, step_n."""
    s.upload(0, v)
    s.upload(1, c)
    if forces:
        cells, vel = zip(*forces)
        s.queue_forces(np.array(cells, np.int32), np.array(vel, np.float32))
    s.step_n(steps, DT, dx, iters, OMEGA)
    s.synchronize()
    return [s.download(f) for f in (0, 2, 3, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", BATCH_SHAPES)
@pytest.mark.parametrize("batch", [1, 3, 37])
def test_every_member_equals_the_oracle(sfl, oracle, dim_x, dim_y, batch):
    fields = [member_fields(dim_x, dim_y, 1000 * batch + 7 * m + dim_x) for m in range(batch)]
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        assert b.shape == (dim_x, dim_y, batch)
        for iters, dx in ((9, 1.0), (1, 0.5), (0, 1.0)):
            upload_members(b, fields)
            b.poisson_solve(dx, iters, OMEGA)
            b.synchronize()
            p = b.download(3)
            for m, (_, _, d) in enumerate(fields):
                assert_bit_equal(p[m], oracle.poisson_solve(d, dx, iters, OMEGA), f"solve, member {m}, iters {iters}")
            b.step_n(1, DT, dx, iters, OMEGA)
            b.synchronize()
            got = download_all(b)
            for m, (v, c, _) in enumerate(fields):
                want = oracle.step(v, c, DT, dx, iters, OMEGA)
                for k, name in enumerate(FIELDS):
                    assert_bit_equal(got[k][m], want[k], f"{name}, member {m}, iters {iters}, dx {dx}")


@pytest.mark.gpu
def test_257_members_with_forces_equal_single_contexts(sfl):
    dim_x, dim_y, batch = 61, 81, 257
    fields = [member_fields(dim_x, dim_y, 5000 + m, 40.0) for m in range(batch)]
    forces = {
        0: [((30, 40), (55.0, -35.0)), ((30, 40), (-8.0, 6.0)), ((0, 0), (3.0, 4.0))],   # the same cell twice: last wins
        128: [((dim_x, 5), (99.0, 99.0)), ((60, 80), (-20.0, 10.0))],                   # (dim_x, 5) lies outside: skipped
        256: [((10, 70), (12.0, -7.0)), ((11, 70), (1.5, 2.5))],
    }
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        upload_members(b, fields)
        records = [(m, cell, vel) for m in (0, 128, 256) for cell, vel in forces[m]]
        for part in (records[:4], records[4:]):   # queued in two calls, interleaved members
            b.queue_forces([r[0] for r in part], [r[1] for r in part], [r[2] for r in part])
        b.step_n(3, DT, 1.0, 9, OMEGA)
        b.synchronize()
        got = download_all(b)
    with sfl.Solver(dim_x, dim_y) as s:
        for m, (v, c, _) in enumerate(fields):
            want = solver_run(s, v, c, forces.get(m, ()), steps=3, iters=9)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m}")


def oracle_forced_step(oracle, v, c, cells_vel, iters):
    """One step of the oracle with point forces between the velocity advection and the divergence (ino:264-269)."""
    v1 = oracle.advect_vec2f(v, v, DT, True)
    for (i, j), f in cells_vel:
        if 0 <= i < v.shape[1] and 0 <= j < v.shape[0]:
            v1[j, i] = f
    d = oracle.divergence(v1, 1.0)
    p = oracle.poisson_solve(d, 1.0, iters, OMEGA)
    return oracle.subtract_gradient(v1, p, 1.0), d, p


@pytest.mark.gpu
def test_the_sketch_start_with_drags(sfl, oracle):
    """setup_sketch_fields on every member, drags (the sketch's transform, ino:264-269) on two, five steps."""
    dim_x, dim_y, batch, steps, iters = 61, 81, 16, 5, 20
    drags = {3: [(40, 20, 30.0, -12.0)], 11: [(5, 50, -25.0, 9.0), (6, 50, 2.0, 2.0)]}   # graphics coords (x, y), vel (x, y)
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.setup_sketch_fields()
        for m, ds in drags.items():   # cell = (coords.y, coords.x), velocity = (vel.y, vel.x)
            b.queue_forces([m] * len(ds), [(y, x) for x, y, _, _ in ds], [(vy, vx) for _, _, vx, vy in ds])
        b.step_n(steps, DT, 1.0, iters, OMEGA)
        b.synchronize()
        got = download_all(b)
    v0 = np.zeros((dim_y, dim_x, 2), np.float32)
    with sfl.Solver(dim_x, dim_y) as s:
        for m in range(batch):
            s.setup_sketch_fields()
            if m in drags:
                s.queue_drags(drags[m])
            s.step_n(steps, DT, 1.0, iters, OMEGA)
            s.synchronize()
            want = [s.download(f) for f in (0, 2, 3, 1)]
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, member {m} against a context")
            # velocity, divergence and pressure do not depend on the dye: the oracle too
            cells_vel = [((y, x), (vy, vx)) for x, y, vx, vy in drags.get(m, [])]
            v, d, p = oracle_forced_step(oracle, v0, None, cells_vel, iters)
            c = oracle.setup_fields(dim_x, dim_y)[1]
            for _ in range(steps - 1):
                v, d, p, c = oracle.step(v, c, DT, 1.0, iters, OMEGA)
            for k, (name, w) in enumerate(zip(FIELDS, (v, d, p))):
                assert_bit_equal(got[k][m], w, f"{name}, member {m} against the oracle")


@pytest.mark.gpu
def test_render_of_one_member(sfl, oracle):
    dim_x, dim_y, batch = 61, 81, 5
    fields = [member_fields(dim_x, dim_y, 900 + m) for m in range(batch)]
    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.Solver(dim_x, dim_y) as s:
        upload_members(b, fields)
        for m in (0, 2, 4):
            for scaling, byteswap in ((4, True), (1, False)):
                got = b.render_rgb565(m, scaling, byteswap)
                s.upload(1, fields[m][1])
                assert_bit_equal(got, s.render_rgb565(scaling, byteswap), f"member {m} against a context")
                assert_bit_equal(got, oracle.render_rgb565(fields[m][1], scaling, byteswap), f"member {m} against the oracle")
        with pytest.raises(sfl.SflError):
            b.render_rgb565(batch)


@pytest.mark.gpu
def test_members_are_isolated_and_io_checks_its_ranges(sfl):
    dim_x, dim_y, batch = 61, 81, 5
    rng = np.random.default_rng(77)
    loud = [(rng.uniform(-1, 1, (dim_y, dim_x, 2)) * 1e4).astype(np.float32) for _ in range(batch)]
    v = np.stack([loud[m] if m % 2 == 0 else np.zeros_like(loud[m]) for m in range(batch)])
    c = np.stack([rng.integers(0, 2 ** 32, (dim_y, dim_x, 3), dtype=np.uint32) if m % 2 == 0 else
                  np.zeros((dim_y, dim_x, 3), np.uint32) for m in range(batch)])
    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.Solver(dim_x, dim_y) as s:
        b.upload(0, v)
        b.upload(1, c)
        b.step_n(2, DT, 1.0, 20, OMEGA)
        b.synchronize()
        got = download_all(b)
        want = solver_run(s, v[1], c[1], steps=2, iters=20)
        for m in (1, 3):   # quiet members between loud ones: every value +-0, exactly as a context from zero fields
            for k, name in enumerate(FIELDS):
                assert_bit_equal(got[k][m], want[k], f"{name}, quiet member {m}")
                assert not np.any(got[k][m])
        # member-range round trip
        d = rng.standard_normal((2, dim_y, dim_x)).astype(np.float32)
        b.upload(2, d, first=2)
        assert_bit_equal(b.download(2, 2, 2), d, "divergence members 2..3")
        assert_bit_equal(b.download(0, 1, 3), got[0][1:4], "velocity members 1..3")
        # refused: a range beyond the batch, a wrong byte count, a member out of range (nothing queued)
        with pytest.raises(sfl.SflError):
            b.download(0, 4, 2)
        with pytest.raises(sfl.SflError):
            b.upload(2, d, first=4)
        lib, h = sfl.capi.lib(), b._h
        assert lib.sfl_batch_upload(h, 2, 0, 1, d.ctypes.data, d[0].nbytes - 4) == sfl.capi.ERR_INVALID
        assert lib.sfl_batch_download(h, 3, 0, 2, d.ctypes.data, d[0].nbytes) == sfl.capi.ERR_INVALID
        before = download_all(b)
        with pytest.raises(sfl.SflError) as e:
            b.queue_forces([0, batch], [(3, 3), (4, 4)], [(50.0, 50.0), (60.0, 60.0)])
        assert re.search(r"member %d" % batch, str(e.value))
        b.step_n(1, DT, 1.0, 5, OMEGA)
        b.synchronize()
        after = download_all(b)
        for m in range(batch):   # the next step is an unforced one
            want = solver_run(s, before[0][m], before[3][m], steps=1, iters=5)
            for k, name in enumerate(FIELDS):
                assert_bit_equal(after[k][m], want[k], f"{name}, member {m} after a refused queue")


@pytest.mark.gpu
def test_members_beyond_four_gigabytes_of_one_field(sfl):
    """61 x 81 x 73000 members: the dye alone is 4.33 GB (> 2^32 bytes), ~17.3 GB of fields in all."""
    dim_x, dim_y, batch = 61, 81, 73000
    assert batch * dim_x * dim_y * 12 > 2 ** 32
    forces = {0: [((30, 40), (40.0, -25.0))], batch - 1: [((12, 70), (-33.0, 18.0)), ((13, 70), (5.0, 5.0))]}
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.setup_sketch_fields()
        for m, fs in forces.items():
            b.queue_forces([m] * len(fs), [f[0] for f in fs], [f[1] for f in fs])
        b.step_n(1, DT, 1.0, 20, OMEGA)
        b.synchronize()
        got = {m: [b.download(f, m, 1)[0] for f in (0, 2, 3, 1)] for m in (0, 1, batch - 2, batch - 1)}
    with sfl.Solver(dim_x, dim_y) as s:
        for m, fields in got.items():
            s.setup_sketch_fields()
            if m in forces:
                s.queue_forces(np.array([f[0] for f in forces[m]], np.int32), np.array([f[1] for f in forces[m]], np.float32))
            s.step_n(1, DT, 1.0, 20, OMEGA)
            s.synchronize()
            for k, name in enumerate(FIELDS):
                assert_bit_equal(fields[k], s.download((0, 2, 3, 1)[k]), f"{name}, member {m}")
