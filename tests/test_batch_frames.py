"""Frames of a batch (include/sfl.h group 4): sfl_batch_render_members, the draw task of many members in one launch, and the
recorder sfl_batch_record_*, which renders a frame every k-th step between the step launches.

The contract: every image is, bit for bit, what sfl_batch_render_rgb565 makes of the same member's dye -- and, where the dye
is member_fields' own (below 0xFF000000, so that every interpolated value stays inside [0, 2^32) where the oracle's
conversion is defined), what the oracle makes of it.  Runs that start from setup_sketch_fields hold 0xFFFFFFFF and are
compared with the existing GPU path only.  A recording changes nothing else about the step calls: a twin batch without a
recorder, stepped one step at a time and rendered member by member, is the yardstick.  The CPU tests need no GPU: argument
checks run before any device is touched."""
import ctypes as C

import numpy as np
import pytest

from conftest import assert_bit_equal
from test_batch import DT, FIELDS, OMEGA, download_all, member_fields, upload_members

FRAME_SYMBOLS = ["sfl_batch_render_members", "sfl_batch_record_start", "sfl_batch_record_stop", "sfl_batch_record_info",
                 "sfl_batch_record_read"]
TILE_EDGES = [15, 16, 17, 31, 32, 33, 63, 64, 65]   # cell blocks along an axis: one below, at and above any power-of-two tile
ITERS = 5


def _u16(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_frame_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in FRAME_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    for name in ("render_members", "record_start", "record_stop", "record_info", "frames"):
        assert hasattr(sfl.BatchSolver, name), name


def test_a_null_batch_is_refused_by_every_frame_call(sfl):
    lib = sfl.capi.lib()
    img = (C.c_uint16 * 4)()
    i, n = C.c_int(), C.c_int64()
    calls = [
        lambda: lib.sfl_batch_render_members(None, 0, 1, 1, 1, img, 8),
        lambda: lib.sfl_batch_record_start(None, 1, 0, 1, 1, 1, 1),
        lambda: lib.sfl_batch_record_stop(None),
        lambda: lib.sfl_batch_record_info(None, C.byref(i), C.byref(i), C.byref(n)),
        lambda: lib.sfl_batch_record_read(None, 0, 0, 1, img, 8),
    ]
    assert len(calls) == len(FRAME_SYMBOLS)
    for call in calls:
        assert call() == sfl.capi.ERR_INVALID
        assert "NULL" in lib.sfl_last_error().decode()


# ---- GPU, render_members ------------------------------------------------------------------------------
def check_render_members(sfl, oracle, dim_x, dim_y, batch, scalings, large=False, first=0, count=None, byteswaps=(True,), seed=0):
    """render_members of [first, first + count) against render_rgb565(m) and the oracle, image by image."""
    fields = [member_fields(dim_x, dim_y, 31 * seed + 7 * m + dim_x + 1000 * dim_y) for m in range(batch)]
    count = batch - first if count is None else count
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b:
        upload_members(b, fields)
        for scaling in scalings:
            for byteswap in byteswaps:
                got = b.render_members(first, count, scaling, byteswap)
                assert got.shape == (count, scaling * (dim_x - 1), scaling * (dim_y - 1)) and got.dtype == np.uint16
                for k in range(count):
                    what = f"{dim_x} x {dim_y}, scaling {scaling}, swap {byteswap}, member {first + k}"
                    assert_bit_equal(got[k], b.render_rgb565(first + k, scaling, byteswap), what + " against render_rgb565")
                    assert_bit_equal(got[k], oracle.render_rgb565(fields[first + k][1], scaling, byteswap), what + " against the oracle")
        assert b.render_members(first, 0).shape[0] == 0   # count == 0 does nothing


@pytest.mark.gpu
def test_one_block_and_the_longest_chains(sfl, oracle):
    check_render_members(sfl, oracle, 2, 2, 3, (1, 2, 3, 64))   # 1.0f / 3 is not exact; 63 sequential additions per lerp


@pytest.mark.gpu
def test_images_that_start_on_odd_pixels(sfl, oracle):
    # 9-pixel images: members 1 and 3 start on odd pixel offsets of the device buffer... and of the batch's images
    check_render_members(sfl, oracle, 4, 4, 5, (1,), first=1, count=3, byteswaps=(True, False))
    check_render_members(sfl, oracle, 4, 4, 5, (1,), byteswaps=(True, False))


@pytest.mark.gpu
@pytest.mark.parametrize("edge", TILE_EDGES)
def test_tile_edges(sfl, oracle, edge):
    """`edge` cell blocks along each axis in turn, against a short (2 blocks) and a long (70 blocks) other axis."""
    for dim_x, dim_y in ((edge + 1, 3), (edge + 1, 71), (3, edge + 1), (71, edge + 1)):
        check_render_members(sfl, oracle, dim_x, dim_y, 3, (4, 5), seed=edge)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (80, 60), (257, 23), (2047, 3), (2, 3072)])
def test_thin_shapes(sfl, oracle, dim_x, dim_y):
    check_render_members(sfl, oracle, dim_x, dim_y, 3, (4,))


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(128, 128), (160, 120), (142, 142)])
def test_large_members(sfl, oracle, dim_x, dim_y):
    check_render_members(sfl, oracle, dim_x, dim_y, 2, (4,), large=True)


@pytest.mark.gpu
def test_more_members_than_a_grid_dimension(sfl, oracle):
    """70000 members of 3 x 3: the member index must not live in gridDim.y (65535 at most).  The kernel's launch has at most
    65536 workgroups, which stride over the (member, tile) pairs: members 65536 .. 69999 are the loop's second pass."""
    dim_x, dim_y, batch, scaling = 3, 3, 70000, 2
    probes = (0, 65535, 65536, 69999)
    colour = np.random.default_rng(70000).integers(0, 0xFF000000, (batch, dim_y, dim_x, 3), dtype=np.uint32)
    for m in probes:
        colour[m] = member_fields(dim_x, dim_y, 70000 + m)[1]
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.upload(1, colour)
        got = b.render_members(0, batch, scaling)
        assert got.shape == (batch, 4, 4)
        for m in probes:
            assert_bit_equal(got[m], b.render_rgb565(m, scaling), f"member {m} against render_rgb565")
            assert_bit_equal(got[m], oracle.render_rgb565(colour[m], scaling), f"member {m} against the oracle")
        # ... and every other member, against the oracle's arithmetic on a sample across both sides of 65536
        for m in list(range(65500, 65600)) + list(range(0, batch, 997)):
            assert_bit_equal(got[m], oracle.render_rgb565(colour[m], scaling), f"member {m} against the oracle")


@pytest.mark.gpu
def test_one_frame_larger_than_4_gib(sfl):
    """1760 members of 61 x 81 at scaling 16: one frame is 1760 * 960 * 1280 * 2 = 4 325 376 000 bytes.  Members 0 and 1759 sit
    on either side of every 32-bit wrap of a byte offset (2^32) and of a signed pixel index (2^31 pixels = 2^32 bytes here).
    (A uint32 pixel index would wrap only at 8 GiB: the kernel's 64-bit member bases are checked by reading.)"""
    dim_x, dim_y, batch, scaling = 61, 81, 1760, 16
    assert batch * scaling * (dim_x - 1) * scaling * (dim_y - 1) * 2 > 2 ** 32
    distinct = [member_fields(dim_x, dim_y, 4096 + m, 40.0) for m in range(8)]
    reps = batch // 8
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        for field in (0, 1, 2):
            b.upload(field, np.tile(np.stack([f[field] for f in distinct]), (reps,) + (1,) * (distinct[0][field].ndim)))
        # capacity * count * H * W * 2 bytes past 2^64: refused, not allocated too small
        assert sfl.capi.lib().sfl_batch_record_start(b._h, 1, 0, batch, 64, 1, 2 ** 31 - 1) == sfl.capi.ERR_INVALID
        assert "capacity 2147483647" in sfl.capi.lib().sfl_last_error().decode()
        assert b.record_info() == (0, 0, 0)
        b.record_start(every=1, scaling=scaling, capacity=1)
        b.step_n(1, DT, 1.0, 1, OMEGA)
        assert b.record_info() == (1, 1, 1)
        got = {m: b.frames(0, 1, m, 1)[0, 0] for m in (0, batch - 1)}
    for m, image in got.items():
        with sfl.BatchSolver(dim_x, dim_y, 1) as twin:
            upload_members(twin, [distinct[m % 8]])
            twin.step_n(1, DT, 1.0, 1, OMEGA)
            assert_bit_equal(image, twin.render_rgb565(0, scaling), f"member {m} against a one-member twin")


# ---- GPU, recorder ------------------------------------------------------------------------------------
DIM_X, DIM_Y, BATCH = 61, 81, 5


def five_members(seed=300):
    return [member_fields(DIM_X, DIM_Y, seed + m, 40.0) for m in range(BATCH)]


def render_each(b, scaling=4, byteswap=True, first=0, count=None):
    """The yardstick: one sfl_batch_render_rgb565 per member."""
    count = b.batch - first if count is None else count
    return np.stack([b.render_rgb565(first + k, scaling, byteswap) for k in range(count)])


def assert_fields_equal(b, twin, what):
    for name, got, want in zip(FIELDS, download_all(b), download_all(twin)):
        assert_bit_equal(got, want, f"{what}: {name}")


def read_rc(sfl, b, frame, first, count, scaling=4):
    """The return code of a raw sfl_batch_record_read into a buffer of exactly the right size."""
    buf = np.empty(max(count, 0) * scaling * (b.dim_x - 1) * scaling * (b.dim_y - 1), np.uint16)
    return sfl.capi.lib().sfl_batch_record_read(b._h, frame, first, count, _u16(buf), buf.nbytes)


@pytest.mark.gpu
def test_recording_every_step(sfl, oracle):
    fields = five_members()
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin:
        upload_members(b, fields)
        upload_members(twin, fields)
        assert b.record_info() == (0, 0, 0)
        b.record_start(every=1, capacity=4)
        assert b.record_info() == (0, 4, 0)
        b.step_n(3, DT, 1.0, ITERS, OMEGA)
        assert b.record_info() == (3, 4, 3)
        got = b.frames()
        assert got.shape == (3, BATCH, 4 * (DIM_X - 1), 4 * (DIM_Y - 1))
        v, c = fields[2][0], fields[2][1]
        for f in range(3):
            twin.step_n(1, DT, 1.0, ITERS, OMEGA)
            assert_bit_equal(got[f], render_each(twin), f"frame {f} against the twin")
            v, _, _, c = oracle.step(v, c, DT, 1.0, ITERS, OMEGA)
            assert_bit_equal(got[f, 2], oracle.render_rgb565(c, 4, True), f"frame {f}, member 2 against the oracle")
        assert_fields_equal(b, twin, "after three recorded steps")
        assert_bit_equal(b.frames(1, 1, 3, 2)[0], got[1, 3:5], "frames are not consumed; a sub-range of members")


@pytest.mark.gpu
def test_recording_across_calls(sfl):
    """every = 3 across step_n(2), step_n_each(2), step_n_until(3): frames after steps 3 and 6, the reports of the last call."""
    fields = five_members(310)
    prm = sfl.member_params(BATCH, [DT, DT / 2, DT, DT * 2, DT], [1.0, 0.5, 1.0, 2.0, 1.0], [5, 9, 3, 7, 12], [1.96, 1.5, 1.0, 1.9, 1.7])
    stops = sfl.member_stops(BATCH, [1e-2, -1.0, 1e30, 1e-4, 1.0], [1, 2, 3, 4, 5])
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin, \
            sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as stepwise:
        for x in (b, twin, stepwise):
            upload_members(x, fields)
        b.record_start(every=3, capacity=5)
        for x in (b, twin):   # the twin: the same calls, no recorder
            x.step_n(2, DT, 1.0, ITERS, OMEGA)
            x.step_n_each(2, prm)
            x.step_n_until(3, prm, tol=stops)
        assert b.record_info() == (2, 5, 7)
        assert_bit_equal(b.residual(), twin.residual(), "the update norm")
        assert_bit_equal(b.iterations(), twin.iterations(), "the iterations")
        assert_fields_equal(b, twin, "after seven recorded steps")
        got, want = b.frames(), []
        assert got.shape[0] == 2
        one = [lambda: stepwise.step_n(1, DT, 1.0, ITERS, OMEGA)] * 2 + [lambda: stepwise.step_n_each(1, prm)] * 2 + \
              [lambda: stepwise.step_n_until(1, prm, tol=stops)] * 3
        for k, step in enumerate(one, 1):
            step()
            if k % 3 == 0:
                want.append(render_each(stepwise))
        assert_bit_equal(got, np.stack(want), "the frames after steps 3 and 6")
        assert_fields_equal(b, stepwise, "one step at a time")


@pytest.mark.gpu
def test_the_frames_follow_forces_queued_between_calls(sfl):
    fields = five_members(320)
    strokes = [([1, 3], [(30, 40), (20, 20)], [(900.0, -700.0), (-800.0, 600.0)]), ([1], [(31, 41)], [(-500.0, 900.0)])]
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin, \
            sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as calm:
        for x in (b, twin, calm):
            upload_members(x, fields)
        b.record_start(every=1, capacity=2)
        for f, stroke in enumerate(strokes):
            b.queue_forces(*stroke)
            b.step_n(1, DT, 1.0, ITERS, OMEGA)
            twin.queue_forces(*stroke)
            twin.step_n(1, DT, 1.0, ITERS, OMEGA)
            calm.step_n(1, DT, 1.0, ITERS, OMEGA)
            frame = b.frames(f, 1)[0]
            assert_bit_equal(frame, render_each(twin), f"frame {f} against the twin with the same forces")
            unforced = render_each(calm)
            assert not np.array_equal(frame[1], unforced[1]), "member 1's frame shows its force"
            assert_bit_equal(frame[0], unforced[0], "member 0 has none")
        assert_fields_equal(b, twin, "after two forced steps")


@pytest.mark.gpu
def test_a_recorded_sub_range(sfl):
    fields = five_members(330)
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin:
        upload_members(b, fields)
        upload_members(twin, fields)
        b.record_start(every=1, first=1, count=3, scaling=3, byteswap=False, capacity=2)
        b.step_n(2, DT, 1.0, ITERS, OMEGA)
        twin.step_n(2, DT, 1.0, ITERS, OMEGA)
        got = b.frames()
        assert got.shape == (2, 3, 3 * (DIM_X - 1), 3 * (DIM_Y - 1))
        assert_bit_equal(got[1], render_each(twin, 3, False, 1, 3), "members 1..3 of the second frame")
        assert_bit_equal(b.frames(1, 1, 2, 2)[0], got[1, 1:3], "members 2 and 3 by their batch numbers")
        lib = sfl.capi.lib()
        for first, count in ((0, 1), (4, 1), (0, 5), (3, 2), (1, -1)):
            assert read_rc(sfl, b, 0, first, count, 3) == sfl.capi.ERR_INVALID, (first, count)
            assert "recorded" in lib.sfl_last_error().decode()
        assert read_rc(sfl, b, 0, 1, 3, 3) == sfl.capi.OK


@pytest.mark.gpu
def test_a_full_recorder_refuses_the_whole_call(sfl):
    fields = five_members(340)
    stroke = ([2, 4], [(30, 40), (10, 70)], [(700.0, -300.0), (-200.0, 500.0)])
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin:
        upload_members(b, fields)
        upload_members(twin, fields)
        b.record_start(every=1, capacity=2)
        b.queue_forces(*stroke)
        with pytest.raises(sfl.SflError) as e:
            b.step_n(3, DT, 1.0, ITERS, OMEGA)
        assert e.value.code == sfl.capi.ERR_STATE
        assert "sfl_batch_record_read" in str(e.value) and "sfl_batch_record_start" in str(e.value)
        assert b.record_info() == (0, 2, 0)
        assert_fields_equal(b, twin, "after the refused call")
        # the queue is untouched: the next step applies the forces exactly as the twin's does
        b.step_n(1, DT, 1.0, ITERS, OMEGA)
        twin.queue_forces(*stroke)
        twin.step_n(1, DT, 1.0, ITERS, OMEGA)
        assert_fields_equal(b, twin, "the queued forces went into the next step")
        prm = sfl.member_params(BATCH, DT, 1.0, ITERS, OMEGA)
        b.step_n_each(1, prm)
        twin.step_n_each(1, prm)
        assert b.record_info() == (2, 2, 2)
        residual = b.residual()
        for refused in (lambda: b.step_n(1, DT, 1.0, ITERS, OMEGA), lambda: b.step_n_each(1, prm),
                        lambda: b.step_n_until(1, prm, tol=1e-3)):
            with pytest.raises(sfl.SflError) as e:
                refused()
            assert e.value.code == sfl.capi.ERR_STATE
        assert b.record_info() == (2, 2, 2)
        assert_bit_equal(b.residual(), residual, "a refused call leaves the reports valid")
        assert_fields_equal(b, twin, "after three refused calls")
        b.step_n(0, DT, 1.0, ITERS, OMEGA)   # n == 0 completes no frame
        assert_bit_equal(b.frames()[1], render_each(twin), "the second frame")
        b.record_start(every=1, capacity=2)   # makes room
        b.step_n(1, DT, 1.0, ITERS, OMEGA)
        twin.step_n(1, DT, 1.0, ITERS, OMEGA)
        assert b.record_info() == (1, 2, 1)
        assert_bit_equal(b.frames()[0], render_each(twin), "the first frame after the restart")


@pytest.mark.gpu
def test_restart_and_stop(sfl):
    fields = five_members(350)
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b, sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as twin:
        upload_members(b, fields)
        upload_members(twin, fields)
        b.record_start(every=2, capacity=3)
        b.step_n(3, DT, 1.0, ITERS, OMEGA)
        twin.step_n(3, DT, 1.0, ITERS, OMEGA)
        assert b.record_info() == (1, 3, 3)
        # solves, uploads and setup_sketch_fields do not advance the count
        b.poisson_solve(1.0, 3, OMEGA)
        b.poisson_solve_each(1.0, 3, OMEGA)
        b.poisson_solve_until(1.0, 3, OMEGA, tol=1e-3)
        b.upload(3, b.download(3))
        assert b.record_info() == (1, 3, 3)
        b.record_start(every=1, scaling=2, capacity=2)   # while recording: afresh, other parameters
        assert b.record_info() == (0, 2, 0)
        assert read_rc(sfl, b, 0, 0, BATCH, 2) == sfl.capi.ERR_INVALID   # the earlier frames are dropped
        twin.poisson_solve(1.0, 3, OMEGA)
        for x in (b, twin):
            x.step_n(1, DT, 1.0, ITERS, OMEGA)
        assert b.record_info() == (1, 2, 1)
        assert_bit_equal(b.frames()[0], render_each(twin, 2), "the first frame of the second recording")
        b.record_stop()
        assert b.record_info() == (0, 0, 0)
        assert read_rc(sfl, b, 0, 0, BATCH, 2) == sfl.capi.ERR_STATE
        assert "sfl_batch_record_start" in sfl.capi.lib().sfl_last_error().decode()
        for x in (b, twin):
            x.step_n(2, DT, 1.0, ITERS, OMEGA)   # records nothing, refuses nothing
        assert b.record_info() == (0, 0, 0)
        assert_fields_equal(b, twin, "after the recorder stopped")
        b.record_stop()   # not recording: SFL_OK
        b.record_start(every=1, capacity=1)
        b.setup_sketch_fields()
        assert b.record_info() == (0, 1, 0)


@pytest.mark.gpu
def test_recording_a_large_batch_from_the_sketch_start(sfl):
    dim_x, dim_y, batch = 128, 128, 2
    drags = ([0, 1, 1], [(64, 64), (30, 90), (31, 90)], [(30.0, -12.0), (-25.0, 9.0), (2.0, 2.0)])
    with sfl.BatchSolver(dim_x, dim_y, batch, large=True) as b, sfl.BatchSolver(dim_x, dim_y, batch, large=True) as twin:
        want = []
        for x in (b, twin):
            x.setup_sketch_fields()
            x.queue_forces(*drags)
        b.record_start(every=2, capacity=2)
        b.step_n(4, DT, 1.0, ITERS, OMEGA)
        for k in range(1, 5):
            twin.step_n(1, DT, 1.0, ITERS, OMEGA)
            if k % 2 == 0:
                want.append(render_each(twin))
        assert b.record_info() == (2, 2, 4)
        assert_bit_equal(b.frames(), np.stack(want), "the frames after steps 2 and 4")
        assert_bit_equal(b.render_members(), want[1], "render_members of the dye the fourth step left")
        assert_fields_equal(b, twin, "after four recorded steps")


@pytest.mark.gpu
def test_every_refusal_comes_before_any_gpu_work(sfl):
    fields = five_members(360)
    lib, INVALID = sfl.capi.lib(), sfl.capi.ERR_INVALID
    h, w = 4 * (DIM_X - 1), 4 * (DIM_Y - 1)
    img = np.zeros((BATCH, h, w), np.uint16)
    with sfl.BatchSolver(DIM_X, DIM_Y, BATCH) as b:
        upload_members(b, fields)
        b.record_start(every=2, first=1, count=3, capacity=2)
        b.step_n(2, DT, 1.0, ITERS, OMEGA)
        before, state, frame = download_all(b), b.record_info(), b.frames()
        one = img[0].nbytes
        refusals = [   # (call, what its message names)
            (lambda: lib.sfl_batch_render_members(b._h, 0, 1, 0, 1, _u16(img), 0), "scaling must be 1..64 (got 0)"),
            (lambda: lib.sfl_batch_render_members(b._h, 0, 1, 65, 1, _u16(img), one), "scaling must be 1..64 (got 65)"),
            (lambda: lib.sfl_batch_render_members(b._h, -1, 1, 4, 1, _u16(img), one), "[-1, -1 + 1)"),
            (lambda: lib.sfl_batch_render_members(b._h, 4, 2, 4, 1, _u16(img), 2 * one), "[4, 4 + 2)"),
            (lambda: lib.sfl_batch_render_members(b._h, 0, -1, 4, 1, _u16(img), 0), "[0, 0 + -1)"),
            (lambda: lib.sfl_batch_render_members(b._h, 0, 2, 4, 1, _u16(img), 2 * one - 2), f"got {2 * one - 2}"),
            (lambda: lib.sfl_batch_render_members(b._h, 0, 2, 4, 1, None, 2 * one), "host_images is NULL"),
            (lambda: lib.sfl_batch_record_start(b._h, 0, 0, 5, 4, 1, 2), "every must be >= 1 (got 0)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, 0, 5, 4, 1, 0), "capacity must be >= 1 (got 0)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, 0, 5, 0, 1, 2), "scaling must be 1..64 (got 0)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, 0, 5, 65, 1, 2), "scaling must be 1..64 (got 65)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, 0, 0, 4, 1, 2), "count must be >= 1 (got 0)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, 3, 3, 4, 1, 2), "[3, 3 + 3)"),
            (lambda: lib.sfl_batch_record_start(b._h, 1, -1, 2, 4, 1, 2), "[-1, -1 + 2)"),
            (lambda: lib.sfl_batch_record_read(b._h, 1, 1, 1, _u16(img), one), "frame 1"),
            (lambda: lib.sfl_batch_record_read(b._h, -1, 1, 1, _u16(img), one), "frame -1"),
            (lambda: lib.sfl_batch_record_read(b._h, 0, 0, 1, _u16(img), one), "[0, 0 + 1)"),
            (lambda: lib.sfl_batch_record_read(b._h, 0, 3, 2, _u16(img), 2 * one), "[3, 3 + 2)"),
            (lambda: lib.sfl_batch_record_read(b._h, 0, 1, 2, _u16(img), one), f"got {one}"),
            (lambda: lib.sfl_batch_record_read(b._h, 0, 1, 2, None, 2 * one), "host is NULL"),
        ]
        for k, (call, names) in enumerate(refusals):
            assert call() == INVALID, k
            assert names in lib.sfl_last_error().decode(), (k, lib.sfl_last_error().decode())
        assert not img.any(), "no refused call wrote an image"
        assert lib.sfl_batch_record_info(b._h, None, None, None) == sfl.capi.OK   # any out may be NULL
        assert b.record_info() == state == (1, 2, 2)
        assert_bit_equal(b.frames(), frame, "the recording is as it was")
        for name, got, want in zip(FIELDS, download_all(b), before):
            assert_bit_equal(got, want, f"{name} after the refusals")
        for bad in (lambda: b.step_n(-1, DT, 1.0, ITERS, OMEGA), lambda: b.step_n(5, DT, 1.0, -1, OMEGA)):
            with pytest.raises(sfl.SflError) as e:   # the call's own argument checks come first
                bad()
            assert e.value.code == INVALID
