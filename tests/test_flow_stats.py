"""Flow statistics of contexts and batches (sfl_flow_stats, sfl_batch_flow_stats, sfl_batch_flow_stats_each): the maxima of
|v.x|, |v.y| and |calculate_divergence(v, dx)| and the exact per-channel dye sums of the fields the library holds.

The contract under test (include/sfl.h): every figure is, bit for bit, what numpy and the oracle give on the downloaded
fields -- maxima and integer sums do not depend on the order of reduction, so there is no tolerance anywhere; a NaN matches
any NaN.  The yardstick is `yardstick` below: np.max(np.abs(.)) (which propagates NaN) of the two components and of the
oracle's divergence (pinned to the compiled reference by the parity tests), and a uint64 sum.

Shapes: those of test_context_until.py -- the one-workgroup shapes and the general ones; odd and even widths (rows that are
and are not 16-byte aligned), widths below, at no multiple of and beyond the velocity kernel's 128-column strips, heights
that are no multiple of its 8-row chunks, two columns, three rows."""
import ctypes as C
import functools

import numpy as np
import pytest

from conftest import assert_bit_equal, random_fields
from test_batch_params import assert_report_equal

SYMBOLS = ["sfl_flow_stats", "sfl_batch_flow_stats", "sfl_batch_flow_stats_each"]
SHAPES = [(2, 2), (3, 3), (61, 81), (130, 70), (96, 65), (257, 130), (512, 96), (1030, 67), (2, 4000), (3073, 3)]
SPEEDS = ("max_abs_vx", "max_abs_vy")


# ---- the yardstick ------------------------------------------------------------------------------------
def yardstick(oracle, v, c, dx=1.0):
    """(max |v.x|, max |v.y|, max |div|, dye sums) of host fields; v or c may be None."""
    out = [np.float32(0), np.float32(0), np.float32(0), np.zeros(3, np.uint64)]
    with np.errstate(all="ignore"):
        if v is not None:
            out[0], out[1] = np.max(np.abs(v[..., 0])), np.max(np.abs(v[..., 1]))
            out[2] = np.max(np.abs(oracle.divergence(v, np.float32(dx))))
        if c is not None:
            out[3] = c.astype(np.uint64).sum(axis=(0, 1))
    return out


def assert_stats(got, want, what, velocity=True, dye=True):
    """One record against a yardstick tuple: bit for bit; the members not asked for are zero."""
    print(f"{what}: got {got}, want {want}")
    bits = (1 if velocity else 0) | (2 if dye else 0)
    assert int(got["what"]) == bits, (what, got["what"])
    for k, name in enumerate(SPEEDS + ("max_abs_div",)):
        assert_report_equal(got[name], want[k] if velocity else np.float32(0), f"{what}: {name}")
    assert got["dye_sum"].dtype == np.uint64
    assert [int(x) for x in got["dye_sum"]] == [int(x) for x in (want[3] if dye else np.zeros(3, np.uint64))], f"{what}: dye_sum"


@functools.lru_cache(maxsize=None)
def fields(dim_x, dim_y, seed=0):
    """A random velocity (|v| <= 100) and a dye drawn over the whole UQ32 range.  Shared: never written to."""
    v, _, _ = random_fields(dim_x, dim_y, 100 + dim_x + seed)
    c = np.random.default_rng(7 + dim_x + seed).integers(0, 2 ** 32, (dim_y, dim_x, 3), dtype=np.uint32)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def spike_cells(sfl, dim_x, dim_y):
    """The four corners, the middle of each edge, the cells on both sides of the first internal strip boundary of the
    velocity kernel (columns 127 | 128, in a middle row) and on both sides of its first internal row-chunk boundary (rows
    7 | 8, in a middle column) where the grid has them.  The constants are the library's own (solver.py, from
    csrc/stats_kernels.h)."""
    strip, chunk = sfl.FLOW_STATS_STRIP_COLS, sfl.FLOW_STATS_CHUNK_ROWS
    assert (strip, chunk) == (128, 8)
    mx, my = dim_x // 2, dim_y // 2
    cells = [(0, 0), (dim_x - 1, 0), (0, dim_y - 1), (dim_x - 1, dim_y - 1), (mx, 0), (mx, dim_y - 1), (0, my), (dim_x - 1, my)]
    if dim_x > strip:
        cells += [(strip - 1, my), (strip, my)]
    if dim_y > chunk:
        cells += [(mx, chunk - 1), (mx, chunk)]
    return sorted(set(cells))


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    want = {"sfl_flow_stats": [C.c_void_p, C.c_int, C.c_float, C.POINTER(cap.FlowStats)],
            "sfl_batch_flow_stats": [C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_int, C.POINTER(cap.FlowStats), C.c_size_t],
            "sfl_batch_flow_stats_each": [C.c_void_p, C.c_int, C.POINTER(cap.MemberParams), C.c_int, C.c_int,
                                          C.POINTER(cap.FlowStats), C.c_size_t]}
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, want[name]), name     # the header's argument types
        assert getattr(lib, name).argtypes == want[name] and getattr(lib, name).restype == C.c_int
    assert (cap.STATS_VELOCITY, cap.STATS_DYE) == (1, 2)
    assert C.sizeof(cap.FlowStats) == 40
    offsets = {"max_abs_vx": 0, "max_abs_vy": 4, "max_abs_div": 8, "what": 12, "dye_sum": 16}
    for name, offset in offsets.items():
        assert getattr(cap.FlowStats, name).offset == offset, name
        assert sfl.FLOW_STATS_DTYPE.fields[name][1] == offset, name
    assert sfl.FLOW_STATS_DTYPE.itemsize == 40 and sfl.FLOW_STATS_DTYPE.names == tuple(offsets)
    assert sfl.FLOW_STATS_DTYPE["dye_sum"] == np.dtype(("<u8", (3,))) and sfl.FLOW_STATS_DTYPE["what"] == np.dtype("<u4")
    assert all(sfl.FLOW_STATS_DTYPE[n] == np.dtype("<f4") for n in SPEEDS + ("max_abs_div",))
    assert hasattr(sfl.Solver, "flow_stats") and hasattr(sfl.BatchSolver, "flow_stats")
    assert lib.sfl_abi_version() == 1


def test_bad_arguments_are_refused_without_a_gpu(sfl):
    """Every check that needs no context comes first, so each answers with its own message on a box with no GPU."""
    lib, cap = sfl.capi.lib(), sfl.capi
    out, prm = (cap.FlowStats * 2)(), (cap.MemberParams * 2)()
    refusals = [
        (lambda: lib.sfl_flow_stats(None, 3, 1.0, out), "NULL"),
        (lambda: lib.sfl_flow_stats(None, 0, 1.0, out), "what"),
        (lambda: lib.sfl_flow_stats(None, 4, 1.0, out), "what"),
        (lambda: lib.sfl_flow_stats(None, 7, 1.0, out), "what"),
        (lambda: lib.sfl_batch_flow_stats(None, 3, 1.0, 0, 2, out, 80), "NULL"),
        (lambda: lib.sfl_batch_flow_stats(None, 0, 1.0, 0, 2, out, 80), "what"),
        (lambda: lib.sfl_batch_flow_stats(None, 4, 1.0, 0, 2, out, 80), "what"),
        (lambda: lib.sfl_batch_flow_stats(None, 3, 1.0, 0, 2, out, 79), "80 bytes"),
        (lambda: lib.sfl_batch_flow_stats(None, 3, 1.0, 0, 2, out, 40), "80 bytes"),
        (lambda: lib.sfl_batch_flow_stats(None, 3, 1.0, 0, -1, out, 0), "bytes"),
        (lambda: lib.sfl_batch_flow_stats_each(None, 3, prm, 0, 2, out, 80), "NULL"),
        (lambda: lib.sfl_batch_flow_stats_each(None, 0, prm, 0, 2, out, 80), "what"),
        (lambda: lib.sfl_batch_flow_stats_each(None, 4, prm, 0, 2, out, 80), "what"),
        (lambda: lib.sfl_batch_flow_stats_each(None, 2, prm, 0, 2, out, 84), "80 bytes")]
    for k, (call, word) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert word in lib.sfl_last_error().decode(), (k, word, lib.sfl_last_error())
    with pytest.raises(ValueError):
        sfl.Solver.flow_stats(object(), velocity=False, dye=False)


def test_the_longest_back_trace_is_the_maximum_speed_times_dt():
    """advect.h:78-80 traces cell c back by v(c) * dt.  Float rounding is monotone and symmetric in sign, so the maximum of
    |v(c) * dt| over the cells is |max|v| * dt|, bit for bit: max_abs_vx (max_abs_vy) is the back-trace figure for any dt."""
    rng = np.random.default_rng(5)
    tiny = np.float32(1.4e-45)
    samples = {
        "random": (rng.standard_normal(4099) * 100).astype(np.float32),
        "every scale": (rng.standard_normal(4099) * 10.0 ** rng.integers(-44, 38, 4099)).astype(np.float32),
        "denormals": (rng.integers(-2 ** 22, 2 ** 22, 999).astype(np.float32) * tiny),
        "signed zeros": np.array([0.0, -0.0, -0.0], np.float32),
        "zeros and a denormal": np.array([-0.0, 0.0, -tiny], np.float32),
        "+inf": np.array([1.0, np.inf, -3.0], np.float32),
        "-inf": np.array([1.0, -np.inf, 2.0], np.float32),
        "a negative maximum": np.array([1.0, -7.5, 2.0], np.float32),
        "the largest finite": np.array([3.4028235e38, -1.0], np.float32),
    }
    with np.errstate(all="ignore"):
        for name, x in samples.items():
            assert x.dtype == np.float32
            top = np.max(np.abs(x))
            for dt in (1.0, 1 / 30, 0.1, -0.1, 3.0, 1e-3, 1e30, 1e-30, 2.0 ** -140, 1.9999999):
                dt = np.float32(dt)
                lhs, rhs = np.max(np.abs(x * dt)), np.abs(top * dt)
                assert lhs.dtype == rhs.dtype == np.float32
                assert lhs.view(np.uint32) == rhs.view(np.uint32), (name, dt, lhs, rhs)


# ---- GPU: contexts ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_random_fields_each_part_alone_and_both(sfl, oracle, dim_x, dim_y):
    v, c = fields(dim_x, dim_y)
    with sfl.Solver(dim_x, dim_y) as s:
        assert_stats(s.flow_stats(), yardstick(oracle, np.zeros_like(v), np.zeros_like(c)), "a fresh context")
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
        for dx in (1.0, 0.5):
            want = yardstick(oracle, v, c, dx)
            assert_stats(s.flow_stats(dx), want, f"{dim_x} x {dim_y}, dx {dx}, both")
            assert_stats(s.flow_stats(dx, dye=False), want, f"{dim_x} x {dim_y}, dx {dx}, velocity", dye=False)
            assert_stats(s.flow_stats(dx, velocity=False), want, f"{dim_x} x {dim_y}, dx {dx}, dye", velocity=False)
        assert_stats(s.flow_stats(float("nan"), velocity=False), want, "dye alone ignores dx", velocity=False)
        assert_bit_equal(s.download(sfl.capi.FIELD_VELOCITY), v, "velocity after flow_stats()")   # the call reads only
        assert_bit_equal(s.download(sfl.capi.FIELD_COLOR), c, "dye after flow_stats()")


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_a_spike_is_found_wherever_it_sits(sfl, oracle, dim_x, dim_y):
    v, _ = fields(dim_x, dim_y)
    plain = yardstick(oracle, v, None)
    with sfl.Solver(dim_x, dim_y) as s:
        for (i, j) in spike_cells(sfl, dim_x, dim_y):
            for k in (0, 1):
                for value in (1e6, -1e6):
                    q = v.copy()
                    q[j, i, k] = np.float32(value)
                    want = yardstick(oracle, q, None)
                    assert want[k] > 100 * plain[k] and want[2] > 100 * plain[2], "the spike must be what sets the maxima"
                    s.upload(sfl.capi.FIELD_VELOCITY, q)
                    assert_stats(s.flow_stats(dye=False), want, f"{dim_x} x {dim_y}, v[{k}] = {value} at ({i}, {j})", dye=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_non_finite_values_and_signed_zeros(sfl, oracle, dim_x, dim_y):
    v, _ = fields(dim_x, dim_y)
    with sfl.Solver(dim_x, dim_y) as s:
        for k in (0, 1):
            for value in (np.nan, np.inf, -np.inf):
                q = v.copy()
                q[dim_y // 2, dim_x // 3, k] = np.float32(value)
                want = yardstick(oracle, q, None)
                assert np.isnan(want[k]) or np.isinf(want[k])
                s.upload(sfl.capi.FIELD_VELOCITY, q)
                assert_stats(s.flow_stats(dye=False), want, f"{dim_x} x {dim_y}, one {value} in v[{k}]", dye=False)
        for value in (0.0, -0.0):
            q = np.full_like(v, value)
            s.upload(sfl.capi.FIELD_VELOCITY, q)
            got = s.flow_stats(dye=False)
            assert_stats(got, yardstick(oracle, q, None), f"{dim_x} x {dim_y}, all {value}", dye=False)
            for name in SPEEDS + ("max_abs_div",):
                assert got[name].view(np.uint32) == 0, f"all {value}: {name} must be +0.0f"


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_extreme_dye(sfl, oracle, dim_x, dim_y):
    with sfl.Solver(dim_x, dim_y) as s:
        c = np.full((dim_y, dim_x, 3), 0xFFFFFFFF, np.uint32)
        s.upload(sfl.capi.FIELD_COLOR, c)
        want = yardstick(oracle, None, c)
        assert all(int(x) == dim_x * dim_y * 0xFFFFFFFF for x in want[3]) and int(want[3][0]) > 2 ** 32
        assert_stats(s.flow_stats(velocity=False), want, f"{dim_x} x {dim_y}, all 0xFFFFFFFF", velocity=False)
        c = np.zeros((dim_y, dim_x, 3), np.uint32)
        c[0, 0, 1], c[-1, -1, 2] = 0x80000001, 0xFFFFFFFE
        s.upload(sfl.capi.FIELD_COLOR, c)
        want = yardstick(oracle, None, c)
        assert [int(x) for x in want[3]] == [0, 0x80000001, 0xFFFFFFFE]
        assert_stats(s.flow_stats(velocity=False), want, f"{dim_x} x {dim_y}, first and last texel", velocity=False)


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (130, 70), (257, 130)])
def test_the_fields_a_step_leaves_are_the_fields_read(sfl, oracle, dim_x, dim_y):
    """After sfl_step_n(3) -- the one-workgroup path at 61 x 81, fused step boundaries on the others -- the statistics are
    those of the downloads taken right after, and the call changes no field."""
    dx = 1.0
    with sfl.Solver(dim_x, dim_y) as s:
        s.setup_sketch_fields()
        s.queue_drags([(40, 20, 30.0, -12.0), (41, 20, 8.0, 25.0)])
        s.step_n(3, 0.05, dx, 20, 1.9)
        before = [s.download(f) for f in range(4)]
        got = s.flow_stats(dx)
        after = [s.download(f) for f in range(4)]
        again = s.flow_stats(dx)
    want = yardstick(oracle, before[0], before[1], dx)
    assert want[0] > 0 and want[1] > 0 and want[2] > 0 and int(want[3][0]) > 0
    assert_stats(got, want, f"{dim_x} x {dim_y} after three steps")
    assert_stats(again, want, f"{dim_x} x {dim_y} after three steps, asked again")
    for f in range(4):
        assert_bit_equal(after[f], before[f], f"field {f} after flow_stats()")


@pytest.mark.gpu
def test_a_slab_is_refused(sfl):
    with sfl.Solver(130, 70, rank=0, nranks=2) as s:
        with pytest.raises(sfl.SflError) as e:
            s.flow_stats()
        assert e.value.code == sfl.capi.ERR_STATE, str(e.value)
        assert "whole-domain contexts only" in str(e.value)


@pytest.mark.gpu
def test_seventeen_million_cells(sfl, oracle):
    """4099 x 4100: more tiles than the capped grid has waves (the waves stride, with 16-row chunks), rows that are not 16-byte
    aligned, dye blocks beyond what one pass of the grid takes.  One yardstick evaluation; the spikes sit in the last tile
    handed out."""
    dim_x, dim_y = 4099, 4100
    rng = np.random.default_rng(4099)
    v = (rng.random((dim_y, dim_x, 2), dtype=np.float32) - np.float32(0.5)) * np.float32(200)
    c = rng.integers(0, 2 ** 32, (dim_y, dim_x, 3), dtype=np.uint32)
    v[dim_y - 2, dim_x - 3, 0], v[dim_y - 1, dim_x - 1, 1] = np.float32(-1e6), np.float32(2e6)
    with sfl.Solver(dim_x, dim_y) as s:
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
        got = s.flow_stats(0.5)
    want = yardstick(oracle, v, c, 0.5)
    assert want[0] == 1e6 and want[1] == 2e6 and want[2] > 1e5
    assert_stats(got, want, "4099 x 4100")


# ---- GPU: batches -------------------------------------------------------------------------------------
BATCHES = [(61, 81, 5), (2, 2, 3), (96, 64, 2)]   # 61 x 81: member bases that are not 16-byte aligned; 96 x 64: the 6144-cell limit


@functools.lru_cache(maxsize=None)
def batch_fields(dim_x, dim_y, batch):
    """Every member with data of its own and a spike in a place of its own."""
    vs, cs = [], []
    for m in range(batch):
        v, c = fields(dim_x, dim_y, seed=1000 * (m + 1))
        v = v.copy()
        i, j = (m * 37 + 1) % dim_x, (m * 53 + dim_y - 1) % dim_y
        v[j, i, m % 2] = np.float32((-1) ** m * 1e5 * (m + 1))
        vs.append(v)
        cs.append(c)
    v, c = np.stack(vs), np.stack(cs)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,batch", BATCHES)
def test_every_member_reports_its_own_fields(sfl, oracle, dim_x, dim_y, batch):
    v, c = batch_fields(dim_x, dim_y, batch)
    dxs = [0.5 + 0.25 * m for m in range(batch)]
    what = f"{dim_x} x {dim_y} x {batch}"
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        for m, rec in enumerate(b.flow_stats()):
            assert_stats(rec, yardstick(oracle, np.zeros_like(v[0]), np.zeros_like(c[0])), f"{what}: fresh member {m}")
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.upload(sfl.capi.FIELD_COLOR, c)
        full = b.flow_stats(0.5)
        assert full.dtype == sfl.FLOW_STATS_DTYPE and full.shape == (batch,)
        for m in range(batch):
            assert_stats(full[m], yardstick(oracle, v[m], c[m], 0.5), f"{what}: member {m}")
        # a sub-range (first = 1; two members where the batch has them beyond member 0)
        count = min(2, batch - 1)
        part = b.flow_stats(0.5, first=1, count=count)
        assert part.tobytes() == full[1:1 + count].tobytes(), f"{what}: members [1, 1 + {count})"
        for velocity, dye in ((True, False), (False, True)):
            for m, rec in enumerate(b.flow_stats(0.5, first=1, count=count, velocity=velocity, dye=dye)):
                assert_stats(rec, yardstick(oracle, v[1 + m], c[1 + m], 0.5), f"{what}: member {1 + m}, one part", velocity, dye)
        # a dx per member
        each = b.flow_stats(dxs)
        for m in range(batch):
            assert_stats(each[m], yardstick(oracle, v[m], c[m], dxs[m]), f"{what}: member {m} with its own dx {dxs[m]}")
        part = b.flow_stats(dxs, first=1, count=count, dye=False)
        for m in range(count):
            assert_stats(part[m], yardstick(oracle, v[1 + m], None, dxs[1 + m]), f"{what}: member {1 + m}, own dx, sub-range", dye=False)
        # what is refused, with a batch at hand
        lib, out = sfl.capi.lib(), (sfl.capi.FlowStats * (batch + 1))()
        assert lib.sfl_batch_flow_stats(b._h, 3, 1.0, 1, batch, out, 40 * batch) == sfl.capi.ERR_INVALID
        assert "not inside the batch" in lib.sfl_last_error().decode()
        assert lib.sfl_batch_flow_stats(b._h, 3, 1.0, -1, 1, out, 40) == sfl.capi.ERR_INVALID
        assert lib.sfl_batch_flow_stats(b._h, 3, 1.0, 0, batch, None, 40 * batch) == sfl.capi.ERR_INVALID
        assert lib.sfl_batch_flow_stats_each(b._h, 3, None, 0, batch, out, 40 * batch) == sfl.capi.ERR_INVALID
        assert lib.sfl_batch_flow_stats(b._h, 3, 1.0, 0, 0, out, 0) == sfl.capi.OK          # an empty range is one
        assert_bit_equal(b.download(sfl.capi.FIELD_VELOCITY), v, "velocity after flow_stats()")
        assert_bit_equal(b.download(sfl.capi.FIELD_COLOR), c, "dye after flow_stats()")
    # a member and a context with the same fields agree bit for bit
    with sfl.Solver(dim_x, dim_y) as s:
        for m in range(batch):
            s.upload(sfl.capi.FIELD_VELOCITY, v[m])
            s.upload(sfl.capi.FIELD_COLOR, c[m])
            assert s.flow_stats(dxs[m]).tobytes() == each[m].tobytes(), f"{what}: member {m} against a context"


@pytest.mark.gpu
def test_the_batchs_reports_do_not_go_stale(sfl, oracle):
    dim_x, dim_y, batch = 61, 81, 3
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.setup_sketch_fields()
        b.queue_forces([0, 2], [(20, 40), (30, 10)], [(-12.0, 30.0), (9.0, -25.0)])
        b.step_n_until(2, 0.05, 1.0, 40, 1.9, tol=[1e-2, 1e-3, 1e-1], every=4)
        residual, iterations = b.residual(), b.iterations()
        got = b.flow_stats(1.0)
        assert_bit_equal(b.residual(), residual, "residual() after flow_stats()")
        assert np.array_equal(b.iterations(), iterations), "iterations() after flow_stats()"
        v, c = b.download(sfl.capi.FIELD_VELOCITY), b.download(sfl.capi.FIELD_COLOR)
    for m in range(batch):
        assert_stats(got[m], yardstick(oracle, v[m], c[m], 1.0), f"member {m} after step_n_until")
    assert got["max_abs_vx"][0] > 0 and got["max_abs_vx"][1] == 0    # (member 1 was never pushed)
