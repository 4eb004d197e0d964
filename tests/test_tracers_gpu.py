"""Tracers on the GPU (csrc/tracers.hip behind sfl_tracers_* / sfl_batch_tracers_*; include/sfl.h "TRACERS").

Every comparison is bit for bit (a NaN by any NaN): against the golden fixtures, which hold what the reference's advect.h
leaves (tests/golden/make_tracer_goldens.py), or against tests/tracer_rule.py -- the same rule in numpy, pinned to those
fixtures by tests/test_tracers.py -- applied to the fields downloaded from a twin that is stepped one step at a time.
The fields of a context or batch with tracers are compared with a twin without by the library's own distance calls: all
three counts zero <=> identical bits."""
import functools
import os

import numpy as np
import pytest

import tracer_rule as rule
from conftest import GOLDEN, random_fields

pytestmark = pytest.mark.gpu

FV, FC, FDIV, FP = 0, 1, 2, 3       # SFL_FIELD_VELOCITY, SFL_FIELD_COLOR, SFL_FIELD_DIVERGENCE, SFL_FIELD_PRESSURE
FIELDS = (FV, FC, FDIV, FP)
DT, DX, ITERS, OMEGA = 0.05, 1.0, 8, 1.9
ERR_INVALID, ERR_STATE = -1, -5


def assert_same(got, want, what):
    assert rule.same_bits(got, want), f"{what}: got\n{got}\nwant\n{want}"


def assert_no_distance(records, what):
    for name in ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ"):
        assert not np.any(records[name]), f"{what}: {name} {records[name]}"


@functools.lru_cache(maxsize=None)
def fields(dim_x, dim_y, seed=0):
    """(velocity, dye, divergence, pressure): a velocity of up to +-20 cells per unit of time (one cell per step at DT), a
    dye below 2^31, two scalars.  Shared: never written to."""
    v, c, s = random_fields(dim_x, dim_y, 700 + dim_x + seed, vamp=20.0)
    p = np.random.default_rng(77 + dim_y + seed).standard_normal((dim_y, dim_x)).astype(np.float32)
    for a in (v, c, s, p):
        a.setflags(write=False)
    return v, c, s, p


@functools.lru_cache(maxsize=None)
def starts(dim_x, dim_y, n, seed=0):
    """n positions from 1.5 cells outside one wall to 1.5 cells outside the other -- about one in three of a 3 x 3 grid
    inside -- the first ones on the walls, the corners and both sides of the half cell where the no-slip weight ends."""
    rng = np.random.default_rng(5 + n + seed)
    xy = np.stack([rng.uniform(-1.5, dim_x + 0.5, n), rng.uniform(-1.5, dim_y + 0.5, n)], axis=1).astype(np.float32)
    lx, ly = dim_x - 1, dim_y - 1
    special = np.array([[0, 0], [lx, ly], [-0.25, 0.5], [lx + 0.25, 0.25], [0.5, -0.75], [0.25, ly + 0.5], [-0.1, -0.2],
                        [lx + 0.3, ly + 0.4], [lx - 0.5, ly - 0.5], [-3, ly + 3]], np.float32)
    xy[:min(n, len(special))] = special[:n]
    xy.setflags(write=False)
    return xy


def context_with(sfl, dim_x, dim_y, seed=0):
    s = sfl.Solver(dim_x, dim_y)
    for field, a in zip(FIELDS, fields(dim_x, dim_y, seed)):
        s.upload(field, a)
    return s


def check_samples(s, held, xy, what):
    """The four fields sampled at xy, both ways, against the rule on the fields `held`."""
    for field, a in zip(FIELDS, held):
        for no_slip in (False, True):
            assert_same(s.sample_tracers(field, no_slip), rule.sample(a, xy[:, 0], xy[:, 1], no_slip), f"{what}: field {field}, no_slip {no_slip}")


# ---- the golden fixtures through a context ------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["33x17", "61x81"])
def test_the_fixtures_through_a_context(sfl, shape):
    """6 manual advances, then the four samples: the bits the reference's advect.h left."""
    fix = np.load(os.path.join(GOLDEN, f"tracers_{shape}.npz"))
    dim_y, dim_x = fix["pressure"].shape
    with sfl.Solver(dim_x, dim_y) as s:
        for field, name in zip(FIELDS, ("velocity", "dye", "divergence", "pressure")):
            s.upload(field, fix[name])
        s.set_tracers(fix["positions"][0], follow=False)
        assert s.tracer_count() == fix["positions"].shape[1]
        for k in range(1, 7):
            s.advance_tracers(float(fix["dt"]))
            assert_same(s.tracers(), fix["positions"][k], f"after advance {k}")
        for field, name in zip(FIELDS, ("velocity", "dye", "divergence", "pressure")):
            for no_slip in (0, 1):
                assert_same(s.sample_tracers(field, bool(no_slip)), fix["sample_" + name][no_slip], f"{name}, no_slip {no_slip}")


# ---- counts: the wave and block edges -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 257, 1000])
def test_counts(sfl, n):
    dim_x, dim_y = 61, 81
    held = fields(dim_x, dim_y)
    with context_with(sfl, dim_x, dim_y) as s:
        xy = starts(dim_x, dim_y, n)
        s.set_tracers(xy, follow=False)
        assert s.tracer_count() == n
        if n == 0:   # an empty set is no set
            for call in (s.tracers, lambda: s.advance_tracers(DT), lambda: s.sample_tracers(FP), lambda: s.trail_start(1, 4)):
                with pytest.raises(sfl.SflError) as e:
                    call()
                assert e.value.code == ERR_STATE
            return
        for k in range(2):
            s.advance_tracers(0.1)
            xy = rule.advance(held[0], xy, 0.1)
            assert_same(s.tracers(), xy, f"n {n}, advance {k}")
        check_samples(s, held, xy, f"n {n}")


# ---- shapes: walls and corners almost everywhere, the one-workgroup path, the tiled path --------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (3, 3), (61, 81), (130, 70)])
def test_context_shapes(sfl, dim_x, dim_y):
    held = fields(dim_x, dim_y)
    with context_with(sfl, dim_x, dim_y) as s:
        xy = starts(dim_x, dim_y, 300)
        s.set_tracers(xy, follow=False)
        for k in range(3):
            s.advance_tracers(0.08)
            xy = rule.advance(held[0], xy, 0.08)
            assert_same(s.tracers(), xy, f"advance {k}")
        check_samples(s, held, xy, f"{dim_x} x {dim_y}")
        for field, a in zip(FIELDS, held):   # the calls read only
            assert_same(s.download(field), a, f"field {field} after the tracer calls")


# ---- following on a context ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (130, 70)])
def test_following_on_a_context(sfl, dim_x, dim_y):
    """step_n(5) with a following set == 5 x (step; advance) == the rule on the velocity a twin holds after each single
    step; the fields are those of a twin without tracers that runs step_n(5) (with its seams, where it has them)."""
    xy0 = starts(dim_x, dim_y, 200)
    force = (np.array([[dim_x // 2, dim_y // 2]], np.int32), np.array([[30.0, -20.0]], np.float32))
    with context_with(sfl, dim_x, dim_y) as a, context_with(sfl, dim_x, dim_y) as b, context_with(sfl, dim_x, dim_y) as twin, \
            context_with(sfl, dim_x, dim_y) as plain:
        for s in (a, b, twin, plain):
            if dim_x * dim_y > 6144:   # beyond the one-workgroup path: the tiled kernels, so that step_n has its seams
                s.set_option(sfl.capi.OPT_ADVECT_KERNEL, 2)
            s.queue_forces(*force, step=2)
        a.set_tracers(xy0, follow=True)
        a.step_n(5, DT, DX, ITERS, OMEGA)
        b.set_tracers(xy0, follow=False)
        xy = xy0
        for k in range(5):
            b.step(DT, DX, ITERS, OMEGA)
            b.advance_tracers(DT)
            twin.step(DT, DX, ITERS, OMEGA)
            xy = rule.advance(twin.download(FV), xy, DT)
            assert_same(b.tracers(), xy, f"step; advance {k}")
        assert_same(a.tracers(), xy, "step_n(5) with a following set")
        assert not np.array_equal(xy, xy0)
        plain.step_n(5, DT, DX, ITERS, OMEGA)
        for s, name in ((a, "following"), (b, "manual")):
            assert_no_distance(s.distance(plain), f"{name} against a context without tracers")
        check_samples(a, [a.download(f) for f in FIELDS], xy, "after the steps")


# ---- batches ---------------------------------------------------------------------------------------------------------------
BATCHES = {"small": (61, 81, 5, 37, False), "large": (96, 96, 3, 300, True)}
DTS = [0.02, 0.035, 0.05, 0.065, 0.08]


def batch_with(sfl, kind):
    dim_x, dim_y, B, K, large = BATCHES[kind]
    b = sfl.BatchSolver(dim_x, dim_y, B, large=large)
    for field in (FV, FC):
        b.upload(field, np.stack([fields(dim_x, dim_y, seed=m)[field] for m in range(B)]))
    return b


def batch_starts(kind):
    dim_x, dim_y, B, K, _ = BATCHES[kind]
    return np.stack([starts(dim_x, dim_y, K, seed=m) for m in range(B)])


def step_call(call, B):
    """(the call on n steps, each member's dt); the members' iterations differ, so their records are not in member order"""
    dts = DTS[:B]
    if call == "step_n":
        return (lambda b, n: b.step_n(n, DT, DX, ITERS, OMEGA)), [DT] * B
    if call == "step_n_each":
        return (lambda b, n: b.step_n_each(n, dts, DX, [ITERS + m for m in range(B)], OMEGA)), dts
    return (lambda b, n: b.step_n_until(n, dts, DX, 40, OMEGA, tol=1e-3, every=4)), dts


@pytest.mark.parametrize("kind", list(BATCHES))
@pytest.mark.parametrize("call", ["step_n", "step_n_each", "step_n_until", "timeline", "timeline_each"])
def test_following_in_a_batch(sfl, kind, call):
    """One call of 4 steps with a following set, the recorder running alongside: the positions equal the per-step rule on a
    twin stepped one step at a time, each member by its own dt; the fields equal a twin's without tracers that makes the
    same one call.  `timeline`: a record at step 2 of the 4, which small members without tracers replay in one launch."""
    dim_x, dim_y, B, K, _ = BATCHES[kind]
    run, dts = step_call({"timeline": "step_n", "timeline_each": "step_n_each"}.get(call, call), B)
    n = 4
    with batch_with(sfl, kind) as a, batch_with(sfl, kind) as twin, batch_with(sfl, kind) as plain:
        if call.startswith("timeline"):
            for b in (a, twin, plain):
                b.queue_forces([1, B - 1], [[dim_x // 2, dim_y // 3], [3, 4]], [[25.0, 10.0], [-15.0, 30.0]], step=2)
        xy0 = batch_starts(kind)
        a.set_tracers(xy0, follow=True)
        a.record_start(every=2, first=0, count=2, scaling=1, capacity=4)
        run(a, n)
        xy = xy0
        for k in range(n):
            run(twin, 1)
            v = twin.download(FV)
            xy = np.stack([rule.advance(v[m], xy[m], dts[m]) for m in range(B)])
        got = a.tracers()
        assert got.shape == (B, K, 2)
        assert_same(got, xy, f"{kind} {call}")
        assert not np.array_equal(xy, xy0)
        plain.record_start(every=2, first=0, count=2, scaling=1, capacity=4)
        run(plain, n)
        assert_no_distance(a.distance(plain), "against a batch without tracers")
        assert_no_distance(a.distance(twin), "against the twin stepped one step at a time")
        assert np.array_equal(a.frames(), plain.frames()) and a.record_info() == (2, 4, 4)
        v, c = a.download(FV), a.download(FC)
        for field, held in ((FV, v), (FC, c)):
            want = np.stack([rule.sample(held[m], xy[m, :, 0], xy[m, :, 1], True) for m in range(B)])
            assert_same(a.sample_tracers(field, True), want, f"sample of field {field}")


# ---- trails ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("every", [1, 2])
def test_trails_of_a_context(sfl, every):
    dim_x, dim_y = 61, 81
    xy0 = starts(dim_x, dim_y, 100)
    with context_with(sfl, dim_x, dim_y) as a, context_with(sfl, dim_x, dim_y) as twin:
        a.set_tracers(xy0, follow=True)
        a.trail_start(every, 3)
        a.step_n(2, DT, DX, ITERS, OMEGA)
        a.advance_tracers(0.1)                      # a manual advance counts too
        a.step_n(3 * every - 3, DT, DX, ITERS, OMEGA)
        xy, after = xy0, []
        for k in range(3 * every):
            if k != 2:
                twin.step(DT, DX, ITERS, OMEGA)
            xy = rule.advance(twin.download(FV), xy, 0.1 if k == 2 else DT)
            after.append(xy)
        assert a.trail_info() == (3, 3, 3 * every)
        assert_same(a.trail(), np.stack(after[every - 1::every]), f"every {every}")
        # overflow: refused whole -- fields, positions, timeline and counts untouched
        a.queue_forces([[5, 5]], [[1.0, 2.0]], step=1)
        before = [a.download(f) for f in FIELDS], a.tracers(), a.forces_pending()
        for call in (lambda: a.step_n(every, DT, DX, ITERS, OMEGA), lambda: [a.advance_tracers(DT) for _ in range(every)]):
            with pytest.raises(sfl.SflError) as e:
                call()
            assert e.value.code == ERR_STATE and "room for 0 more" in str(e.value)
            if every == 2:   # (the first of two manual advances fits: start over for the comparison below)
                break
        for f, held in zip(FIELDS, before[0]):
            assert_same(a.download(f), held, f"field {f} after the refused call")
        assert_same(a.tracers(), before[1], "positions after the refused call")
        assert a.forces_pending() == before[2] and a.trail_info() == (3, 3, 3 * every)
        a.trail_stop()
        assert a.trail_info() == (0, 0, 0)
        a.step_n(2, DT, DX, ITERS, OMEGA)           # ... and steps again


@pytest.mark.parametrize("kind", list(BATCHES))
def test_trails_of_a_batch(sfl, kind):
    dim_x, dim_y, B, K, _ = BATCHES[kind]
    run, dts = step_call("step_n_each", B)
    with batch_with(sfl, kind) as a, batch_with(sfl, kind) as twin:
        xy0 = batch_starts(kind)
        a.set_tracers(xy0, follow=True)
        a.trail_start(2, 2)
        run(a, 5)
        xy, after = xy0, []
        for k in range(5):
            run(twin, 1)
            v = twin.download(FV)
            xy = np.stack([rule.advance(v[m], xy[m], dts[m]) for m in range(B)])
            after.append(xy)
        assert a.trail_info() == (2, 2, 5)
        trail = a.trail()
        assert trail.shape == (2, B, K, 2)
        assert_same(trail, np.stack([after[1], after[3]]), "slots after advances 2 and 4")
        before = a.download(FV), a.download(FC), a.tracers()
        with pytest.raises(sfl.SflError) as e:
            run(a, 1)
        assert e.value.code == ERR_STATE
        for got, held in zip((a.download(FV), a.download(FC), a.tracers()), before):
            assert_same(got, held, "after the refused call")
        assert a.trail_info() == (2, 2, 5)


# ---- special values --------------------------------------------------------------------------------------------------------
def test_special_values(sfl):
    dim_x, dim_y = 33, 17
    v, c, d, p = [a.copy() for a in fields(dim_x, dim_y)]
    nan, inf = np.float32(np.nan), np.float32(np.inf)
    xy0 = starts(dim_x, dim_y, 400).copy()
    xy0[:8] = [[nan, 3.0], [4.0, nan], [nan, nan], [inf, 2.5], [-inf, 3.5], [5.5, inf], [-inf, -inf], [3e38, -3e38]]
    xy0[8:12] = [[10.5, 6.5], [11.25, 7.75], [10.01, 7.99], [11.99, 6.01]]   # the four cells' squares around cell (11, 7)
    with sfl.Solver(dim_x, dim_y) as s:
        for field, a in zip(FIELDS, (v, c, d, p)):
            s.upload(field, a)
        s.set_tracers(xy0, follow=False)
        s.advance_tracers(0.1)
        xy = rule.advance(v, xy0, 0.1)
        got = s.tracers()
        assert_same(got, xy, "NaN and infinite coordinates")
        assert np.array_equal(got[:3].view(np.uint32), xy0[:3].view(np.uint32)), "a tracer with a NaN coordinate keeps both"
        assert np.array_equal(got[3:8], xy0[3:8]), "infinitely far outside, no-slip: they stay"
        check_samples(s, (v, c, d, p), xy, "special coordinates")
        assert np.all(np.isnan(s.sample_tracers(FV)[:3])) and not np.any(s.sample_tracers(FC)[:3]) and np.all(np.isnan(s.sample_tracers(FP)[:3]))
        # a NaN planted in the velocity: the tracers that read it turn NaN and no others
        v[7, 11] = [nan, 1.0]
        s.upload(FV, v)
        s.set_tracers(xy0[8:], follow=False)
        s.advance_tracers(0.1)
        want = rule.advance(v, xy0[8:], 0.1)
        turned = np.isnan(want).any(axis=1)
        x, y = xy0[8:, 0], xy0[8:, 1]
        assert turned.any() and np.array_equal(turned, (x > 10) & (x < 12) & (y > 6) & (y < 8))
        assert_same(s.tracers(), want, "a NaN in the velocity")
        s.advance_tracers(0.1)
        assert_same(s.tracers(), rule.advance(v, want, 0.1), "a NaN position stays")


# ---- more members than one launch's grid holds -------------------------------------------------------------------------
def test_a_batch_of_more_members_than_a_grid_has_rows(sfl):
    """65537 members of 3 x 3: the members are the y dimension of the launch's grid, which ends at 65535, so the advance
    and the sample take a second launch -- with the call's dt, and with the member records of a step_n_each call.  Checked
    on the members at both ends of both launches."""
    dim_x, dim_y, B, K = 3, 3, 65537, 3
    rng = np.random.default_rng(9)
    v = rng.uniform(-20, 20, (B, dim_y, dim_x, 2)).astype(np.float32)
    xy0 = np.stack([rng.uniform(-1.5, dim_x + 0.5, (B, K)), rng.uniform(-1.5, dim_y + 0.5, (B, K))], axis=-1).astype(np.float32)
    watch = [0, 1, 65534, 65535, 65536]
    dts = np.linspace(0.02, 0.08, B).astype(np.float32)
    iters = 2 + (np.arange(B) % 3)                       # the records are not in member order
    with sfl.BatchSolver(dim_x, dim_y, B) as a, sfl.BatchSolver(dim_x, dim_y, B) as twin:
        for b in (a, twin):
            b.upload(FV, v)
        a.set_tracers(xy0, follow=True)
        a.advance_tracers(0.1)
        got = a.tracers()
        for m in watch:
            assert_same(got[m], rule.advance(v[m], xy0[m], 0.1), f"manual advance, member {m}")
        smp = a.sample_tracers(FV, False)
        for m in watch:
            assert_same(smp[m], rule.sample(v[m], got[m, :, 0], got[m, :, 1], False), f"sample, member {m}")
        a.step_n_each(1, dts, DX, iters, OMEGA)
        twin.step_n_each(1, dts, DX, iters, OMEGA)
        after, moved = twin.download(FV), a.tracers()
        for m in watch:
            assert_same(moved[m], rule.advance(after[m], got[m], dts[m]), f"following step_n_each, member {m}")
        # ... and a sample of every 97th member: none moved twice, none left out
        for m in range(2, B, 97):
            assert_same(moved[m], rule.advance(after[m], got[m], dts[m]), f"following step_n_each, member {m}")
        assert_no_distance(a.distance(twin), "against the twin without tracers")
