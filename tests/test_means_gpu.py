"""Averages on the GPU (include/sfl.h "AVERAGES"; csrc/means.hip): the per-cell sums over time of a batch and of a whole-domain
context against tests/mean_rule.py -- the header's rule in numpy, whose own sanity tests/test_means.py checks.  Every
comparison is on the BYTES of the planes: there is no tolerance anywhere.

Shapes, the smallest at which this kernel can go wrong (a lane holds two neighbouring cells of one member; a member's plane is
padded to an even number of values; the fields are not): batches 2 x 2 x 3 (all corners), 7 x 5 x 4 (fewer cells than threads,
an odd cell count), 61 x 81 x 5 recording members [1, 4) (odd member bases, every alignment of the dye, unrecorded members on
both sides), 64 x 96 x 2 and 127 x 159 x 2 of large members; contexts 7 x 5, 61 x 81 and 257 x 131 (several workgroups and a
tail)."""
import contextlib
import functools

import numpy as np
import pytest

import mean_rule as rule
import value_cases as vc
from conftest import random_fields

pytestmark = pytest.mark.gpu

F = np.float32
DT, DX, ITERS, OMEGA = 1 / 30.0, 0.37, 6, 1.9
COUNTS = ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ")
MASKS = (1, 2, 4, 8, 6, 15)
# (dim_x, dim_y, batch, large, (first, count) recorded)
BATCHES = [(2, 2, 3, False, (0, 3)), (7, 5, 4, False, (0, 4)), (61, 81, 5, False, (1, 3)), (64, 96, 2, False, (0, 2)), (127, 159, 2, True, (0, 2))]
CONTEXTS = [(7, 5), (61, 81), (257, 131)]


# ---- inputs and comparisons --------------------------------------------------------------------------------------------------
def wide(shape, rng):
    """float32 with magnitudes 10^-44 .. 10^18 (denormals included), both signs, every tenth value -0.0f or +0.0f."""
    with np.errstate(all="ignore"):
        a = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-44, 18, shape)).astype(F)
    a[rng.random(shape) < 0.05] = F(-0.0)
    a[rng.random(shape) < 0.05] = F(0.0)
    return a


@functools.lru_cache(maxsize=None)
def seeded_samples(members, dim_y, dim_x, seed=0, n=3):
    """n samples of (v, p, dye) for `members` members; the dye over the whole of uint32.  Shared, never written."""
    rng = np.random.default_rng(9000 + 131 * dim_x + dim_y + seed)
    out = []
    for _ in range(n):
        v, p = wide((members, dim_y, dim_x, 2), rng), wide((members, dim_y, dim_x), rng)
        dye = rng.integers(0, 2 ** 32, (members, dim_y, dim_x, 3), dtype=np.uint64).astype(np.uint32)
        for a in (v, p, dye):
            a.setflags(write=False)
        out.append((v, p, dye))
    return tuple(out)


def upload(s, cap, v, p, dye, context):
    for field, a in ((cap.FIELD_VELOCITY, v), (cap.FIELD_PRESSURE, p), (cap.FIELD_COLOR, dye)):
        s.upload(field, a[0] if context else a)


def planes(s, what):
    return {k: s.mean_sums(k) for k in rule.planes_of(what)}


def assert_planes_equal(got, want, what=""):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for k in want:
        g, w = np.ascontiguousarray(got[k]), np.ascontiguousarray(want[k])
        assert g.dtype == w.dtype == rule.dtype_of(k) and g.shape == w.shape, (what, rule.NAMES[k], g.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint64) != w.view(np.uint64))
            at = tuple(bad[0])
            raise AssertionError(f"{what}: plane {rule.NAMES[k]} differs in {len(bad)} of {g.size} values, first at {at}: got {g[at]!r}, want {w[at]!r}")


def zero_counts(d):
    return all((np.asarray(d[c]) == 0).all() for c in COUNTS)


# ---- 1. the kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y,batch,large,rec", BATCHES, ids=[f"{x}x{y}x{b}" for x, y, b, _, _ in BATCHES])
def test_a_batchs_samples_are_the_rules_for_every_mask_and_change_no_field(sfl, dim_x, dim_y, batch, large, rec):
    cap = sfl.capi
    first, count = rec
    samples = seeded_samples(batch, dim_y, dim_x)
    want = rule.sums(rule.ALL, [(v[first:first + count], p[first:first + count], d[first:first + count]) for v, p, d in samples])
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b, sfl.BatchSolver(dim_x, dim_y, batch, large=large) as twin:
        for what in MASKS:
            b.mean_start(what, 0, first, count)
            for fields in samples:
                upload(b, cap, *fields, False)
                b.mean_sample()
            assert b.mean_info() == (what, 0, 3, 0)
            assert_planes_equal(planes(b, what), {k: want[k] for k in rule.planes_of(what)}, f"{dim_x}x{dim_y}x{batch} mask {what}")
        upload(twin, cap, *samples[-1], False)
        assert zero_counts(b.distance(twin)), "the fields held are what was uploaded"
        if count > 1:   # a part of the recorded range
            got = b.mean_sums(rule.UV, first + 1, count - 1)
            assert got.tobytes() == want[rule.UV][1:].tobytes()


@pytest.mark.parametrize("dim_x,dim_y", CONTEXTS, ids=[f"{x}x{y}" for x, y in CONTEXTS])
def test_a_contexts_samples_are_the_rules_for_every_mask_and_change_no_field(sfl, dim_x, dim_y):
    cap = sfl.capi
    samples = seeded_samples(1, dim_y, dim_x)
    want = rule.sums(rule.ALL, samples)
    with sfl.Solver(dim_x, dim_y) as c, sfl.Solver(dim_x, dim_y) as twin:
        for what in MASKS:
            c.mean_start(what, 0)
            for fields in samples:
                upload(c, cap, *fields, True)
                c.mean_sample()
            assert c.mean_info() == (what, 0, 3, 0)
            assert_planes_equal(planes(c, what), {k: want[k] for k in rule.planes_of(what)}, f"context {dim_x}x{dim_y} mask {what}")
        upload(twin, cap, *samples[-1], True)
        assert zero_counts(c.distance(twin)), "the fields held are what was uploaded"


# ---- 2. behind the steps -------------------------------------------------------------------------------------------------------
def start_fields(members, dim_x, dim_y):
    vs, cs = zip(*(random_fields(dim_x, dim_y, 40 + m, vamp=30.0)[:2] for m in range(members)))
    return np.stack(vs), np.stack(cs)


def batch_step(b, kind, n, batch):
    """n steps of one kind of step call, every member with parameters of its own where the kind has them."""
    dts = [DT * (1 + 0.25 * (m % 3)) for m in range(batch)]
    its = [ITERS + (m % 2) * 3 for m in range(batch)]
    if kind == "uniform":
        b.step_n(n, DT, DX, ITERS, OMEGA)
    elif kind == "each":
        b.step_n_each(n, dts, DX, its, OMEGA)
    else:
        b.step_n_until(n, dts, DX, 12, OMEGA, tol=[1e-3, 0.0, 1e-1][:batch] + [1e-2] * max(0, batch - 3), every=2)


BEHIND = [("uniform", False, False), ("each", False, False), ("until", False, False), ("uniform", True, False), ("each", True, False),
          ("until", True, False), ("uniform", False, True), ("each", False, True)]


@pytest.mark.parametrize("every,calls", [(1, (5,)), (3, (7,)), (3, (4, 4))], ids=["every1", "every3", "every3-two-calls"])
@pytest.mark.parametrize("kind,large,timeline", BEHIND, ids=[f"{k}{'-large' if lg else ''}{'-timeline' if t else ''}" for k, lg, t in BEHIND])
def test_a_batchs_samples_behind_the_steps_are_the_manual_samples_of_a_twin(sfl, kind, large, timeline, every, calls):
    cap = sfl.capi
    dim_x, dim_y, batch = (96, 96, 2) if large else (61, 81, 3)
    first, count = (0, batch) if large else (1, 2)
    v0, c0 = start_fields(batch, dim_x, dim_y)
    with contextlib.ExitStack() as stack:
        b, twin, plain = (stack.enter_context(sfl.BatchSolver(dim_x, dim_y, batch, large=large)) for _ in range(3))
        for s in (b, twin, plain):
            s.upload(cap.FIELD_VELOCITY, v0)
            s.upload(cap.FIELD_COLOR, c0)
            s.queue_forces([0, batch - 1], [(dim_x // 2, dim_y // 2), (3, 4)], [(35.0, -20.0), (-12.0, 9.0)])
            if timeline:   # records in later steps: a call of several steps replays the timeline in one launch, cut where a sample is due
                s.queue_forces([1], [(dim_x // 3, dim_y // 3)], [(-18.0, 27.0)], step=2)
                s.queue_forces([0], [(5, 6)], [(8.0, 8.0)], step=5)
        b.mean_start(rule.ALL, every, first, count)
        twin.mean_start(rule.ALL, 0, first, count)
        done = 0
        for n in calls:
            batch_step(b, kind, n, batch)
            batch_step(plain, kind, n, batch)
            for _ in range(n):
                batch_step(twin, kind, 1, batch)
                done += 1
                if done % every == 0:
                    twin.mean_sample()
        assert b.mean_info() == (rule.ALL, every, done // every, done) and twin.mean_info() == (rule.ALL, 0, done // every, 0)
        assert done // every >= 2
        got, want = planes(b, rule.ALL), planes(twin, rule.ALL)
        assert_planes_equal(got, want, f"{kind} every {every}")
        assert got[rule.UU].any() and got[rule.PP].any() and got[rule.R].any()
        assert zero_counts(b.distance(plain)), "the same run without averages leaves the same fields"
        assert zero_counts(b.distance(twin)), "... and so does the run step by step"
        # the last sample is the fields held: the sums of one more manual sample move by exactly the rule's terms
        v, p, dye = (b.download(f, first, count) for f in (cap.FIELD_VELOCITY, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
        b.mean_sample()
        assert_planes_equal(planes(b, rule.ALL), rule.add({k: a.copy() for k, a in got.items()}, rule.ALL, v, p, dye), "one more sample")


@pytest.mark.parametrize("every,calls", [(1, (4,)), (3, (7,)), (3, (4, 4))], ids=["every1", "every3", "every3-two-calls"])
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (300, 141)], ids=["61x81", "300x141"])
def test_a_contexts_samples_behind_step_n_are_the_manual_samples_of_a_twin(sfl, dim_x, dim_y, every, calls):
    cap = sfl.capi
    v0, c0 = random_fields(dim_x, dim_y, 77, vamp=30.0)[:2]
    with sfl.Solver(dim_x, dim_y) as c, sfl.Solver(dim_x, dim_y) as twin, sfl.Solver(dim_x, dim_y) as plain:
        for s in (c, twin, plain):
            s.upload(cap.FIELD_VELOCITY, v0)
            s.upload(cap.FIELD_COLOR, c0)
            s.queue_forces([(dim_x // 2, dim_y // 2)], [(35.0, -20.0)])
            s.queue_forces([(3, 4)], [(-12.0, 9.0)], step=2)
        c.mean_start(rule.ALL, every)
        twin.mean_start(rule.ALL, 0)
        done = 0
        for n in calls:
            c.step_n(n, DT, DX, ITERS, OMEGA)
            plain.step_n(n, DT, DX, ITERS, OMEGA)
            for _ in range(n):
                twin.step_n(1, DT, DX, ITERS, OMEGA)
                done += 1
                if done % every == 0:
                    twin.mean_sample()
        assert c.mean_info() == (rule.ALL, every, done // every, done)
        got = planes(c, rule.ALL)
        assert_planes_equal(got, planes(twin, rule.ALL), f"context {dim_x}x{dim_y} every {every}")
        assert got[rule.UU].any() and got[rule.PP].any() and got[rule.R].any()
        assert zero_counts(c.distance(plain)) and zero_counts(c.distance(twin)), "the run without averages and the run step by step leave the same fields"


# ---- 3. a small tunnel -------------------------------------------------------------------------------------------------------
def test_a_small_tunnel_gives_the_same_planes_as_a_context_and_as_a_batch_member_solid_cells_included(sfl):
    cap = sfl.capi
    dim_x, dim_y, steps = 12, 9, 4
    solid = np.zeros((dim_y, dim_x), bool)
    solid[0, :] = solid[-1, :] = True          # walls
    solid[4, 5] = solid[5, 5] = True           # a peg
    tunnel = np.zeros((dim_y, dim_x), np.uint8)
    tunnel[1:-1, 0], tunnel[1:-1, -1] = sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW
    v0 = np.zeros((dim_y, dim_x, 2), F)
    v0[~solid, 0] = 3.0
    v0[solid] = (-7.5, 2.25)                   # what a solid cell holds is averaged as it is
    c0 = random_fields(dim_x, dim_y, 5)[1]
    with sfl.Solver(dim_x, dim_y) as c, sfl.BatchSolver(dim_x, dim_y, 2) as b, sfl.BatchSolver(dim_x, dim_y, 2) as by_step:
        for s, lead in ((c, False), (b, True), (by_step, True)):
            s.upload(cap.FIELD_VELOCITY, np.stack([v0, v0]) if lead else v0)
            s.upload(cap.FIELD_COLOR, np.stack([c0, c0]) if lead else c0)
            s.set_solids(solid)
            s.set_openings(tunnel, (3.0, 0.0))
        c.mean_start(rule.ALL, 1)
        b.mean_start(rule.ALL, 1, 1, 1)
        c.step_n(steps, DT, 1.0, ITERS, OMEGA)
        b.step_n(steps, DT, 1.0, ITERS, OMEGA)
        held = []
        for _ in range(steps):
            by_step.step_n(1, DT, 1.0, ITERS, OMEGA)
            held.append(tuple(by_step.download(f, 1, 1) for f in (cap.FIELD_VELOCITY, cap.FIELD_PRESSURE, cap.FIELD_COLOR)))
        want = rule.sums(rule.ALL, held)
        assert_planes_equal(planes(b, rule.ALL), want, "the batch member")
        assert_planes_equal(planes(c, rule.ALL), want, "the context")
        assert any(a[0][solid].any() for a in want.values()), "solid cells take part as they are"
        assert want[rule.P].any() and want[rule.U][0][~solid].any()


# ---- 4. values ------------------------------------------------------------------------------------------------------------------
def test_a_nan_and_an_inf_poison_their_own_cells_sums_only(sfl):
    cap = sfl.capi
    dim_x, dim_y = 61, 81
    (v, p, dye), = seeded_samples(2, dim_y, dim_x, seed=3, n=1)
    v, p = v.copy(), p.copy()
    v[1, 40, 30, 0] = np.nan          # u of one cell: U, UU, UV
    v[1, 80, 60] = (2.0, -np.inf)     # v of the member's LAST cell, which sits alone in its lane: V, VV, UV
    p[0, 0, 0] = np.inf               # the first cell of member 0
    p[1, 17, 33] = np.nan
    # (every NaN here is the one that was put in, carried along: IEEE leaves the sign of a NaN that an invalid operation makes
    # -- Inf - Inf, 0 * Inf -- to the implementation, so the inputs make none)
    with sfl.BatchSolver(dim_x, dim_y, 2) as b:
        b.mean_start(rule.ALL, 0)
        upload(b, cap, v, p, dye, False)
        b.mean_sample()
        b.mean_sample()
        got = planes(b, rule.ALL)
    want = rule.sums(rule.ALL, [(v, p, dye)] * 2)
    assert_planes_equal(got, want, "nonfinite cells")
    bad = {k: np.argwhere(~np.isfinite(got[k])).tolist() for k in range(7)}
    assert bad == {rule.U: [[1, 40, 30]], rule.V: [[1, 80, 60]], rule.UU: [[1, 40, 30]], rule.VV: [[1, 80, 60]],
                   rule.UV: [[1, 40, 30], [1, 80, 60]], rule.P: [[0, 0, 0], [1, 17, 33]], rule.PP: [[0, 0, 0], [1, 17, 33]]}
    assert np.isnan(got[rule.U][1, 40, 30]) and got[rule.V][1, 80, 60] == -np.inf and got[rule.VV][1, 80, 60] == np.inf
    assert got[rule.UV][1, 80, 60] == -np.inf and got[rule.P][0, 0, 0] == np.inf and np.isnan(got[rule.PP][1, 17, 33])


@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (7, 9)], ids=["61x81", "7x9"])
def test_denormals_are_kept_zero_signs_follow_ieee_and_a_quiescent_field_gives_plus_zero(sfl, dim_x, dim_y):
    cap = sfl.capi
    tiny, zeros = vc.texture("tiny", dim_x, dim_y), vc.texture("zeros", dim_x, dim_y)
    assert vc.denormals(tiny.v) >= 5 and vc.denormals(tiny.rhs) >= 5 and vc.negative_zeros(zeros.v) >= 5 and vc.numpy_keeps_denormals()
    v = np.stack([tiny.v, zeros.v, np.zeros_like(tiny.v)])
    p = np.stack([tiny.rhs, zeros.rhs, np.zeros_like(tiny.rhs)])
    dye = np.stack([tiny.dye, zeros.dye, np.zeros_like(tiny.dye)])
    with sfl.BatchSolver(dim_x, dim_y, 3) as b, sfl.Solver(dim_x, dim_y) as c:
        b.mean_start(rule.ALL, 0)
        upload(b, cap, v, p, dye, False)
        b.mean_sample()
        one = planes(b, rule.ALL)
        b.mean_sample()
        b.mean_sample()
        three = planes(b, rule.ALL)
        c.mean_start(rule.ALL, 0)
        upload(c, cap, v[:1], p[:1], dye[:1], True)
        for _ in range(3):
            c.mean_sample()
        ctx = planes(c, rule.ALL)
    assert_planes_equal(one, rule.sums(rule.ALL, [(v, p, dye)]), "one sample")
    assert_planes_equal(three, rule.sums(rule.ALL, [(v, p, dye)] * 3), "three samples")
    assert_planes_equal(ctx, {k: a[:1] for k, a in three.items()}, "the context holds what member 0 holds")
    # a denormal converts exactly: the sum of one sample IS the value, and its square is there too (2^-298 is a normal double)
    assert one[rule.U][0].tobytes() == tiny.v[..., 0].astype(np.float64).tobytes() and one[rule.P][0].tobytes() == tiny.rhs.astype(np.float64).tobytes()
    small = (tiny.v[..., 0] != 0) & (np.abs(tiny.v[..., 0]) < vc.TINY)
    assert small.any() and (one[rule.UU][0][small] > 0).all()
    # +0.0 + (-0.0) is +0.0: no plane of the zeros member holds a negative zero, wherever its velocity is zero
    for k in (rule.U, rule.V, rule.UU, rule.VV, rule.UV):
        at = (zeros.v[..., 0] == 0) & (zeros.v[..., 1] == 0)
        assert not np.signbit(three[k][1][at]).any() and (three[k][1][at] == 0).all()
    for k, a in three.items():
        assert a[2].tobytes() == bytes(a[2].nbytes), f"a quiescent field: plane {rule.NAMES[k]} is +0.0 everywhere"


# ---- 5. lifecycle ----------------------------------------------------------------------------------------------------------------
def test_info_restart_refusals_and_stop(sfl):
    cap = sfl.capi
    dim_x, dim_y, batch = 7, 5, 4
    (v, p, dye), = seeded_samples(batch, dim_y, dim_x, seed=5, n=1)
    with sfl.BatchSolver(dim_x, dim_y, batch) as b, sfl.BatchSolver(dim_x, dim_y, batch) as plain, sfl.Solver(dim_x, dim_y) as c:
        assert b.mean_info() == (0, 0, 0, 0) and c.mean_info() == (0, 0, 0, 0)
        for s, lead in ((b, False), (plain, False), (c, True)):
            upload(s, cap, v, p, dye, lead)
        for s, name in ((b, "sfl_batch_mean"), (c, "sfl_mean")):
            with pytest.raises(sfl.SflError, match=f"{name}_sample: no averages to add to") as e:
                s.mean_sample()
            assert e.value.code == cap.ERR_STATE
            with pytest.raises(sfl.SflError, match=f"{name}_download: no averages to download") as e:
                s.mean_sums(rule.U)
            assert e.value.code == cap.ERR_STATE
        b.mean_start(rule.VELOCITY | rule.DYE, 2, 1, 2)
        b.step_n(5, DT, DX, ITERS, OMEGA)
        b.mean_sample()
        assert b.mean_info() == (9, 2, 3, 5)
        with pytest.raises(sfl.SflError, match="sfl_batch_mean_download: plane 5 belongs to group 4, which is not in the mask 9") as e:
            b.mean_sums(rule.P)
        assert e.value.code == cap.ERR_INVALID
        with pytest.raises(sfl.SflError, match=r"sfl_batch_mean_download: plane must be one of SFL_MEAN_PLANE_\*, 0\.\.9 \(got 10\)"):
            b.mean_sums(10)
        for first, count in ((0, 1), (1, 3), (3, 1), (0, 4)):
            with pytest.raises(sfl.SflError, match=r"sfl_batch_mean_download: members .* are not inside the recorded \[1, 1 \+ 2\)") as e:
                b.mean_sums(rule.U, first, count)
            assert e.value.code == cap.ERR_INVALID
        out = np.empty((2, dim_y, dim_x), np.float64)
        rc = b._lib.sfl_batch_mean_download(b._h, rule.U, 1, 2, out.ctypes.data, out.nbytes - 8)
        assert rc == cap.ERR_INVALID and "a plane of 2 members of 35 values of 8 bytes is 560 bytes, got 552" in b._lib.sfl_last_error().decode()
        assert b.mean_sums(rule.U).shape == (2, dim_y, dim_x) and b.mean_sums(rule.R, 2, 1).dtype == np.uint64
        # a restart begins anew from zero, with another mask and range
        b.mean_start(rule.PRESSURE, 0, 0, 4)
        assert b.mean_info() == (4, 0, 0, 0)
        assert all(a.tobytes() == bytes(a.nbytes) for a in planes(b, rule.PRESSURE).values())
        held = b.download(cap.FIELD_PRESSURE)
        b.mean_sample()
        assert_planes_equal(planes(b, rule.PRESSURE), rule.sums(rule.PRESSURE, [(None, held, None)]), "after the restart")
        # means and central moments are formed in float64 from the sums
        b.mean_start(rule.VELOCITY | rule.STRESS, 1)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        sums = planes(b, 3)
        m, rs, want = b.means(), b.reynolds_stress(), rule.reynolds_stress(sums, 3)
        assert sorted(m) == ["U", "UU", "UV", "V", "VV"] and m["U"].tobytes() == (sums[rule.U] / 3.0).tobytes()
        assert all(rs[k].tobytes() == want[k].tobytes() for k in ("uu", "vv", "uv", "tke")) and (rs["tke"] >= 0).any()
        # after a stop a download is refused and the steps leave what a batch that never averaged leaves
        plain.step_n(5, DT, DX, ITERS, OMEGA)
        plain.step_n(3, DT, DX, ITERS, OMEGA)
        b.mean_stop()
        b.mean_stop()
        assert b.mean_info() == (0, 0, 0, 0)
        with pytest.raises(sfl.SflError, match="sfl_batch_mean_download: no averages to download"):
            b.mean_sums(rule.U)
        b.step_n(2, DT, DX, ITERS, OMEGA)
        plain.step_n(2, DT, DX, ITERS, OMEGA)
        assert zero_counts(b.distance(plain))
        # the context's calls: the same rules
        c.mean_start(rule.STRESS, 1)
        c.step(DT, DX, ITERS, OMEGA)
        c.step_n(2, DT, DX, ITERS, OMEGA)
        assert c.mean_info() == (2, 1, 3, 3)
        with pytest.raises(sfl.SflError, match="sfl_mean_download: plane 0 belongs to group 1, which is not in the mask 2"):
            c.mean_sums(rule.U)
        out = np.empty((dim_y, dim_x), np.float64)
        rc = c._lib.sfl_mean_download(c._h, rule.UU, out.ctypes.data, out.nbytes + 8)
        assert rc == cap.ERR_INVALID and "sfl_mean_download: a plane of 35 values of 8 bytes is 280 bytes, got 288" in c._lib.sfl_last_error().decode()
        assert c.mean_sums(rule.UU).shape == (1, dim_y, dim_x)
        c.mean_stop()
        assert c.mean_info() == (0, 0, 0, 0)
