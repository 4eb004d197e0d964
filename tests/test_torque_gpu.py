"""Torque on the GPU (include/sfl.h "TORQUE"; csrc/torque.hip): the samplers of a batch and of a whole-domain context against
tests/torque_rule.py -- the header's rule in numpy, whose own sanity tests/test_torque.py checks.  Every comparison is bit for
bit, on the bytes of the 64-byte records: there is no tolerance anywhere.

Shapes: a batch of 7 x 5 with one solid cell (a member smaller than a wavefront) and 2 x 2 with all 16 masks; 61 x 81 x 3 with a disc, a seeded mask and an
empty member, labels and pivots per member, 16 bodies, one of them without a face; a large-member batch 96 x 96 x 2 (no solids
there: zeros and the pivots); contexts 67 x 35 and 130 x 70, whose flat arrays end in a partial group of 16, and 515 x 260 (several workgroups; most words skipped; channel walls
labelled 0); 9 x 9 with a
checkerboard and a pivot 2^23 cells away, where s > 0.  Fields: what three steps with forces left; magnitudes 1e-44..1e37 with
both signs and -0.0f; NaN and +-Inf planted in p and in ONE velocity component of a third of the wet cells; denormals only; all
zeros.  Pivots: seeded half-integers, negative ones and ones outside the grid included."""
import numpy as np
import pytest

import friction_rule
import load_rule
import test_friction_gpu as fg
import test_loads_gpu as lg
import test_solids_gpu as sg
import torque_rule as rule
from conftest import assert_bit_equal, random_fields

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = sg.DT, sg.DX, sg.ITERS, sg.OMEGA
F = np.float32
labels_of, assert_records_equal = lg.labels_of, lg.assert_records_equal


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def pivots_of(shape, dim_x, dim_y, seed):
    """Seeded pivots in HALF cells, int32 of `shape` + (2,): within two grid widths of the grid, either side of it."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(-2 * dim_x, 4 * dim_x, shape), rng.integers(-2 * dim_y, 4 * dim_y, shape)], axis=-1).astype(np.int32)


def denormal_fields(shape, seed):
    """p and v whose every value is a denormal of either sign (or, one in eight, a zero of either sign)."""
    rng = np.random.default_rng(seed)

    def one(sh):
        bits = rng.integers(1, 1 << 23, sh, dtype=np.uint32) | (rng.integers(0, 2, sh, dtype=np.uint32) << np.uint32(31))
        bits[rng.random(sh) < 0.125] &= np.uint32(0x80000000)
        return bits.view(F)
    return one(shape), one(shape + (2,))


def want_of(p, v, masks, labels, bodies, pivot2):
    """The rule's records of every member: DTYPE[batch, bodies].  masks / labels / pivot2: per member, or one for all."""
    out = np.zeros((len(p), bodies), rule.DTYPE)
    for m in range(len(p)):
        solid = masks if masks.ndim == 2 else masks[m]
        lab = None if labels is None else labels if labels.ndim == 2 else labels[m]
        piv = None if pivot2 is None else pivot2 if pivot2.ndim == 2 else pivot2[m]
        out[m] = rule.torque(p[m], v[m], solid, lab, bodies, piv)
    return out


def field_cases(masks, seed, stepped=None):
    """name -> (p, v) of every member."""
    shape = masks.shape
    cases = {"1e-44..1e37": (lg.wide_pressure(shape, seed), fg.wide_velocity(shape, seed + 1)),
             "nonfinite": (lg.nonfinite_pressure(masks, seed + 2), fg.nonfinite_velocity(masks, seed + 3)),
             "denormals": denormal_fields(shape, seed + 4),
             "zeros": (np.zeros(shape, F), np.zeros(shape + (2,), F))}
    if stepped is not None:
        cases["three steps with forces"] = stepped
    return cases


def set_fields(sfl, x, p, v):
    x.upload(sfl.capi.FIELD_PRESSURE, p)
    x.upload(sfl.capi.FIELD_VELOCITY, v)


def set_pivots(x, pivot2):
    x.set_body_pivots(None if pivot2 is None else pivot2 / 2.0)


# ---- batches ---------------------------------------------------------------------------------------------------------------
def test_a_member_smaller_than_a_wavefront_with_one_solid_cell(sfl):
    dim_x, dim_y = 7, 5
    solid = np.zeros((dim_y, dim_x), bool)
    solid[2, 4] = True
    pivot2 = np.array([[9, 5]], np.int32)   # the cell's own centre: (4.5, 2.5)
    with sfl.BatchSolver(dim_x, dim_y, 2) as b:
        b.set_solids(solid)
        for name, (p, v) in field_cases(np.stack([solid, solid]), 40).items():
            set_fields(sfl, b, p, v)
            for piv in (None, pivot2):
                set_pivots(b, piv)
                want = want_of(p, v, solid, None, 1, piv)
                assert_records_equal(b.torque(), want, f"7x5 {name}")
                assert (want["faces"] == 4).all()
        assert (b.body_pivots() == [[[4.5, 2.5]]] * 2).all()
    # ... and the smallest member there is: 2 x 2 with all 16 masks as one batch of 16, pivots per member
    masks = sg.masks_of(2, 2)
    pivot2 = pivots_of((16, 1), 2, 2, 44)
    with sfl.BatchSolver(2, 2, 16) as b:
        b.set_solids(masks)
        some_face = False
        for name, (p, v) in field_cases(masks, 45).items():
            set_fields(sfl, b, p, v)
            for piv in (None, pivot2):
                set_pivots(b, piv)
                want = want_of(p, v, masks, None, 1, piv)
                assert_records_equal(b.torque(), want, f"2x2 {name}")
                some_face |= bool(want["mp"].any() and want["mf"].any())
        assert some_face and want["faces"].max() == 4 and not want[0]["faces"].any() and not want[15]["faces"].any()


def test_a_batch_with_masks_labels_and_pivots_per_member_and_16_bodies(sfl):
    cap, dim_x, dim_y, bodies = sfl.capi, 61, 81, 16
    masks = sg.masks_of(dim_x, dim_y)   # a disc, a seeded mask, no solid cell
    labels = labels_of("each", bodies, 3, dim_x, dim_y).copy()
    labels[0][labels[0] == 16] = 15     # member 0: body 16 has no cell, hence no face
    pivot2 = pivots_of((3, bodies), dim_x, dim_y, 41)
    with lg.stepped_batch(sfl, dim_x, dim_y, masks) as b:
        stepped = (b.download(cap.FIELD_PRESSURE), b.download(cap.FIELD_VELOCITY))
        b.set_bodies(labels, bodies)
        seen_nonfinite = False
        for name, (p, v) in field_cases(masks, 42, stepped).items():
            set_fields(sfl, b, p, v)
            for piv in (pivot2, pivot2[1], None):   # per member, shared, none
                set_pivots(b, piv)
                want = want_of(p, v, masks, labels, bodies, piv)
                got = b.torque()
                assert_records_equal(got, want, f"61x81 {name}")
                seen_nonfinite |= bool(want["nonfinite_p"].any() and want["nonfinite_t"].any())
            assert want[0, 15]["faces"] == 0 and want[0, :15]["faces"].all() and not want[2]["faces"].any()
            assert got[0, 15].tobytes() == bytes(64), "a body without a face, no pivot: all zeros"
            assert_bit_equal(b.download(cap.FIELD_VELOCITY), v, "the velocity held")
            assert_bit_equal(b.download(cap.FIELD_PRESSURE), p, "the pressure held")
        assert seen_nonfinite
        # the figures of the load and of the friction record are the torque's own: s = 0 here
        set_pivots(b, pivot2)
        got, loads, friction = b.torque(), b.loads(), b.friction()
        assert (got["exp2_p"] == loads["exp2"]).all() and (got["exp2_f"] == friction["exp2"]).all()
        assert (got["faces"] == loads["faces"].sum(axis=-1)).all() and got["max_abs_t"].tobytes() == friction["max_abs_t"].tobytes()
        assert got["pivot2"].tobytes() == pivot2.tobytes() and (b.body_pivots() * 2 == pivot2).all()
        # a range of members at the far end
        assert_records_equal(b.torque(1, 2), want_of(p, v, masks, labels, bodies, pivot2)[1:], "members [1, 3)")
        # another number of bodies puts the pivots back
        b.set_bodies(None)
        assert (b.body_pivots() == 0).all() and b.torque()["pivot2"].tobytes() == bytes(3 * 8)


def test_moving_the_pivot_changes_the_sums_by_the_load_and_the_friction_records(sfl):
    """The header's identity, on the device: mp(pivot + (a2, b2)) - mp(pivot) == -(a2 * fy - b2 * fx) of the load record, and mf
    the same with the friction record."""
    dim_x, dim_y = 61, 81
    masks = sg.masks_of(dim_x, dim_y)
    with lg.stepped_batch(sfl, dim_x, dim_y, masks) as b:
        at0, loads, friction = b.torque(), b.loads(), b.friction()
        a2, b2 = 61, -34
        b.set_body_pivots(np.array([[a2 / 2.0, b2 / 2.0]]))
        moved = b.torque()
        assert (moved["exp2_p"] == at0["exp2_p"]).all(), "s = 0 at both pivots"
        for m in range(3):
            assert int(moved["mp"][m, 0]) - int(at0["mp"][m, 0]) == -(a2 * int(loads["fy"][m, 0]) - b2 * int(loads["fx"][m, 0]))
            assert int(moved["mf"][m, 0]) - int(at0["mf"][m, 0]) == -(a2 * int(friction["fy"][m, 0]) - b2 * int(friction["fx"][m, 0]))
        assert at0["mp"][:2].all() and at0["mf"][:2].all()


def test_a_large_member_batch_reports_zeros_and_the_pivots(sfl):
    dim_x, dim_y = 96, 96
    pivot2 = pivots_of((2, 1), dim_x, dim_y, 43)
    want = np.zeros((2, 1), rule.DTYPE)
    want["pivot2"] = pivot2
    with sfl.BatchSolver(dim_x, dim_y, 2, large=True) as big:   # no solids there
        assert big.torque().tobytes() == bytes(2 * 64)
        set_pivots(big, pivot2)
        assert_records_equal(big.torque(), want, "no solids: zeros and the pivots")
        big.torque_start(1, 2)
        big.step_n(2, DT, DX, 2, OMEGA)
        assert big.torque_info() == (2, 2, 2, 1)
        assert_records_equal(big.torque_history(), np.stack([want, want]), "samples without solids")


# ---- contexts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(67, 35), (130, 70), (515, 260)], ids=["67x35", "130x70", "515x260"])
def test_a_contexts_torque_is_the_rules_and_a_batch_members(sfl, dim_x, dim_y):
    cap = sfl.capi
    assert (dim_x * dim_y) % 16 != 0, "the flat array ends in a partial group"
    channel = (dim_x, dim_y) == (515, 260)   # several workgroups, most words skipped: the loads' channel walls, labelled 0, and two discs
    if channel:
        solid, walls = lg.channel_with_disc(dim_x, dim_y)
        labellings = [(None, 1), (walls, 2), (walls, 16)]
    else:
        solid = sg.mask_of("seeded", dim_x, dim_y) | sg.mask_of("disc", dim_x, dim_y)
        labellings = [(None if bodies == 1 else labels_of("shared", bodies, 1, dim_x, dim_y), bodies) for bodies in (1, 3, 16)]
    fits_a_batch = dim_x * dim_y <= 6144
    with sfl.Solver(dim_x, dim_y) as c:
        v0, col = random_fields(dim_x, dim_y, 300, vamp=40.0)[:2]
        c.upload(cap.FIELD_VELOCITY, v0)
        c.upload(cap.FIELD_COLOR, col)
        assert c.torque().tobytes() == bytes(64), "no solids: zero records"
        c.set_solids(solid)
        c.queue_forces([(dim_x // 2, 1)], [(25.0, -10.0)])
        c.step_n(3, DT, DX, ITERS, OMEGA)
        stepped = (c.download(cap.FIELD_PRESSURE)[None], c.download(cap.FIELD_VELOCITY)[None])
        batch = sfl.BatchSolver(dim_x, dim_y, 1) if fits_a_batch else None
        if batch:
            batch.set_solids(solid)
        for name, (p, v) in field_cases(solid[None], 50, stepped).items():
            set_fields(sfl, c, p[0], v[0])
            if batch:
                set_fields(sfl, batch, p, v)
            for labels, bodies in labellings:
                c.set_bodies(labels, bodies)
                if batch:
                    batch.set_bodies(labels, bodies)
                for piv in (None, pivots_of((bodies,), dim_x, dim_y, 51 + bodies)):
                    set_pivots(c, piv)
                    want = want_of(p, v, solid, labels, bodies, piv)
                    got = c.torque()
                    assert_records_equal(got, want, f"{dim_x}x{dim_y} {name}, {bodies} bodies")
                    if batch:
                        set_pivots(batch, piv)
                        assert batch.torque().tobytes() == got.tobytes(), "a batch member of the same shape, mask, labels, pivots and fields"
            assert want[0, :2]["faces"].all() and not want[0, 2:]["faces"].any() if channel else want["faces"].all()
            assert_bit_equal(c.download(cap.FIELD_VELOCITY), v[0], "the velocity held")
            assert_bit_equal(c.download(cap.FIELD_PRESSURE), p[0], "the pressure held")
        if batch:
            batch.close()
        assert c.torque().tobytes() == c.torque().tobytes()


def checkerboard_case():
    """9 x 9, every other cell solid, the pivot 2^23 cells away on both axes: L(faces) + L(max_arm2) > 30."""
    j, i = np.mgrid[0:9, 0:9]
    solid = (i + j) % 2 == 1
    pivot2 = np.array([[1 << 24, -(1 << 24)]], np.int32)
    rng = np.random.default_rng(60)
    p = (rng.standard_normal((1, 9, 9)) * 1e3).astype(F)
    v = (rng.standard_normal((1, 9, 9, 2)) * 1e-3).astype(F)
    return solid, pivot2, p, v


def test_the_exponents_are_raised_where_faces_times_arm_would_overflow(sfl):
    solid, pivot2, p, v = checkerboard_case()
    want = want_of(p, v, solid, None, 1, pivot2)
    s = int(want["exp2_p"][0, 0]) - load_rule.exponent(want["max_abs_p"][0, 0])
    assert want["faces"][0, 0] >= 32 and s >= 1 and s == rule.shift(want["faces"][0, 0], want["max_arm2"][0, 0])
    assert int(want["exp2_f"][0, 0]) - load_rule.exponent(want["max_abs_t"][0, 0]) == s
    with sfl.BatchSolver(9, 9, 1) as b, sfl.Solver(9, 9) as c:
        for x, pp, vv in ((b, p, v), (c, p[0], v[0])):
            x.set_solids(solid)
            set_fields(sfl, x, pp, vv)
            set_pivots(x, pivot2)
            assert_records_equal(x.torque(), want, "s > 0")
            # FLT_MAX on every face: the products are as large as the rule lets them be
            set_fields(sfl, x, np.full_like(pp, np.finfo(F).max), np.full_like(vv, -np.finfo(F).max))
            big = want_of(np.full_like(p, np.finfo(F).max), np.full_like(v, -np.finfo(F).max), solid, None, 1, pivot2)
            assert_records_equal(x.torque(), big, "s > 0, FLT_MAX")
        # one component beyond the bound is refused and names the body
        with pytest.raises(sfl.SflError, match=r"sfl_set_body_pivots: pivot2\[1\] = -16777217 of body 1 is beyond") as e:
            c.set_body_pivots(np.array([[0.0, -(2.0 ** 23) - 0.5]]))
        assert e.value.code == sfl.capi.ERR_INVALID and (c.body_pivots() * 2 == pivot2).all()
        with pytest.raises(ValueError, match="multiple of 0.5"):
            c.set_body_pivots(np.array([[0.25, 0.0]]))


# ---- the recorders ---------------------------------------------------------------------------------------------------------
def batch_run(sfl, calls, every, capacity, recorder, pivots=None, change_at=None, each=False):
    """A 33 x 18 batch of three members (no solid cell, a plate, all solid) with labels and 3 bodies run through `calls` --
    with the torque recorder and the loads and friction recorders beside it, or with the loop `step; torque()` it replaces.
    pivots: {steps done: pivot2} set before the step call (recorder) / the step (loop) that follows.  Returns (torque
    samples, fields, torque_info, loads samples, friction samples)."""
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    labels = labels_of("each", 3, 3, dim_x, dim_y)
    pivots = pivots or {}
    with sg.make(sfl, dim_x, dim_y, masks) as b:
        for step, records in sg.forces_of(dim_x, dim_y, masks).items():
            sg.queue(b, records, step)
        b.set_bodies(labels, 3)
        dts = [DT, DT / 2, DT * 1.5]
        step = (lambda n: b.step_n_each(n, dts, DX, [ITERS, ITERS + 1, ITERS + 2], OMEGA)) if each else (lambda n: b.step_n(n, DT, DX, ITERS, OMEGA))
        done = 0
        if recorder:
            b.loads_start(every, capacity)
            b.friction_start(every, capacity)
            b.torque_start(every, capacity)
            for n in calls:
                if done in pivots:
                    set_pivots(b, pivots[done])
                step(n)
                done += n
            return b.torque_history(), sg.download_all(sfl, b), b.torque_info(), b.loads_history(), b.friction_history()
        samples = []
        for _ in range(sum(calls)):
            if done in pivots:
                set_pivots(b, pivots[done])
            step(1)
            done += 1
            if done % every == 0:
                samples.append(b.torque())
        return np.stack(samples), sg.download_all(sfl, b), None, None, None


@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
def test_a_batchs_recorder_of_every_second_step_over_calls_that_leave_remainders(sfl, each):
    pivot2 = pivots_of((3, 3), 33, 18, 70)
    want, want_fields, _, _, _ = batch_run(sfl, [8], 2, 4, False, {0: pivot2}, each=each)
    got, fields, info, _, _ = batch_run(sfl, [3, 2, 3], 2, 4, True, {0: pivot2}, each=each)
    assert info == (4, 4, 8, 3) and got.shape == (4, 3, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6, 8")
    assert want["faces"][:, 1:].any() and len({s.tobytes() for s in want}) == 4 and (got["pivot2"] == pivot2).all()
    sg.assert_fields_equal(fields, want_fields, "the fields after the calls are those of a run without a recorder")


def test_step_n_is_n_steps_with_a_torque_after_each_and_pivots_change_mid_recording(sfl):
    first, second = pivots_of((3,), 33, 18, 71), pivots_of((3, 3), 33, 18, 72)
    plan = {0: first, 2: second, 3: None}
    want, want_fields, _, _, _ = batch_run(sfl, [5], 1, 5, False, plan)
    got, fields, info, _, _ = batch_run(sfl, [2, 1, 2], 1, 5, True, plan)
    assert info == (5, 5, 5, 3)
    assert_records_equal(got, want, "a sample behind every step")
    assert (got["pivot2"][:2] == first).all() and (got["pivot2"][2] == second).all() and not got["pivot2"][3:].any(), "the new pivots hold from the next sample"
    sg.assert_fields_equal(fields, want_fields, "fields")
    whole, _, _, _, _ = batch_run(sfl, [5], 1, 5, True, {0: first})
    assert_records_equal(whole, batch_run(sfl, [5], 1, 5, False, {0: first})[0], "one step_n(5)")


def test_a_recorder_without_room_refuses_the_call_whole_and_a_restart_keeps_going(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    with lg.stepped_batch(sfl, dim_x, dim_y, masks, steps=1) as b:
        before = sg.download_all(sfl, b)
        b.torque_start(2, 2)
        for call in (lambda: b.step_n(6, DT, DX, ITERS, OMEGA), lambda: b.step_n_each(6, DT, DX, ITERS, OMEGA)):
            with pytest.raises(sfl.SflError, match="torque recorder has room for 2 more samples") as e:
                call()
            assert e.value.code == sfl.capi.ERR_STATE
        assert b.torque_info() == (0, 2, 0, 1)
        sg.assert_fields_equal(sg.download_all(sfl, b), before, "a refused call")
        with pytest.raises(sfl.SflError, match="the torque recorder is on") as e:
            b.set_bodies(labels_of("shared", 3, 3, dim_x, dim_y), 3)
        assert e.value.code == sfl.capi.ERR_STATE and b.bodies_info() == (1, False, False)
        b.step_n(4, DT, DX, ITERS, OMEGA)
        assert b.torque_info() == (2, 2, 4, 1)
        b.step_n(1, DT, DX, ITERS, OMEGA)   # completes no sample: let through
        with pytest.raises(sfl.SflError, match="the torque recorder has room for 0 more samples"):
            b.step_n(1, DT, DX, ITERS, OMEGA)
        kept = b.torque_history()
        b.torque_start(2, 2)   # a restart: the counts are 0 again, the buffer serves on
        assert b.torque_info() == (0, 2, 0, 1)
        b.step_n(2, DT, DX, ITERS, OMEGA)
        p, v = b.download(sfl.capi.FIELD_PRESSURE), b.download(sfl.capi.FIELD_VELOCITY)
        assert_records_equal(b.torque_history(), want_of(p, v, masks, None, 1, None)[None], "the first sample after the restart")
        b.torque_stop()
        assert b.torque_info() == (0, 0, 0, 1) and kept.shape == (2, 3, 1)
    with sfl.Solver(dim_x, dim_y) as c:
        c.set_solids(masks[1])
        c.step(DT, DX, ITERS, OMEGA)
        v = c.download(sfl.capi.FIELD_VELOCITY)
        c.torque_start(1, 2)
        with pytest.raises(sfl.SflError, match="torque recorder has room for 2 more samples") as e:
            c.step_n(3, DT, DX, ITERS, OMEGA)
        assert e.value.code == sfl.capi.ERR_STATE and c.torque_info() == (0, 2, 0, 1)
        assert_bit_equal(c.download(sfl.capi.FIELD_VELOCITY), v, "a refused call")
        with pytest.raises(sfl.SflError, match="sfl_set_bodies: the torque recorder is on"):
            c.set_bodies(None)


def context_run(sfl, torque, calls=(3, 2, 3)):
    """A 33 x 18 context with a disc, 3 bodies and pivots run through `calls` with the history, the loads recorder and the
    friction recorder on, and (torque True) the torque recorder too; or (torque None) the loop `step; torque()` after every
    second step.  Returns (fields, history, loads samples, friction samples, torque samples or None, torque_info or None)."""
    cap, dim_x, dim_y = sfl.capi, 33, 18
    solid = sg.mask_of("disc", dim_x, dim_y)
    with sfl.Solver(dim_x, dim_y) as c:
        v, col = random_fields(dim_x, dim_y, 301, vamp=40.0)[:2]
        c.upload(cap.FIELD_VELOCITY, v)
        c.upload(cap.FIELD_COLOR, col)
        c.set_solids(solid)
        c.set_bodies(labels_of("shared", 3, 1, dim_x, dim_y), 3)
        set_pivots(c, pivots_of((3,), dim_x, dim_y, 73))
        c.queue_forces([(dim_x // 2, 1)], [(25.0, -10.0)])
        c.queue_forces([(2, dim_y // 2)], [(-15.0, 5.0)], 3)
        fields = lambda: tuple(c.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
        if torque is None:
            samples = []
            for k in range(1, sum(calls) + 1):
                c.step(DT, DX, ITERS, OMEGA)
                if k % 2 == 0:
                    samples.append(c.torque())
            return fields(), None, None, None, np.stack(samples), None
        c.history_start(1, 8)
        c.loads_start(2, 4)
        c.friction_start(2, 4)
        if torque:
            c.torque_start(2, 4)
        for n in calls:
            c.step_n(n, DT, DX, ITERS, OMEGA)
        return fields(), c.history(), c.loads_history(), c.friction_history(), (c.torque_history() if torque else None), (c.torque_info() if torque else None)


def test_all_four_recorders_at_once_leave_the_fields_and_the_other_three_unchanged(sfl):
    loop_fields, _, _, _, want, _ = context_run(sfl, None)
    without = context_run(sfl, False)
    fields, hist, loads, friction, got, info = context_run(sfl, True)
    assert info == (4, 4, 8, 3) and got.shape == (4, 1, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6, 8")
    assert want["faces"].all() and want["mp"].any() and want["mf"].any() and len({s.tobytes() for s in want}) == 4
    sg.assert_fields_equal(fields, without[0], "the fields with and without the torque recorder")
    sg.assert_fields_equal(fields, loop_fields, "... and those of the loop of single steps")
    assert len(hist) == 8 and hist.tobytes() == without[1].tobytes(), "the history's records, bit for bit"
    assert loads.shape == (4, 1, 3) and loads.tobytes() == without[2].tobytes(), "the loads samples"
    assert friction.tobytes() == without[3].tobytes(), "the friction samples"


def test_a_contexts_recorder_keeps_the_seams_where_its_samples_are_zeros_and_pivots(sfl):
    """Without solids sfl_step_n keeps its step seams while a torque recorder is on (130 x 70 on the tiled kernels) and counts each
    step inside that loop: the samples are zero but for pivot2, and the fields those of a run without a recorder."""
    cap, dim_x, dim_y = sfl.capi, 130, 70
    pivot2 = np.array([[7, -3]], np.int32)

    def run(recorder):
        with sfl.Solver(dim_x, dim_y) as c:
            v, col = random_fields(dim_x, dim_y, 303, vamp=40.0)[:2]
            c.upload(cap.FIELD_VELOCITY, v)
            c.upload(cap.FIELD_COLOR, col)
            c.set_option(cap.OPT_ADVECT_KERNEL, 2)
            if recorder:
                set_pivots(c, pivot2)
                c.torque_start(2, 4)
            for n in (3, 3):
                c.step_n(n, DT, DX, ITERS, OMEGA)
            fields = tuple(c.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
            return fields, (c.torque_info(), c.torque_history()) if recorder else None

    plain, _ = run(False)
    fields, (info, samples) = run(True)
    want = np.zeros((3, 1, 1), rule.DTYPE)
    want["pivot2"] = pivot2
    assert info == (3, 4, 6, 1), info
    assert_records_equal(samples, want, "zeros and the pivot")
    sg.assert_fields_equal(fields, plain, "the fields are those of a run without a recorder")


def test_torque_xy_scales_by_dx_rho_and_the_viscosity_that_is_set(sfl):
    """This checks the binding, not the physics."""
    dim_x, dim_y = 61, 81
    disc = sg.mask_of("disc", dim_x, dim_y)
    nus = np.array([0.0, 1e-3, 0.05], F)
    with sg.make(sfl, dim_x, dim_y, disc, batch=3) as b:
        b.set_body_pivots(np.array([[dim_x // 2, dim_y // 2 + 0.5]]))
        b.set_viscosity(nus, 2)
        b.queue_forces([0, 1, 2], [(3, dim_y // 2)] * 3, [(30.0, 4.0)] * 3)
        b.torque_start(1, 2, 1, 2)
        b.step_n(2, DT, DX, ITERS, OMEGA)
        rec = b.torque()
        assert rec["faces"].all() and rec["mp"].any() and rec["mf"].any()
        want = rule.torque_xy(rec, 0.7, 1.2, nus.astype(np.float64)[:, None])
        assert b.torque_xy(0.7, 1.2).tobytes() == want.tobytes() and (want[0, :, 1] == 0).all() and want[1:, :, 1].all()
        hist = b.torque_history()
        assert hist.shape == (2, 2, 1) and hist[1].tobytes() == rec[1:].tobytes()
        assert b.torque_history_xy(0.7, 1.2).tobytes() == rule.torque_xy(hist, 0.7, 1.2, nus.astype(np.float64)[1:, None]).tobytes()
