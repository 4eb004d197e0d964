"""Friction on the GPU (include/sfl.h "FRICTION"; csrc/friction.hip): the samplers of a batch and of a whole-domain context
against tests/friction_rule.py -- the header's rule in numpy, whose own sanity tests/test_friction.py checks.  Every
comparison is bit for bit, on the bytes of the 48-byte records: there is no tolerance anywhere.

Shapes, masks and labels are those of tests/test_loads_gpu.py, the smallest at which the walk can go wrong: 2 x 2 with all 16
masks as one batch of 16; 7 x 5, 33 x 18 (an odd width), 61 x 81 and 96 x 64 (the 6144-cell limit) as batches of three members
with a DIFFERENT mask each.  Velocities: what three steps with forces left; seeded magnitudes over 1e-44..1e37 with both signs
and -0.0f; NaN and +-Inf in ONE component of a third of the wet cells (a face's normal component must not matter) together
with NaN in cells that are not wet and in solid cells.  Contexts: 33 x 18, 96 x 64, 131 x 70 (a flat array that ends in a
partial group of 16, rows at odd addresses) and 515 x 260 (several workgroups; most words skipped; channel walls labelled 0)."""
import functools

import numpy as np
import pytest

import friction_rule as rule
import load_rule
import test_loads_gpu as lg
import test_solids_gpu as sg
from conftest import assert_bit_equal, random_fields

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = sg.DT, sg.DX, sg.ITERS, sg.OMEGA
F = np.float32
labels_of, assert_records_equal, stepped_batch = lg.labels_of, lg.assert_records_equal, lg.stepped_batch
COUNTS = ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ")


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def wide_velocity(shape, seed):
    """Both components with magnitudes 10^-44 .. 10^37 (denormals included), both signs, every tenth value -0.0f."""
    return np.stack([lg.wide_pressure(shape, seed), lg.wide_pressure(shape, seed + 1000)], axis=-1)


def nonfinite_velocity(masks, seed):
    """Seeded values; NaN, +Inf or -Inf in ONE component -- x or y, seeded -- of a third of the fluid cells that touch a solid
    one; NaN in both components of a tenth of the other fluid cells (not wet: no effect) and of every other solid cell."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal(masks.shape + (2,)).astype(F) * F(37.5)
    for m, solid in enumerate(masks):
        wet = np.zeros(solid.shape, bool)
        for j, i, _ in load_rule.wet_faces(solid):
            wet[j, i] = True
        pick = wet & (rng.random(solid.shape) < 1 / 3)
        n = int(pick.sum())
        jj, ii = np.nonzero(pick)
        v[m][jj, ii, rng.integers(0, 2, n)] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), n)
        v[m][~wet & ~solid & (rng.random(solid.shape) < 0.1)] = np.nan
        v[m][solid & (rng.random(solid.shape) < 0.5)] = np.nan
    return v


def want_of(v, masks, labels, bodies):
    """The rule's records of every member: DTYPE[batch, bodies].  masks / labels: per member, or one for all (2-D)."""
    out = np.zeros((len(v), bodies), rule.DTYPE)
    for m in range(len(v)):
        solid = masks if masks.ndim == 2 else masks[m]
        lab = None if labels is None else labels if labels.ndim == 2 else labels[m]
        out[m] = rule.friction(v[m], solid, lab, bodies)
    return out


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2)] + sg.SHAPES, ids=["2x2"] + sg.IDS)
def test_a_batchs_friction_is_the_rules(sfl, dim_x, dim_y):
    cap = sfl.capi
    masks = sg.masks_of(dim_x, dim_y)
    batch = len(masks)
    with stepped_batch(sfl, dim_x, dim_y, masks) as b:
        velocities = {"three steps with forces": b.download(cap.FIELD_VELOCITY), "1e-44..1e37": wide_velocity(masks.shape, 5),
                      "nonfinite": nonfinite_velocity(masks, 6)}
        some_face = False
        for name, v in velocities.items():
            b.upload(cap.FIELD_VELOCITY, v)
            for mode, bodies in lg.LABELLINGS:
                labels = labels_of(mode, bodies, batch, dim_x, dim_y)
                b.set_bodies(labels, bodies)
                want = want_of(v, masks, labels, bodies)
                some_face |= bool(want["faces"].any())
                got = b.friction()
                assert_records_equal(got, want, f"{dim_x}x{dim_y} {name}, labels {mode}, {bodies} bodies")
                assert got["faces"].tobytes() == b.loads()["faces"].tobytes(), "the faces are the loads' faces"
            assert_bit_equal(b.download(cap.FIELD_VELOCITY), v, "the velocity held")
        assert some_face
        nf = want_of(velocities["nonfinite"], masks, None, 1)
        assert dim_x * dim_y <= 35 or nf["nonfinite"].any(), "the nonfinite case has nonfinite faces"
        assert dim_x * dim_y <= 35 or (nf["nonfinite"] < nf["faces"].sum(axis=-1)).any(), "... and faces whose normal component alone is not finite"


def test_masks_and_labels_are_shared_or_per_member_independently_and_in_either_order(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    shared_mask = sg.mask_of("disc", dim_x, dim_y)
    v = wide_velocity(masks.shape, 8)
    each, shared = labels_of("each", 3, 3, dim_x, dim_y), labels_of("shared", 3, 3, dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, 3) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.set_bodies(each, 3)   # the labels first: no solids yet, zero records
        assert b.friction().tobytes() == bytes(3 * 3 * 48)
        b.set_solids(shared_mask)
        assert_records_equal(b.friction(), want_of(v, shared_mask, each, 3), "mask shared, labels per member")
        b.set_bodies(shared, 3)
        b.set_solids(masks)
        assert_records_equal(b.friction(), want_of(v, masks, shared, 3), "masks per member, labels shared")
        b.set_solids(None)
        assert b.friction().tobytes() == bytes(3 * 3 * 48), "solids cleared: zero records"
        b.set_solids(masks)
        b.set_bodies(None)
        assert_records_equal(b.friction(), want_of(v, masks, None, 1), "labels cleared: every solid cell is body 1")


def test_range_arguments_at_both_ends_of_the_batch_and_a_large_batch(sfl):
    dim_x, dim_y = 7, 5
    masks = sg.masks_of(dim_x, dim_y)
    v = wide_velocity(masks.shape, 9)
    labels = labels_of("each", 3, 3, dim_x, dim_y)
    want = want_of(v, masks, labels, 3)
    with sfl.BatchSolver(dim_x, dim_y, 3) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.set_solids(masks)
        b.set_bodies(labels, 3)
        for first, count in ((0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (0, 3)):
            assert_records_equal(b.friction(first, count), want[first:first + count], f"members [{first}, {first} + {count})")
        assert b.friction(3, 0).shape == (0, 3) and b.friction(0, 0).shape == (0, 3)
        for first, count in ((3, 1), (-1, 1), (2, 2)):
            with pytest.raises(sfl.SflError, match="sfl_batch_friction: members .* not inside the batch") as e:
                b.friction(first, count)
            assert e.value.code == sfl.capi.ERR_INVALID
    with sfl.BatchSolver(128, 128, 2, large=True) as big:   # no solids there: zero records, and a recorder of zeros
        assert big.friction().tobytes() == bytes(2 * 48)
        big.friction_start(1, 2)
        big.step_n(2, DT, DX, 2, OMEGA)
        assert big.friction_info() == (2, 2, 2, 1) and big.friction_history().tobytes() == bytes(2 * 2 * 48)


def test_friction_changes_no_field_ignores_the_pressure_and_two_runs_give_identical_bytes(sfl):
    dim_x, dim_y = 61, 81
    masks = sg.masks_of(dim_x, dim_y)
    labels = labels_of("each", 16, 3, dim_x, dim_y)
    with stepped_batch(sfl, dim_x, dim_y, masks) as b, stepped_batch(sfl, dim_x, dim_y, masks) as twin:
        b.set_bodies(labels, 16)
        twin.set_bodies(labels, 16)
        before = b.distance(twin)
        first = b.friction()
        after = b.distance(twin)
        for d in (before, after):
            assert all((d[c] == 0).all() for c in COUNTS), d
        assert first["faces"].any() and (first["fx"] != 0).any() and (first["fy"] != 0).any()
        assert b.friction().tobytes() == first.tobytes() == twin.friction().tobytes()
        assert_records_equal(first, want_of(b.download(sfl.capi.FIELD_VELOCITY), masks, labels, 16), "the stepped batch")
        loads_before = b.loads()
        b.upload(sfl.capi.FIELD_PRESSURE, lg.wide_pressure(masks.shape, 21))
        assert b.loads().tobytes() != loads_before.tobytes(), "the pressure load moved with the pressure ..."
        assert b.friction().tobytes() == first.tobytes(), "... and no byte of the friction did"


# ---- contexts --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", list(lg.CONTEXT_CASES), ids=[f"{x}x{y}" for x, y in lg.CONTEXT_CASES])
def test_a_contexts_friction_is_the_rules_and_a_batch_members(sfl, dim_x, dim_y):
    cap = sfl.capi
    kind = lg.CONTEXT_CASES[(dim_x, dim_y)]
    if kind == "channel+disc":
        solid, walls = lg.channel_with_disc(dim_x, dim_y)
        labellings = [(None, 1), (walls, 2), (walls, 16)]
    else:
        solid = sg.mask_of(kind, dim_x, dim_y)
        labellings = [(None, 1)] + [(labels_of("shared", bodies, 1, dim_x, dim_y), bodies) for bodies in (1, 3, 16)]
    fits_a_batch = dim_x * dim_y <= 6144
    with sfl.Solver(dim_x, dim_y) as c:
        v0, col = random_fields(dim_x, dim_y, 300, vamp=40.0)[:2]
        c.upload(cap.FIELD_VELOCITY, v0)
        c.upload(cap.FIELD_COLOR, col)
        assert c.friction().tobytes() == bytes(48), "no solids: zero records"
        c.set_solids(solid)
        c.queue_forces([(dim_x // 2, 1)], [(25.0, -10.0)])
        c.step_n(3, DT, DX, ITERS, OMEGA)
        velocities = {"three steps": c.download(cap.FIELD_VELOCITY), "1e-44..1e37": wide_velocity((1, dim_y, dim_x), 15)[0],
                      "nonfinite": nonfinite_velocity(solid[None], 16)[0]}
        batch = sfl.BatchSolver(dim_x, dim_y, 1) if fits_a_batch else None
        if batch:
            batch.set_solids(solid)
        for name, v in velocities.items():
            c.upload(cap.FIELD_VELOCITY, v)
            if batch:
                batch.upload(cap.FIELD_VELOCITY, v[None])
            for labels, bodies in labellings:
                c.set_bodies(labels, bodies)
                want = want_of(v[None], solid, labels, bodies)
                got = c.friction()
                assert_records_equal(got, want, f"{dim_x}x{dim_y} {name}, {bodies} bodies")
                assert got["faces"].tobytes() == c.loads()["faces"].tobytes(), "the faces are the loads' faces"
                if batch:
                    batch.set_bodies(labels, bodies)
                    assert batch.friction().tobytes() == got.tobytes(), "a batch member of the same shape, mask, labels and velocity"
            assert_bit_equal(c.download(cap.FIELD_VELOCITY), v, "the velocity held")
        if batch:
            batch.close()
        if kind == "channel+disc":
            assert want[0, 0]["faces"].all() and want[0, 1]["faces"].all() and not want[0, 2:]["faces"].any()
            everything = rule.friction(v, solid)[0]
            assert everything["faces"].sum() > want["faces"].sum(), "the walls labelled 0 are in no body"
        assert c.friction().tobytes() == c.friction().tobytes()


def test_a_contexts_friction_changes_no_field_and_ignores_the_pressure(sfl):
    """Two contexts stepped alike: every count of `distance` is zero before friction() and after it."""
    dim_x, dim_y = 131, 70
    solid = sg.mask_of("seeded", dim_x, dim_y)
    v, col = random_fields(dim_x, dim_y, 302, vamp=40.0)[:2]
    pair = []
    for _ in range(2):
        c = sfl.Solver(dim_x, dim_y)
        c.upload(sfl.capi.FIELD_VELOCITY, v)
        c.upload(sfl.capi.FIELD_COLOR, col)
        c.set_solids(solid)
        c.set_bodies(labels_of("shared", 16, 1, dim_x, dim_y), 16)
        c.step_n(2, DT, DX, ITERS, OMEGA)
        pair.append(c)
    c, twin = pair
    before = c.distance(twin)
    rec = c.friction()
    after = c.distance(twin)
    assert rec["faces"].any() and rec.tobytes() == twin.friction().tobytes()
    for d in (before, after):
        assert all(d[k] == 0 for k in COUNTS), d
    c.upload(sfl.capi.FIELD_PRESSURE, lg.wide_pressure((dim_y, dim_x), 22))
    assert c.friction().tobytes() == rec.tobytes(), "another pressure: no byte of the record changes"
    c.close()
    twin.close()


# ---- the recorders ---------------------------------------------------------------------------------------------------------
def batch_run(sfl, dim_x, dim_y, calls, recorder, each=False, labels=None, bodies=1, rec_range=(0, None), friction=True):
    """A stepped batch run through `calls` (steps per step call) -- with the friction recorder (every, capacity) and a loads
    recorder beside it (friction False: the loads recorder alone), or with the loop `step; friction()` it replaces.  Returns
    (friction samples [n, count, bodies], fields, friction_info or None, loads samples or None)."""
    masks = sg.masks_of(dim_x, dim_y)
    with sg.make(sfl, dim_x, dim_y, masks) as b:
        for step, records in sg.forces_of(dim_x, dim_y, masks).items():
            sg.queue(b, records, step)
        b.set_bodies(labels, bodies)
        dts = [DT, DT / 2, DT * 1.5]
        step = (lambda n: b.step_n_each(n, dts, DX, [ITERS, ITERS + 1, ITERS + 2], OMEGA)) if each else (lambda n: b.step_n(n, DT, DX, ITERS, OMEGA))
        first, count = rec_range
        if recorder:
            b.loads_start(recorder[0], recorder[1], first, count)
            if friction:
                b.friction_start(recorder[0], recorder[1], first, count)
            for n in calls:
                step(n)
            return (b.friction_history() if friction else None), sg.download_all(sfl, b), (b.friction_info() if friction else None), b.loads_history()
        samples, done = [], 0
        for _ in range(sum(calls)):
            step(1)
            done += 1
            if done % 2 == 0:
                samples.append(b.friction(first, count))
        return np.stack(samples), sg.download_all(sfl, b), None, None


@functools.lru_cache(maxsize=None)
def loop_of(sfl, dim_x, dim_y, each):
    """Six steps one by one with friction() after steps 2, 4 and 6, and the loads samples of the same run with the loads
    recorder alone: computed once, shared, never written."""
    labels = labels_of("each", 3, 3, dim_x, dim_y)
    samples, fields, _, _ = batch_run(sfl, dim_x, dim_y, [6], None, each, labels, 3)
    loads_alone = batch_run(sfl, dim_x, dim_y, [6], (2, 3), each, labels, 3, friction=False)[3]
    samples.setflags(write=False)
    loads_alone.setflags(write=False)
    return labels, samples, fields, loads_alone


@pytest.mark.parametrize("calls", [[6], [3, 3]], ids=["one call", "3 + 3"])
@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
def test_a_batchs_recorder_is_the_loop_of_step_and_friction(sfl, each, calls):
    dim_x, dim_y = 61, 81
    labels, want, want_fields, loads_alone = loop_of(sfl, dim_x, dim_y, each)
    got, fields, info, loads = batch_run(sfl, dim_x, dim_y, calls, (2, 3), each, labels, 3)
    assert info == (3, 3, 6, 3) and got.shape == (3, 3, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6")
    assert want["faces"].any() and len({s.tobytes() for s in want}) == 3, "the three samples differ"
    sg.assert_fields_equal(fields, want_fields, "the fields after the call are those of a run without a recorder")
    assert loads.tobytes() == loads_alone.tobytes(), "the loads samples are the same bytes with the friction recorder on and off"


def test_a_batchs_recorder_of_a_range_of_members(sfl):
    dim_x, dim_y = 33, 18
    labels = labels_of("shared", 16, 3, dim_x, dim_y)
    want, want_fields, _, _ = batch_run(sfl, dim_x, dim_y, [6], None, False, labels, 16, (1, 2))
    got, fields, info, _ = batch_run(sfl, dim_x, dim_y, [4, 2], (2, 5), False, labels, 16, (1, 2))
    assert info == (3, 5, 6, 16) and got.shape == (3, 2, 16)
    assert_records_equal(got, want, "members 1 and 2")
    sg.assert_fields_equal(fields, want_fields, "fields")


def context_run(sfl, dim_x, dim_y, solid, labels, bodies, calls, recorder, friction=True):
    """A context run through `calls` with a history, a loads recorder and (friction True) the friction recorder on, or -- no
    recorder -- the loop `step; friction()`.  Returns (friction samples, fields, friction_info, loads samples, history)."""
    cap = sfl.capi
    with sfl.Solver(dim_x, dim_y) as c:
        v, col = random_fields(dim_x, dim_y, 301, vamp=40.0)[:2]
        c.upload(cap.FIELD_VELOCITY, v)
        c.upload(cap.FIELD_COLOR, col)
        c.set_solids(solid)
        c.set_bodies(labels, bodies)
        c.queue_forces([(dim_x // 2, 1)], [(25.0, -10.0)])
        c.queue_forces([(2, dim_y // 2)], [(-15.0, 5.0)], 3)
        fields = lambda: tuple(c.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
        if recorder:
            if friction:
                c.friction_start(*recorder)
            c.loads_start(*recorder)
            c.history_start(1, 8)
            for n in calls:
                c.step_n(n, DT, DX, ITERS, OMEGA)
            return (c.friction_history() if friction else None), fields(), (c.friction_info() if friction else None), c.loads_history(), c.history()
        samples = []
        for k in range(1, sum(calls) + 1):
            c.step(DT, DX, ITERS, OMEGA)
            if k % 2 == 0:
                samples.append(c.friction())
        return np.stack(samples), fields(), None, None, None


@functools.lru_cache(maxsize=None)
def context_loop_of(sfl, dim_x, dim_y):
    solid = sg.mask_of("disc", dim_x, dim_y)
    labels = labels_of("shared", 3, 1, dim_x, dim_y)
    want, want_fields, _, _, _ = context_run(sfl, dim_x, dim_y, solid, labels, 3, [6], None)
    _, _, _, loads_alone, history_alone = context_run(sfl, dim_x, dim_y, solid, labels, 3, [6], (2, 3), friction=False)
    for a in (want, loads_alone, history_alone):
        a.setflags(write=False)
    return solid, labels, want, want_fields, loads_alone, history_alone


@pytest.mark.parametrize("calls", [[6], [3, 3]], ids=["one call", "3 + 3"])
def test_a_contexts_recorder_is_the_loop_of_step_and_friction_with_loads_and_a_history_beside_it(sfl, calls):
    dim_x, dim_y = 33, 18
    solid, labels, want, want_fields, loads_alone, history_alone = context_loop_of(sfl, dim_x, dim_y)
    got, fields, info, loads, hist = context_run(sfl, dim_x, dim_y, solid, labels, 3, calls, (2, 3))
    assert info == (3, 3, 6, 3) and got.shape == (3, 1, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6")
    assert want["faces"].any() and len({s.tobytes() for s in want}) == 3
    sg.assert_fields_equal(fields, want_fields, "the fields after the call are those of a run without a recorder")
    assert len(hist) == 6 and list(hist["step"]) == [1, 2, 3, 4, 5, 6]
    assert loads.tobytes() == loads_alone.tobytes(), "the loads samples are the same bytes with the friction recorder on and off"
    assert hist.tobytes() == history_alone.tobytes(), "... and so are the history's records"


def test_a_recorder_without_room_refuses_the_call_and_leaves_steps_and_fields_untouched(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    with stepped_batch(sfl, dim_x, dim_y, masks, steps=1) as b:
        before = sg.download_all(sfl, b)
        b.friction_start(2, 2)
        for call in (lambda: b.step_n(6, DT, DX, ITERS, OMEGA), lambda: b.step_n_each(6, DT, DX, ITERS, OMEGA)):
            with pytest.raises(sfl.SflError, match="friction recorder has room for 2 more samples") as e:
                call()
            assert e.value.code == sfl.capi.ERR_STATE
        assert b.friction_info() == (0, 2, 0, 1)
        sg.assert_fields_equal(sg.download_all(sfl, b), before, "a refused call")
        with pytest.raises(sfl.SflError, match="the friction recorder is on") as e:
            b.set_bodies(labels_of("shared", 3, 3, dim_x, dim_y), 3)
        assert e.value.code == sfl.capi.ERR_STATE and b.bodies_info() == (1, False, False)
        b.step_n(4, DT, DX, ITERS, OMEGA)
        assert b.friction_info() == (2, 2, 4, 1)
        b.step_n(1, DT, DX, ITERS, OMEGA)   # completes no sample: let through
        with pytest.raises(sfl.SflError, match="room for 0 more samples"):
            b.step_n(1, DT, DX, ITERS, OMEGA)
        kept = b.friction_history()
        b.friction_start(2, 2)   # a restart: the count is 0 again
        assert b.friction_info() == (0, 2, 0, 1)
        b.friction_stop()
        assert b.friction_info() == (0, 0, 0, 1) and kept.shape == (2, 3, 1)
    with sfl.Solver(dim_x, dim_y) as c:
        c.set_solids(masks[1])
        c.step(DT, DX, ITERS, OMEGA)
        v = c.download(sfl.capi.FIELD_VELOCITY)
        c.friction_start(1, 2)
        with pytest.raises(sfl.SflError, match="friction recorder has room for 2 more samples") as e:
            c.step_n(3, DT, DX, ITERS, OMEGA)
        assert e.value.code == sfl.capi.ERR_STATE and c.friction_info() == (0, 2, 0, 1)
        assert_bit_equal(c.download(sfl.capi.FIELD_VELOCITY), v, "a refused call")


def test_a_sample_without_solids_is_zeros_and_the_replay_of_a_timeline_is_not_cut(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    forces = sg.forces_of(dim_x, dim_y, masks)

    def run(recorder):
        with sg.make(sfl, dim_x, dim_y, batch=3) as b:
            for step, records in forces.items():
                sg.queue(b, records, step)
            if recorder:
                b.friction_start(1, 4)
            b.step_n(4, DT, DX, ITERS, OMEGA)
            return sg.download_all(sfl, b), (b.friction_history() if recorder else None)

    plain, _ = run(False)
    fields, samples = run(True)
    assert samples.shape == (4, 3, 1) and samples.tobytes() == bytes(4 * 3 * 48)
    sg.assert_fields_equal(fields, plain, "fields")


def test_a_contexts_recorder_counts_inside_the_seam_loop_where_its_samples_are_zeros(sfl):
    """Without solids sfl_step_n keeps its step seams while a friction recorder is on (130 x 70 on the tiled kernels: every
    condition of the seam holds) and counts each step inside that loop, across calls that leave a remainder: the samples are
    zero records and the fields those of a run without a recorder."""
    cap, dim_x, dim_y = sfl.capi, 130, 70

    def run(recorder):
        with sfl.Solver(dim_x, dim_y) as c:
            v, col = random_fields(dim_x, dim_y, 303, vamp=40.0)[:2]
            c.upload(cap.FIELD_VELOCITY, v)
            c.upload(cap.FIELD_COLOR, col)
            c.set_option(cap.OPT_ADVECT_KERNEL, 2)
            if recorder:
                c.friction_start(2, 4)
            for n in (3, 3):
                c.step_n(n, DT, DX, ITERS, OMEGA)
            fields = tuple(c.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
            return fields, (c.friction_info(), c.friction_history()) if recorder else None

    plain, _ = run(False)
    fields, (info, samples) = run(True)
    assert info == (3, 4, 6, 1), info
    assert samples.shape == (3, 1, 1) and samples.tobytes() == bytes(3 * 48)
    sg.assert_fields_equal(fields, plain, "the fields are those of a run without a recorder")


# ---- with viscosity set: the binding of friction_xy ------------------------------------------------------------------------
def test_friction_xy_takes_the_viscosity_that_is_set_per_member(sfl):
    """This checks the binding, not the physics: nu = None is the viscosity held, member by member."""
    dim_x, dim_y, batch = 61, 81, 4
    disc = sg.mask_of("disc", dim_x, dim_y)
    nus = np.array([0.0, 1e-3, 0.05, 2.0], F)
    with sg.make(sfl, dim_x, dim_y, disc, batch=batch) as b:
        assert (b.friction_xy() == 0).all(), "no viscosity set: zeros"
        b.set_viscosity(nus, 2)
        b.queue_forces([0, 1, 2, 3], [(3, dim_y // 2)] * 4, [(30.0, 4.0)] * 4)
        b.friction_start(1, 2, 1, 3)
        b.step_n(2, DT, DX, ITERS, OMEGA)
        held = b.viscosity()[0]
        assert held.tobytes() == nus.tobytes()
        rec = b.friction()
        assert rec["faces"].all() and (rec["fx"] != 0).any()
        raw = rule.friction_xy(rec, 1.0)
        want = held.astype(np.float64)[:, None, None] * raw
        assert b.friction_xy().tobytes() == want.tobytes() and (b.friction_xy()[0] == 0).all() and (b.friction_xy()[1:] != 0).any()
        assert b.friction_xy(nu=0.5).tobytes() == (0.5 * raw).tobytes()
        assert b.friction_xy(nu=[1.0, 2.0], first=2, count=2).tobytes() == (np.array([1.0, 2.0])[:, None, None] * raw[2:]).tobytes()
        hist = b.friction_history()
        assert hist.shape == (2, 3, 1) and hist[1].tobytes() == rec[1:].tobytes()
        assert b.friction_history_xy().tobytes() == (held.astype(np.float64)[1:, None, None] * rule.friction_xy(hist, 1.0)).tobytes()
    with sfl.Solver(dim_x, dim_y) as c:
        v = random_fields(dim_x, dim_y, 304, vamp=40.0)[0]
        c.upload(sfl.capi.FIELD_VELOCITY, v)
        c.set_solids(disc)
        assert (c.friction_xy() == 0).all() and (c.friction_xy(nu=1.0) != 0).any()
        c.set_viscosity(0.125, 2)
        assert c.friction_xy().tobytes() == (0.125 * rule.friction_xy(c.friction(), 1.0)).tobytes()
