"""Loads on the GPU (include/sfl.h "LOADS"; csrc/loads.hip): the samplers of a batch and of a whole-domain context against
tests/load_rule.py -- the header's rule in numpy, whose own sanity tests/test_loads.py checks.  Every comparison is bit for
bit, on the bytes of the 48-byte records.

Shapes and masks are those of tests/test_solids_gpu.py: 2 x 2 with all 16 masks as one batch of 16; 7 x 5, 33 x 18 (an odd
width), 61 x 81 and 96 x 64 (the 6144-cell limit) as batches of three members with a DIFFERENT mask each, one of them empty
and never in the same place.  Labels: none, shared, and per member with seeded 0..bodies, for bodies in {1, 3, 16}.
Pressures: what three steps with forces left; seeded magnitudes over 1e-44..1e37 with both signs and -0.0f; NaN and +-Inf on
some wet faces together with NaN in cells that are not wet and in solid cells, which must have no effect.  Contexts: 33 x 18,
96 x 64, 131 x 70 (a width that is no multiple of 16: groups that straddle rows, a partial last group) and 515 x 260 (several
workgroups; a disc plus channel walls labelled 0)."""
import functools

import numpy as np
import pytest

import load_rule as rule
import test_solids_gpu as sg
from conftest import assert_bit_equal, random_fields

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = sg.DT, sg.DX, sg.ITERS, sg.OMEGA
F = np.float32
LABELLINGS = [("none", 1)] + [(mode, bodies) for mode in ("shared", "each") for bodies in (1, 3, 16)]


# ---- inputs ----------------------------------------------------------------------------------------------------------------
def labels_of(mode, bodies, batch, dim_x, dim_y, seed=11):
    """None, uint8[dim_y, dim_x] or uint8[batch, dim_y, dim_x] with seeded labels 0..bodies on EVERY cell (a label counts only
    where the cell is solid)."""
    if mode == "none":
        return None
    shape = (dim_y, dim_x) if mode == "shared" else (batch, dim_y, dim_x)
    return np.random.default_rng(seed + bodies).integers(0, bodies + 1, shape, dtype=np.uint8)


def wide_pressure(shape, seed):
    """Magnitudes 10^-44 .. 10^37 (denormals included), both signs, every tenth value -0.0f."""
    rng = np.random.default_rng(seed)
    with np.errstate(under="ignore"):
        p = (10.0 ** rng.uniform(-44, 37, shape) * rng.choice([-1.0, 1.0], shape)).astype(F)
    p[rng.random(shape) < 0.1] = F(-0.0)
    return p


def nonfinite_pressure(masks, seed):
    """Seeded values; NaN, +Inf and -Inf on a third of the fluid cells that touch a solid one; NaN in a tenth of all the other
    fluid cells that touch none (not wet: no effect -- unless a rim-less neighbour makes them wet, which the rule decides) and
    in every other solid cell (no effect)."""
    rng = np.random.default_rng(seed)
    p = rng.standard_normal(masks.shape).astype(F) * F(37.5)
    for m, solid in enumerate(masks):
        faces = rule.wet_faces(solid)
        wet = np.zeros(solid.shape, bool)
        for j, i, _ in faces:
            wet[j, i] = True
        pick = wet & (rng.random(solid.shape) < 1 / 3)
        p[m][pick] = rng.choice(np.array([np.nan, np.inf, -np.inf], F), int(pick.sum()))
        p[m][~wet & ~solid & (rng.random(solid.shape) < 0.1)] = np.nan
        p[m][solid & (rng.random(solid.shape) < 0.5)] = np.nan
    return p


def want_of(p, masks, labels, bodies):
    """The rule's records of every member: DTYPE[batch, bodies].  masks / labels: per member, or one for all (2-D)."""
    out = np.zeros((len(p), bodies), rule.DTYPE)
    for m in range(len(p)):
        solid = masks if masks.ndim == 2 else masks[m]
        lab = None if labels is None else labels if labels.ndim == 2 else labels[m]
        out[m] = rule.loads(p[m], solid, lab, bodies)
    return out


def assert_records_equal(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() == want.tobytes():
        return
    for idx in np.ndindex(got.shape):
        for name in got.dtype.names:
            g, w = np.atleast_1d(got[idx][name]), np.atleast_1d(want[idx][name])
            assert g.tobytes() == w.tobytes(), f"{what}: record {idx} {name}: got {g}, want {w}"


def stepped_batch(sfl, dim_x, dim_y, masks, steps=3):
    """A batch with the shape's fields and masks after `steps` steps with the forces of test_solids_gpu."""
    b = sg.make(sfl, dim_x, dim_y, masks)
    for step, records in sg.forces_of(dim_x, dim_y, masks).items():
        sg.queue(b, records, step)
    b.step_n(steps, DT, DX, ITERS, OMEGA)
    return b


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2)] + sg.SHAPES, ids=["2x2"] + sg.IDS)
def test_a_batchs_loads_are_the_rules(sfl, dim_x, dim_y):
    cap = sfl.capi
    masks = sg.masks_of(dim_x, dim_y)
    batch = len(masks)
    with stepped_batch(sfl, dim_x, dim_y, masks) as b:
        assert b.bodies_info() == (1, False, False) and (b.bodies() == 1).all()
        pressures = {"three steps with forces": b.download(cap.FIELD_PRESSURE), "1e-44..1e37": wide_pressure(masks.shape, 5),
                     "nonfinite": nonfinite_pressure(masks, 6)}
        some_face = False
        for name, p in pressures.items():
            b.upload(cap.FIELD_PRESSURE, p)
            for mode, bodies in LABELLINGS:
                labels = labels_of(mode, bodies, batch, dim_x, dim_y)
                b.set_bodies(labels, bodies)
                assert b.bodies_info() == (bodies, mode != "none", mode == "each")
                want = want_of(p, masks, labels, bodies)
                some_face |= bool(want["faces"].any())
                assert_records_equal(b.loads(), want, f"{dim_x}x{dim_y} {name}, labels {mode}, {bodies} bodies")
            assert_bit_equal(b.download(cap.FIELD_PRESSURE), p, "the pressure held")
        assert some_face
        nf = want_of(pressures["nonfinite"], masks, None, 1)
        assert dim_x * dim_y <= 35 or nf["nonfinite"].any(), "the nonfinite case has nonfinite faces"


def test_masks_and_labels_are_shared_or_per_member_independently_and_in_either_order(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    shared_mask = sg.mask_of("disc", dim_x, dim_y)
    p = wide_pressure(masks.shape, 8)
    each, shared = labels_of("each", 3, 3, dim_x, dim_y), labels_of("shared", 3, 3, dim_x, dim_y)
    with sfl.BatchSolver(dim_x, dim_y, 3) as b:
        b.upload(sfl.capi.FIELD_PRESSURE, p)
        b.set_bodies(each, 3)   # the labels first: no solids yet, zero records
        assert b.loads().tobytes() == bytes(3 * 3 * 48)
        b.set_solids(shared_mask)
        assert_records_equal(b.loads(), want_of(p, shared_mask, each, 3), "mask shared, labels per member")
        assert np.array_equal(b.bodies(), each), "the labels come back"
        b.set_bodies(shared, 3)
        b.set_solids(masks)
        assert_records_equal(b.loads(), want_of(p, masks, shared, 3), "masks per member, labels shared")
        assert np.array_equal(b.bodies(1, 2), np.stack([shared, shared])), "shared labels repeated"
        b.set_solids(None)
        assert b.loads().tobytes() == bytes(3 * 3 * 48), "solids cleared: zero records"
        b.set_solids(masks)
        b.set_bodies(None)
        assert_records_equal(b.loads(), want_of(p, masks, None, 1), "labels cleared: every solid cell is body 1")


def test_range_arguments_at_both_ends_of_the_batch_and_a_large_batch(sfl):
    dim_x, dim_y = 7, 5
    masks = sg.masks_of(dim_x, dim_y)
    p = wide_pressure(masks.shape, 9)
    labels = labels_of("each", 3, 3, dim_x, dim_y)
    want = want_of(p, masks, labels, 3)
    with sfl.BatchSolver(dim_x, dim_y, 3) as b:
        b.upload(sfl.capi.FIELD_PRESSURE, p)
        b.set_solids(masks)
        b.set_bodies(labels, 3)
        for first, count in ((0, 1), (0, 2), (1, 1), (1, 2), (2, 1), (0, 3)):
            assert_records_equal(b.loads(first, count), want[first:first + count], f"members [{first}, {first} + {count})")
        assert b.loads(3, 0).shape == (0, 3) and b.loads(0, 0).shape == (0, 3)
        for first, count in ((3, 1), (-1, 1), (2, 2)):
            with pytest.raises(sfl.SflError, match="not inside the batch") as e:
                b.loads(first, count)
            assert e.value.code == sfl.capi.ERR_INVALID
    with sfl.BatchSolver(128, 128, 2, large=True) as big:   # no solids there: zero records, and a recorder of zeros
        assert big.loads().tobytes() == bytes(2 * 48)
        big.loads_start(1, 2)
        big.step_n(2, DT, DX, 2, OMEGA)
        assert big.loads_info() == (2, 2, 2, 1) and big.loads_history().tobytes() == bytes(2 * 2 * 48)


def test_loads_changes_no_field_and_two_runs_give_identical_bytes(sfl):
    dim_x, dim_y = 61, 81
    masks = sg.masks_of(dim_x, dim_y)
    labels = labels_of("each", 16, 3, dim_x, dim_y)
    with stepped_batch(sfl, dim_x, dim_y, masks) as b, stepped_batch(sfl, dim_x, dim_y, masks) as twin:
        b.set_bodies(labels, 16)
        twin.set_bodies(labels, 16)
        counts = ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ")
        before = b.distance(twin)
        first = b.loads()
        after = b.distance(twin)
        for d in (before, after):
            assert all((d[c] == 0).all() for c in counts), d
        assert first["faces"].any()
        assert b.loads().tobytes() == first.tobytes() == twin.loads().tobytes()
        assert_records_equal(first, want_of(b.download(sfl.capi.FIELD_PRESSURE), masks, labels, 16), "the stepped batch")


# ---- contexts --------------------------------------------------------------------------------------------------------------
def channel_with_disc(dim_x, dim_y):
    """Channel walls two cells thick at j = 0 and at the top, labelled 0, and a disc, body 1, a smaller one, body 2."""
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    disc = (i - dim_x // 3) ** 2 + (j - dim_y // 2) ** 2 <= (dim_y // 5) ** 2
    small = (i - (2 * dim_x) // 3) ** 2 + (j - dim_y // 3) ** 2 <= (dim_y // 9) ** 2
    solid = disc | small
    solid[0:2, :] = solid[-2:, :] = True
    labels = np.zeros((dim_y, dim_x), np.uint8)
    labels[disc], labels[small] = 1, 2
    return solid, labels


CONTEXT_CASES = {(33, 18): "plate", (96, 64): "seeded", (131, 70): "seeded", (515, 260): "channel+disc"}


@pytest.mark.parametrize("dim_x,dim_y", list(CONTEXT_CASES), ids=[f"{x}x{y}" for x, y in CONTEXT_CASES])
def test_a_contexts_loads_are_the_rules_and_a_batch_members(sfl, dim_x, dim_y):
    cap = sfl.capi
    kind = CONTEXT_CASES[(dim_x, dim_y)]
    if kind == "channel+disc":
        solid, walls = channel_with_disc(dim_x, dim_y)
        labellings = [(None, 1), (walls, 2), (walls, 16)]
    else:
        solid = sg.mask_of(kind, dim_x, dim_y)
        labellings = [(None, 1)] + [(labels_of("shared", bodies, 1, dim_x, dim_y), bodies) for bodies in (1, 3, 16)]
    fits_a_batch = dim_x * dim_y <= 6144
    with sfl.Solver(dim_x, dim_y) as c:
        v, col = random_fields(dim_x, dim_y, 300, vamp=40.0)[:2]
        c.upload(cap.FIELD_VELOCITY, v)
        c.upload(cap.FIELD_COLOR, col)
        assert c.loads().tobytes() == bytes(48), "no solids: zero records"
        c.set_solids(solid)
        c.queue_forces([(dim_x // 2, 1)], [(25.0, -10.0)])
        c.step_n(3, DT, DX, ITERS, OMEGA)
        pressures = {"three steps": c.download(cap.FIELD_PRESSURE), "1e-44..1e37": wide_pressure((1, dim_y, dim_x), 15)[0],
                     "nonfinite": nonfinite_pressure(solid[None], 16)[0]}
        batch = sfl.BatchSolver(dim_x, dim_y, 1) if fits_a_batch else None
        if batch:
            batch.set_solids(solid)
        for name, p in pressures.items():
            c.upload(cap.FIELD_PRESSURE, p)
            if batch:
                batch.upload(cap.FIELD_PRESSURE, p[None])
            for labels, bodies in labellings:
                c.set_bodies(labels, bodies)
                assert c.bodies_info() == (bodies, labels is not None)
                want = want_of(p[None], solid, labels, bodies)
                got = c.loads()
                assert_records_equal(got, want, f"{dim_x}x{dim_y} {name}, {bodies} bodies")
                if batch:
                    batch.set_bodies(labels, bodies)
                    assert batch.loads().tobytes() == got.tobytes(), "a batch member of the same shape, mask, labels and pressure"
            assert_bit_equal(c.download(cap.FIELD_PRESSURE), p, "the pressure held")
        if batch:
            batch.close()
        if kind == "channel+disc":
            assert want[0, 0]["faces"].all() and want[0, 1]["faces"].all() and not want[0, 2:]["faces"].any()
            everything = rule.loads(p, solid)[0]
            assert everything["faces"].sum() > want["faces"].sum(), "the walls labelled 0 are in no body"
        assert c.loads().tobytes() == c.loads().tobytes()


def test_a_contexts_loads_changes_no_field(sfl):
    """Two contexts stepped alike: every count of `distance` is zero before loads() and after it."""
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
    counts = ("velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ")
    before = c.distance(twin)
    rec = c.loads()
    after = c.distance(twin)
    assert rec["faces"].any() and rec.tobytes() == twin.loads().tobytes()
    for d in (before, after):
        assert all(d[k] == 0 for k in counts), d
    c.close()
    twin.close()


# ---- the recorder ----------------------------------------------------------------------------------------------------------
def batch_run(sfl, dim_x, dim_y, calls, recorder, each=False, labels=None, bodies=1, rec_range=(0, None)):
    """A stepped batch run through `calls` (steps per step call) -- with the recorder (every, capacity), or with the loop
    `step; loads()` it replaces.  Returns (samples [n, count, bodies], fields, loads_info or None)."""
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
            for n in calls:
                step(n)
            return b.loads_history(), sg.download_all(sfl, b), b.loads_info()
        samples, done = [], 0
        for _ in range(sum(calls)):
            step(1)
            done += 1
            if done % 2 == 0:
                samples.append(b.loads(first, count))
        return np.stack(samples), sg.download_all(sfl, b), None


@functools.lru_cache(maxsize=None)
def loop_of(sfl, dim_x, dim_y, each):
    """Six steps one by one with loads() after steps 2, 4 and 6: computed once, shared, never written."""
    labels = labels_of("each", 3, 3, dim_x, dim_y)
    samples, fields, _ = batch_run(sfl, dim_x, dim_y, [6], None, each, labels, 3)
    samples.setflags(write=False)
    return labels, samples, fields


@pytest.mark.parametrize("calls", [[6], [3, 3]], ids=["one call", "3 + 3"])
@pytest.mark.parametrize("each", [False, True], ids=["step_n", "step_n_each"])
def test_a_batchs_recorder_is_the_loop_of_step_and_loads(sfl, each, calls):
    dim_x, dim_y = 61, 81
    labels, want, want_fields = loop_of(sfl, dim_x, dim_y, each)
    got, fields, info = batch_run(sfl, dim_x, dim_y, calls, (2, 3), each, labels, 3)
    assert info == (3, 3, 6, 3) and got.shape == (3, 3, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6")
    assert want["faces"].any() and len({s.tobytes() for s in want}) == 3, "the three samples differ"
    sg.assert_fields_equal(fields, want_fields, "the fields after the call are those of a run without a recorder")


def test_a_batchs_recorder_of_a_range_of_members(sfl):
    dim_x, dim_y = 33, 18
    labels = labels_of("shared", 16, 3, dim_x, dim_y)
    want, want_fields, _ = batch_run(sfl, dim_x, dim_y, [6], None, False, labels, 16, (1, 2))
    got, fields, info = batch_run(sfl, dim_x, dim_y, [4, 2], (2, 5), False, labels, 16, (1, 2))
    assert info == (3, 5, 6, 16) and got.shape == (3, 2, 16)
    assert_records_equal(got, want, "members 1 and 2")
    sg.assert_fields_equal(fields, want_fields, "fields")


def context_run(sfl, dim_x, dim_y, solid, labels, bodies, calls, recorder, history=False):
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
            c.loads_start(*recorder)
            if history:
                c.history_start(1, 8)
            for n in calls:
                c.step_n(n, DT, DX, ITERS, OMEGA)
            return c.loads_history(), fields(), c.loads_info(), (c.history() if history else None)
        samples = []
        for k in range(1, sum(calls) + 1):
            c.step(DT, DX, ITERS, OMEGA)
            if k % 2 == 0:
                samples.append(c.loads())
        return np.stack(samples), fields(), None, None


@pytest.mark.parametrize("calls,history", [([6], False), ([3, 3], False), ([6], True)], ids=["one call", "3 + 3", "a history beside it"])
def test_a_contexts_recorder_is_the_loop_of_step_and_loads(sfl, calls, history):
    dim_x, dim_y = 33, 18
    solid = sg.mask_of("disc", dim_x, dim_y)
    labels = labels_of("shared", 3, 1, dim_x, dim_y)
    want, want_fields, _, _ = context_run(sfl, dim_x, dim_y, solid, labels, 3, [6], None)
    got, fields, info, hist = context_run(sfl, dim_x, dim_y, solid, labels, 3, calls, (2, 3), history)
    assert info == (3, 3, 6, 3) and got.shape == (3, 1, 3)
    assert_records_equal(got, want, "samples of steps 2, 4, 6")
    assert want["faces"].any() and len({s.tobytes() for s in want}) == 3
    sg.assert_fields_equal(fields, want_fields, "the fields after the call are those of a run without a recorder")
    if history:
        assert len(hist) == 6 and list(hist["step"]) == [1, 2, 3, 4, 5, 6]


def test_a_recorder_without_room_refuses_the_call_and_leaves_steps_and_fields_untouched(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    with stepped_batch(sfl, dim_x, dim_y, masks, steps=1) as b:
        before = sg.download_all(sfl, b)
        b.loads_start(2, 2)
        for call in (lambda: b.step_n(6, DT, DX, ITERS, OMEGA), lambda: b.step_n_each(6, DT, DX, ITERS, OMEGA)):
            with pytest.raises(sfl.SflError, match="loads recorder has room for 2 more samples") as e:
                call()
            assert e.value.code == sfl.capi.ERR_STATE
        assert b.loads_info() == (0, 2, 0, 1)
        sg.assert_fields_equal(sg.download_all(sfl, b), before, "a refused call")
        with pytest.raises(sfl.SflError, match="recorder is on") as e:
            b.set_bodies(labels_of("shared", 3, 3, dim_x, dim_y), 3)
        assert e.value.code == sfl.capi.ERR_STATE and b.bodies_info() == (1, False, False)
        b.step_n(4, DT, DX, ITERS, OMEGA)
        assert b.loads_info() == (2, 2, 4, 1)
        b.step_n(1, DT, DX, ITERS, OMEGA)   # completes no sample: let through
        with pytest.raises(sfl.SflError, match="room for 0 more samples"):
            b.step_n(1, DT, DX, ITERS, OMEGA)
        kept = b.loads_history()
        b.loads_start(2, 2)   # a restart: the count is 0 again
        assert b.loads_info() == (0, 2, 0, 1)
        b.loads_stop()
        assert b.loads_info() == (0, 0, 0, 1) and kept.shape == (2, 3, 1)
    with sfl.Solver(dim_x, dim_y) as c:
        c.set_solids(masks[1])
        c.step(DT, DX, ITERS, OMEGA)
        p = c.download(sfl.capi.FIELD_PRESSURE)
        c.loads_start(1, 2)
        with pytest.raises(sfl.SflError, match="loads recorder has room for 2 more samples") as e:
            c.step_n(3, DT, DX, ITERS, OMEGA)
        assert e.value.code == sfl.capi.ERR_STATE and c.loads_info() == (0, 2, 0, 1)
        assert_bit_equal(c.download(sfl.capi.FIELD_PRESSURE), p, "a refused call")


def test_a_sample_without_solids_is_zeros_and_the_replay_of_a_timeline_is_not_cut(sfl):
    dim_x, dim_y = 33, 18
    masks = sg.masks_of(dim_x, dim_y)
    forces = sg.forces_of(dim_x, dim_y, masks)

    def run(recorder):
        with sg.make(sfl, dim_x, dim_y, batch=3) as b:
            for step, records in forces.items():
                sg.queue(b, records, step)
            if recorder:
                b.loads_start(1, 4)
            b.step_n(4, DT, DX, ITERS, OMEGA)
            return sg.download_all(sfl, b), (b.loads_history() if recorder else None)

    plain, _ = run(False)
    fields, samples = run(True)
    assert samples.shape == (4, 3, 1) and samples.tobytes() == bytes(4 * 3 * 48)
    sg.assert_fields_equal(fields, plain, "fields")


def test_a_contexts_recorder_counts_inside_the_seam_loop_where_its_samples_are_zeros(sfl):
    """Without solids sfl_step_n keeps its step seams while a loads recorder is on (130 x 70 on the tiled kernels: every
    condition of the seam holds) and counts each step inside that loop, across calls that leave a remainder: the samples are
    zero records and the fields those of a run without a recorder.  (The seeded call sequences found that nothing else stood
    on this count: a loop that skipped it passed every other test of this file.)"""
    cap, dim_x, dim_y = sfl.capi, 130, 70

    def run(recorder):
        with sfl.Solver(dim_x, dim_y) as c:
            v, col = random_fields(dim_x, dim_y, 303, vamp=40.0)[:2]
            c.upload(cap.FIELD_VELOCITY, v)
            c.upload(cap.FIELD_COLOR, col)
            c.set_option(cap.OPT_ADVECT_KERNEL, 2)
            if recorder:
                c.loads_start(2, 4)
            for n in (3, 3):
                c.step_n(n, DT, DX, ITERS, OMEGA)
            fields = tuple(c.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))
            return fields, (c.loads_info(), c.loads_history()) if recorder else None

    plain, _ = run(False)
    fields, (info, samples) = run(True)
    assert info == (3, 4, 6, 1), info
    assert samples.shape == (3, 1, 1) and samples.tobytes() == bytes(3 * 48)
    sg.assert_fields_equal(fields, plain, "the fields are those of a run without a recorder")
