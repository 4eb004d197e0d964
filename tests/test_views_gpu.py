"""Views on the GPU (include/sfl.h "VIEWS"; csrc/field_view.hip): the four scalars, their node colours and their images, of
batches of both kinds and of a context, against tests/view_rule.py -- the header's rules in numpy float32, itself checked
against the oracle by tests/test_views.py -- applied to the fields the object holds, and against the definition: a view
image is the dye's render of a member whose dye is the view's node colours (the oracle's render_rgb565 of the rule's texels,
and render_members of a twin batch that was given them as dye).

The shapes are the smallest at which the kernels can go wrong: 2 x 2 (one block, every node on two walls), 3 x 2 and 5 x 4,
17 x 33 (exactly one full 16 x 32 tile), 18 x 34 (one block over on both axes: edge tiles of one block, the ring across a
tile seam), 61 x 81 (the sketch's grid), 96 x 96 as a large batch, and a 130 x 70 context.  Planted in the fields: a NaN, +inf,
-inf, a denormal velocity pair, and values on the two sides of lo and hi.

Scalars are compared bit for bit where they are numbers.  Where they are NaNs both sides must have one, but its sign and
payload are not compared: the header defines none, and the default NaN of inf - inf differs between the host's FPU (sign
set) and the GPU's (sign clear) before any rule is applied.  Texels and images have no such freedom: a NaN is nan_colour."""
import functools

import numpy as np
import pytest

import view_rule as rule
from conftest import assert_bit_equal
from test_batch import DT, OMEGA, download_all, member_fields, upload_members

M = rule.MAX_COLOUR
NAN_COLOUR = (0x12345678, M, 0)
BATCH = 4
SHAPES = [(2, 2, False), (3, 2, False), (5, 4, False), (17, 33, False), (18, 34, False), (61, 81, False), (96, 96, True)]
IDS = [f"{x}x{y}{'L' if large else ''}" for x, y, large in SHAPES]
# what -> (lo, hi): inside the spread of member_fields' values, so that both clamps and the range between them occur
RANGE = {rule.SPEED: (10.0, 100.0), rule.VORTICITY: (-60.0, 60.0), rule.PRESSURE: (-1.0, 1.5), rule.DIVERGENCE: (-50.0, 50.0)}
RNG = np.random.default_rng(99)
PALETTES = {2: np.array([[0, M, 5], [M, 0, M]], np.uint32), 3: np.array([[0, 0, M], [M, M, M], [M, 0, 0]], np.uint32),
            256: RNG.integers(0, M + 1, (256, 3), dtype=np.uint32)}


def _plant(v, p, member):
    """The special values, in place.  A member of fewer than 12 nodes takes only the kinds k = member (mod BATCH), so that a
    NaN does not reach every node of every member; the j-th value a member takes goes to node 7 j + 3 member of the
    flattened field (distinct nodes at every shape of SHAPES)."""
    cells = p.size
    lo, hi = np.float32(RANGE[rule.PRESSURE][0]), np.float32(RANGE[rule.PRESSURE][1])
    slo, shi = np.float32(RANGE[rule.SPEED][0]), np.float32(RANGE[rule.SPEED][1])
    down, up = np.float32(-np.inf), np.float32(np.inf)
    kinds = [((np.nan, 1.0), np.nan), ((np.inf, -2.0), np.inf), ((3.0, -np.inf), -np.inf), ((1e-41, -3e-42), 1e-40),
             ((np.nextafter(slo, down), 0.0), np.nextafter(lo, down)), ((slo, 0.0), lo), ((0.0, np.nextafter(slo, up)), np.nextafter(lo, up)),
             ((np.nextafter(shi, down), 0.0), np.nextafter(hi, down)), ((0.0, shi), hi), ((np.nextafter(shi, up), -0.0), np.nextafter(hi, up))]
    vf, pf = v.reshape(-1, 2), p.reshape(-1)
    mine = [kind for k, kind in enumerate(kinds) if cells >= 12 or k % BATCH == member]
    nodes = [(7 * j + 3 * member) % cells for j in range(len(mine))]
    assert len(set(nodes)) == len(nodes)
    for n, (vel, pressure) in zip(nodes, mine):
        vf[n] = vel
        pf[n] = pressure


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y):
    """BATCH members of one shape with the special values planted: (velocity, dye, pressure) each.  Computed once, shared,
    never written."""
    out = []
    for m in range(BATCH):
        v, c, p = member_fields(dim_x, dim_y, 1000 * dim_x + 10 * dim_y + m)
        _plant(v, p, m)
        for a in (v, c, p):
            a.setflags(write=False)
        out.append((v, c, p))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def scalars_of(dim_x, dim_y, what, dx):
    out = np.stack([rule.scalar(what, v, p, dx) for v, _, p in fields_of(dim_x, dim_y)])
    out.setflags(write=False)
    return out


def make_batch(sfl, dim_x, dim_y, large):
    b = sfl.BatchSolver(dim_x, dim_y, BATCH, large=large)
    f = fields_of(dim_x, dim_y)
    b.upload(0, np.stack([x[0] for x in f]))
    b.upload(1, np.stack([x[1] for x in f]))
    b.upload(3, np.stack([x[2] for x in f]))   # the pressure
    return b


def assert_untouched(b, twin, what):
    d = b.distance(twin)
    assert (int(d["velocity_cells_differ"].sum()), int(d["dye_cells_differ"].sum()), int(d["pressure_cells_differ"].sum())) == (0, 0, 0), what


def assert_scalars_equal(got, want, what):
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaNs at {np.argwhere(gn != wn)[:4].tolist()}"
    assert_bit_equal(np.where(gn, np.float32(0), got), np.where(wn, np.float32(0), want), what)


def view_of(sfl, what, stops=3, dx=1.0):
    lo, hi = RANGE[what]
    return sfl.View(what, lo, hi, PALETTES[stops], dx=dx, nan_colour=NAN_COLOUR)


def rule_texels(dim_x, dim_y, view):
    lo, hi = np.float32(view.lo), np.float32(view.hi)
    return rule.texels(scalars_of(dim_x, dim_y, view.what, view.dx), lo, hi, view.palette, view.nan_colour)


# ---- 1. scalars --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,large", SHAPES, ids=IDS)
def test_scalars_are_the_rules_bit_for_bit(sfl, dim_x, dim_y, large):
    with make_batch(sfl, dim_x, dim_y, large) as b, make_batch(sfl, dim_x, dim_y, large) as twin:
        assert_bit_equal(b.download(0), np.stack([f[0] for f in fields_of(dim_x, dim_y)]), "the velocity as uploaded")
        for dx in (1.0, 0.37):
            for what in range(4):
                want = scalars_of(dim_x, dim_y, what, dx)
                for first, count in ((0, BATCH), (1, 3), (2, 1)):
                    got = b.view_scalar(what, dx, first, count)
                    assert got.shape == (count, dim_y, dim_x) and got.dtype == np.float32
                    assert_scalars_equal(got, want[first:first + count], f"{dim_x} x {dim_y}, view {what}, dx {dx}, members [{first}, {first + count})")
        assert np.isnan(scalars_of(dim_x, dim_y, rule.PRESSURE, 1.0)).any() and np.isinf(scalars_of(dim_x, dim_y, rule.SPEED, 1.0)).any()
        assert b.view_scalar(0, 1.0, 2, 0).shape == (0, dim_y, dim_x)
        assert_untouched(b, twin, "view_scalar reads only")


# ---- 2. texels ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,large", SHAPES, ids=IDS)
def test_texels_are_the_rules_bit_for_bit(sfl, dim_x, dim_y, large):
    with make_batch(sfl, dim_x, dim_y, large) as b, make_batch(sfl, dim_x, dim_y, large) as twin:
        for stops in (2, 3, 256):
            for what in range(4):
                view = view_of(sfl, what, stops, dx=0.37 if stops == 3 else 1.0)
                want = rule_texels(dim_x, dim_y, view)
                got = b.view_texels(view, 1, 3)
                assert got.shape == (3, dim_y, dim_x, 3) and got.dtype == np.uint32
                assert_bit_equal(got, want[1:], f"{dim_x} x {dim_y}, view {what}, {stops} stops")
                assert_bit_equal(b.view_texels(view, 0, 1), want[:1], f"{dim_x} x {dim_y}, view {what}, {stops} stops, member 0")
                nan = np.isnan(scalars_of(dim_x, dim_y, what, view.dx))
                assert nan.any() and np.all(want[nan] == np.array(NAN_COLOUR, np.uint32)), "the planted NaNs give nan_colour"
        assert_untouched(b, twin, "view_texels reads only")


# ---- 3. images ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y,large", SHAPES, ids=IDS)
def test_images_are_the_dyes_render_of_the_texels(sfl, oracle, dim_x, dim_y, large):
    """Against the oracle's draw of the rule's texels, and against render_members of a batch whose dye is those texels.  At
    scaling 1 the images of 3 x 2 have 2 pixels, those of 2 x 2 one: members start on 2-byte boundaries.  Every view at
    scaling 4; the other scalings take the four views in turn."""
    with make_batch(sfl, dim_x, dim_y, large) as b, make_batch(sfl, dim_x, dim_y, large) as twin, \
            sfl.BatchSolver(dim_x, dim_y, BATCH, large=large) as dyed:
        k = 0
        for scaling in (1, 3, 4, 64):
            first, count = (1, 3) if scaling < 64 else (3, 1)   # (one image of 61 x 81 at scaling 64 has 2 * 10^7 pixels)
            for what in (range(4) if scaling == 4 else [(k := k + 1) % 4]):
                view = view_of(sfl, what, 256 if what == rule.SPEED else 3)
                texels = rule_texels(dim_x, dim_y, view)
                dyed.upload(1, texels)
                for byteswap in (True, False):
                    got = b.view_render_members(view, first, count, scaling, byteswap)
                    assert got.shape == (count, scaling * (dim_x - 1), scaling * (dim_y - 1)) and got.dtype == np.uint16
                    what_ = f"{dim_x} x {dim_y}, view {what}, scaling {scaling}, swap {byteswap}"
                    for m in range(count):
                        assert_bit_equal(got[m], oracle.render_rgb565(texels[first + m], scaling, byteswap), f"{what_}, member {first + m} against the oracle")
                    assert_bit_equal(got, dyed.render_members(first, count, scaling, byteswap), what_ + " against a batch whose dye is the texels")
        assert b.view_render_members(view, 1, 0).shape[0] == 0   # count == 0 does nothing
        assert_untouched(b, twin, "view_render_members reads only")


# ---- 4. the stride loop ------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_more_members_than_workgroups(sfl, oracle):
    """65539 members of 2 x 2 at scaling 1: more (member, tile) pairs than the launch has workgroups (65536); the loop's
    second pass takes members 65536 .. 65538.  Texels and scalars take the same path in their kernel."""
    batch, probes = 65539, (0, 65535, 65536, 65538)
    rng = np.random.default_rng(65539)
    v = (rng.uniform(-1, 1, (batch, 2, 2, 2)) * 90).astype(np.float32)
    view = view_of(sfl, rule.VORTICITY, 3)
    with sfl.BatchSolver(2, 2, batch) as b:
        b.upload(0, v)
        images, texels, scalars = b.view_render_members(view, scaling=1), b.view_texels(view), b.view_scalar(rule.VORTICITY)
        assert images.shape == (batch, 1, 1)
        for m in probes:
            s = rule.vorticity(v[m], 1.0)
            t = rule.texels(s, np.float32(view.lo), np.float32(view.hi), view.palette, view.nan_colour)
            assert_bit_equal(scalars[m], s, f"member {m}: scalars")
            assert_bit_equal(texels[m], t, f"member {m}: texels")
            assert_bit_equal(images[m], oracle.render_rgb565(t, 1, True), f"member {m}: image")
        assert_bit_equal(b.download(0), v, "the velocity is as uploaded")


# ---- 5. the recorder ---------------------------------------------------------------------------------------------------
def _record_with_views(sfl, dim_x, dim_y, batch, large):
    """every = 2; each step_n(2) carries a force in its second step, so a batch of small members replays it in one launch
    (batch_play) that ends where the frame is due.  Frame 0 shows the dye, frame 1 the vorticity, frame 2 the dye again,
    frame 3 the pressure; the twin is stepped one step at a time and drawn by the synchronous calls."""
    fields = [member_fields(dim_x, dim_y, 500 + m, 40.0) for m in range(batch)]
    vort, pres = sfl.View(rule.VORTICITY, -30.0, 30.0, sfl.PALETTE_BLUE_WHITE_RED), sfl.View(rule.PRESSURE, -5.0, 5.0, sfl.PALETTE_HEAT)
    shown = [None, vort, None, pres]
    stroke = ([1, batch - 1], [(dim_x // 2, dim_y // 2), (5, 7)], [(600.0, -400.0), (-300.0, 500.0)])
    with sfl.BatchSolver(dim_x, dim_y, batch, large=large) as b, sfl.BatchSolver(dim_x, dim_y, batch, large=large) as twin:
        upload_members(b, fields)
        upload_members(twin, fields)
        with pytest.raises(sfl.SflError) as e:
            b.record_view(vort)
        assert e.value.code == sfl.capi.ERR_STATE
        b.record_start(every=2, first=1, count=batch - 1, scaling=3, capacity=4)
        want = []
        for view in shown:
            if view is not None or want:
                b.record_view(view)
            if view is not None:
                view.palette[:] = 0   # the caller's memory is not read after the call ...
            b.queue_forces(*stroke, step=1)
            b.step_n(2, DT, 1.0, 5, OMEGA)
            if view is not None:
                view.palette[:] = (sfl.PALETTE_BLUE_WHITE_RED if view is vort else sfl.PALETTE_HEAT)   # ... and the twin draws with it
            twin.step_n(1, DT, 1.0, 5, OMEGA)
            twin.queue_forces(*stroke)
            twin.step_n(1, DT, 1.0, 5, OMEGA)
            want.append(twin.render_members(1, batch - 1, 3) if view is None else twin.view_render_members(view, 1, batch - 1, 3))
        assert b.record_info() == (4, 4, 8)
        got = b.frames()
        for f in range(4):
            assert_bit_equal(got[f], want[f], f"frame {f}")
        assert not np.array_equal(got[1], want[0]) and not np.array_equal(got[3], want[2])
        for name, x, y in zip(("velocity", "divergence", "pressure", "colour"), download_all(b), download_all(twin)):
            assert_bit_equal(x, y, f"after eight recorded steps: {name}")
        b.record_start(every=1, first=0, count=1, scaling=1, capacity=1)   # a new recording draws the dye
        b.step_n(1, DT, 1.0, 5, OMEGA)
        twin.step_n(1, DT, 1.0, 5, OMEGA)
        assert_bit_equal(b.frames()[0], twin.render_members(0, 1, 1), "record_start resets to the dye")


@pytest.mark.gpu
def test_recorded_frames_show_the_view_that_was_set(sfl):
    _record_with_views(sfl, 61, 81, 4, False)


@pytest.mark.gpu
def test_recorded_frames_of_a_large_batch(sfl):
    _record_with_views(sfl, 96, 96, 2, True)


# ---- 6. a context ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", [(130, 70), (16, 12)], ids=["tiled", "one-workgroup"])
def test_a_context_is_a_batch_of_one(sfl, dim_x, dim_y):
    """view_render after step_n(3) (fused step boundaries; the one-workgroup path for the small shape) equals that after
    3 x step, bit for bit, and both equal a batch of one that holds the same fields; scalars and texels against the rule."""
    v, c, _ = member_fields(dim_x, dim_y, 130, 40.0)
    views = [sfl.View(rule.VORTICITY, -30.0, 30.0, sfl.PALETTE_BLUE_WHITE_RED), sfl.View(rule.PRESSURE, -5.0, 5.0, sfl.PALETTE_HEAT),
             sfl.View(rule.SPEED, 0.0, 40.0), sfl.View(rule.DIVERGENCE, -1.0, 1.0, dx=0.37)]
    with sfl.Solver(dim_x, dim_y) as fused, sfl.Solver(dim_x, dim_y) as single, sfl.BatchSolver(dim_x, dim_y, 1, large=True) as one:
        for s in (fused, single):
            s.upload(0, v)
            s.upload(1, c)
        fused.step_n(3, DT, 1.0, 5, OMEGA)
        images = [fused.view_render(view, 3, False) for view in views]   # (first: the call itself settles the fields)
        for _ in range(3):
            single.step(DT, 1.0, 5, OMEGA)
        vel, p = single.download(0), single.download(3)
        one.upload(0, vel[None])
        one.upload(3, p[None])
        for view, image in zip(views, images):
            assert image.shape == (3 * (dim_x - 1), 3 * (dim_y - 1))
            assert_bit_equal(image, single.view_render(view, 3, False), f"view {view.what}: step_n(3) against 3 x step")
            assert_bit_equal(image, one.view_render_members(view, scaling=3, byteswap=False)[0], f"view {view.what}: against a batch of one")
            s = rule.scalar(view.what, vel, p, view.dx)
            assert_scalars_equal(fused.view_scalar(view.what, view.dx), s, f"view {view.what}: scalars")
            t = rule.texels(s, np.float32(view.lo), np.float32(view.hi), view.palette, view.nan_colour)
            assert_bit_equal(fused.view_texels(view), t, f"view {view.what}: texels")
            assert_bit_equal(image, rule.render(t, 3, False), f"view {view.what}: the image against the rule's draw")
        assert fused.distance(single)["velocity_cells_differ"] == 0 and fused.distance(single)["pressure_cells_differ"] == 0
        assert fused.distance(single)["dye_cells_differ"] == 0
