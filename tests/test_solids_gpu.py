"""Solid cells inside a batch member's grid on the GPU (include/sfl.h "SOLIDS"; csrc/batch_solids.hip) against
tests/solid_rule.py -- the header's rule in numpy float32, itself held to the reference and the oracle by tests/test_solids.py.
Every comparison is bit for bit.

Shapes: 2 x 2 with all 16 masks as one batch of 16; 7 x 5 (one owned cell per thread and colour is the most any thread gets);
33 x 18 (an odd width, half = 17); 61 x 81 (the sketch's grid, up to three owned cells per thread and colour); 96 x 64 (the
6144-cell limit).  Batches of three members with a DIFFERENT mask each, one of them empty and never in the same place, which
catches member offsets formed from the wrong stride.  The masks: one cell, a disc, a plate touching a domain wall, a
one-cell-wide dead-end channel (present == 1), an isolated fluid cell (present == 0), all solid, and a seeded 30 %."""
import functools

import numpy as np
import pytest

import solid_rule as rule
from conftest import assert_bit_equal, random_fields

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 6, 1.9
NAMES = ("velocity", "divergence", "pressure", "colour")


# ---- the masks -------------------------------------------------------------------------------------------------------
def mask_of(kind, dim_x, dim_y, seed=7):
    m = np.zeros((dim_y, dim_x), bool)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    cx, cy = dim_x // 2, dim_y // 2
    if kind == "one":
        m[cy, cx] = True
    elif kind == "disc":
        m[(i - cx) ** 2 + (j - cy) ** 2 <= (min(dim_x, dim_y) // 4) ** 2] = True
    elif kind == "plate":   # from the wall j = 0 half way up
        m[0:cy + 1, dim_x // 3] = True
    elif kind == "channel":   # a block with a corridor one cell wide, open to the west, closed in the east
        m[1:4, 1:dim_x - 1] = True
        m[2, 1:dim_x - 2] = False
    elif kind == "isolated":   # a fluid cell walled in on all four sides
        m[cy - 1, cx] = m[cy + 1, cx] = m[cy, cx - 1] = m[cy, cx + 1] = True
    elif kind == "all":
        m[:] = True
    elif kind == "seeded":
        m = np.random.default_rng(seed).random((dim_y, dim_x)) < 0.3
    else:
        assert kind == "empty"
    return m


# shape -> the three members' masks: every kind occurs, the empty one in every position
TRIPLES = {(7, 5): ("channel", "empty", "isolated"), (33, 18): ("empty", "plate", "all"), (61, 81): ("disc", "seeded", "empty"),
           (96, 64): ("seeded", "empty", "one")}
SHAPES = list(TRIPLES)
IDS = [f"{x}x{y}" for x, y in SHAPES]


@functools.lru_cache(maxsize=None)
def masks_of(dim_x, dim_y):
    if (dim_x, dim_y) == (2, 2):   # all 16 masks: bit c of the member's number = cell c is solid
        m = np.array([[(n >> c) & 1 for c in range(4)] for n in range(16)], bool).reshape(16, 2, 2)
    else:
        m = np.stack([mask_of(kind, dim_x, dim_y) for kind in TRIPLES[(dim_x, dim_y)]])
    m.setflags(write=False)
    return m


def test_the_masks_hold_the_cases_they_are_there_for():
    assert (rule.count_present(mask_of("channel", 7, 5)) == 1).any() and (rule.count_present(mask_of("isolated", 7, 5)) == 0).any()
    n = rule.count_present(mask_of("seeded", 61, 81))
    assert all((n == k).any() for k in range(5))
    assert mask_of("plate", 33, 18)[0].any() and mask_of("disc", 61, 81).sum() > 100 and mask_of("one", 96, 64).sum() == 1


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y, batch):
    """Seeded velocity and dye of every member (solid cells hold velocity too: the rule reads it as it stands).  Shared, never written."""
    v, c = zip(*(random_fields(dim_x, dim_y, 100 + m, vamp=40.0)[:2] for m in range(batch)))
    v, c = np.stack(v), np.stack(c)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y, masks):
    """step -> [(member, i, j, vx, vy)]: records in steps 0 and 2, one of them on a solid cell where a member has one, one
    outside the grid, two on one cell (the later wins)."""
    out = {0: [], 2: []}
    for m, mask in enumerate(masks):
        fluid, solid = np.argwhere(~mask), np.argwhere(mask)
        if len(fluid):
            j, i = fluid[len(fluid) // 3]
            out[0] += [(m, int(i), int(j), 30.0, -20.0), (m, int(i), int(j), -12.5, 7.25)]
            j, i = fluid[(2 * len(fluid)) // 3]
            out[2].append((m, int(i), int(j), 9.0, 11.0))
        if len(solid):
            j, i = solid[len(solid) // 2]
            out[2 if m % 2 else 0].append((m, int(i), int(j), 55.0, 66.0))
    out[0].append((0, dim_x, 0, 1.0, 1.0))
    return out


def queue(b, records, step=0):
    if records:
        b.queue_forces([r[0] for r in records], [r[1:3] for r in records], [r[3:5] for r in records], step)


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, steps=3):
    """The members after `steps` steps of the rule with the forces of forces_of: [(v, div, p, colour)] per member.  Computed
    once, shared, never written."""
    from oracle import loader
    cpu = loader.port()
    masks = masks_of(dim_x, dim_y)
    v, c = fields_of(dim_x, dim_y, len(masks))
    forces = forces_of(dim_x, dim_y, masks)
    out = []
    for m, mask in enumerate(masks):
        state = (v[m], None, None, c[m])
        for k in range(steps):
            mine = [r[1:] for r in forces.get(k, []) if r[0] == m]
            state = rule.step(cpu, state[0], state[3], mask, DT, DX, ITERS, OMEGA, mine)
        out.append(state)
    return out


def make(sfl, dim_x, dim_y, masks=None, fields=None, batch=None):
    """A batch with the shape's fields uploaded and, unless None, the masks set."""
    batch = len(masks) if batch is None else batch
    b = sfl.BatchSolver(dim_x, dim_y, batch)
    v, c = fields_of(dim_x, dim_y, batch) if fields is None else fields
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)
    if masks is not None:
        b.set_solids(masks)
    return b


def download_all(sfl, b):
    cap = sfl.capi
    return tuple(b.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))


def assert_members_equal(got, want, what):
    """got: fields [B, ...]; want: per member (v, div, p, colour)."""
    for m, fields in enumerate(want):
        for name, g, w in zip(NAMES, got, fields):
            assert_bit_equal(g[m], w, f"{what}: member {m} {name}")


def assert_fields_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_bit_equal(g, w, f"{what}: {name}")


# ---- 1. step_n against the rule ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2)] + SHAPES, ids=["2x2"] + IDS)
def test_step_n_is_three_steps_of_the_rule(sfl, dim_x, dim_y):
    masks = masks_of(dim_x, dim_y)
    forces = forces_of(dim_x, dim_y, masks)
    want = rule_steps(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, masks) as b:
        assert b.solids_info() == (True, True) and np.array_equal(b.solids(), masks)
        for k, records in forces.items():
            queue(b, records, k)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        once = download_all(sfl, b)
        assert_members_equal(once, want, "step_n(3)")
        # ... and step_n(1) called three times gives the same bits
        v, c = fields_of(dim_x, dim_y, len(masks))
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.upload(sfl.capi.FIELD_COLOR, c)
        for k in range(3):
            queue(b, forces.get(k, []))
            b.step_n(1, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, b), once, "step_n(1) x 3")


# ---- 2. the empty-mask member is the plain kernel's -----------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (96, 64)], ids=["61x81", "96x64"])
def test_a_member_without_solid_cells_equals_the_plain_batch(sfl, dim_x, dim_y):
    masks = masks_of(dim_x, dim_y)
    empty = TRIPLES[(dim_x, dim_y)].index("empty")
    forces = forces_of(dim_x, dim_y, masks)
    with make(sfl, dim_x, dim_y, batch=len(masks)) as plain, make(sfl, dim_x, dim_y, masks) as b:
        for x in (plain, b):
            for k, records in forces.items():
                queue(x, records, k)
            x.step_n(3, DT, DX, ITERS, OMEGA)
        want, got = download_all(sfl, plain), download_all(sfl, b)
        for name, g, w in zip(NAMES, got, want):
            assert_bit_equal(g[empty], w[empty], f"member {empty} {name}")
        other = (empty + 1) % 3
        assert not np.array_equal(got[0][other], want[0][other])   # (a member with solid cells is another flow)
        # after set_solids(None) the whole batch is the plain one again
        v, c = fields_of(dim_x, dim_y, len(masks))
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.upload(sfl.capi.FIELD_COLOR, c)
        b.set_solids(None)
        assert b.solids_info() == (False, False) and not b.solids().any()
        for k, records in forces.items():
            queue(b, records, k)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, b), want, "cleared")


# ---- 3. the frame identity ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (94, 62)], ids=["63x83", "96x64"])
def test_inside_a_solid_ring_the_kernels_compute_the_plain_inner_grid(sfl, dim_x, dim_y):
    cap, B = sfl.capi, 3
    v, c = fields_of(dim_x, dim_y, B)
    rhs = np.stack([random_fields(dim_x, dim_y, 40 + m)[2] for m in range(B)])
    ring = np.ones((dim_y + 2, dim_x + 2), bool)
    ring[1:-1, 1:-1] = False

    def framed(a, fill):
        return np.ascontiguousarray(np.pad(a, [(0, 0), (1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 3), constant_values=fill))

    inner = (slice(None), slice(1, -1), slice(1, -1))
    with make(sfl, dim_x, dim_y, batch=B) as plain, make(sfl, dim_x + 2, dim_y + 2, ring, (framed(v, 0), framed(c, 0)), B) as b:
        assert b.solids_info() == (True, False)
        plain.upload(cap.FIELD_DIVERGENCE, rhs)
        b.upload(cap.FIELD_DIVERGENCE, framed(rhs, 5.0))   # (what the ring holds of the rhs plays no part)
        plain.poisson_solve(DX, ITERS, OMEGA)
        b.poisson_solve(DX, ITERS, OMEGA)
        p = b.download(cap.FIELD_PRESSURE)
        assert_bit_equal(np.ascontiguousarray(p[inner]), plain.download(cap.FIELD_PRESSURE), "poisson_solve")
        assert not p[:, ring].view(np.uint32).any()
        plain.step_n(1, 0.0, DX, ITERS, OMEGA)
        b.step_n(1, 0.0, DX, ITERS, OMEGA)
        for name, f in zip(NAMES[:3], (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE)):
            assert_bit_equal(np.ascontiguousarray(b.download(f)[inner]), plain.download(f), f"step at dt = 0: {name}")


# ---- 4. per-member parameters and the update norm ----------------------------------------------------------------------
EACH = dict(dt=[1 / 30.0, 1 / 60.0, 1 / 20.0], dx=[0.7, 1.0, 1.3], iters=[5, 8, 3], omega=[1.9, 1.5, 1.96])


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=IDS)
def test_step_n_each_and_solve_each_follow_the_rule_and_report_its_update_norm(sfl, oracle, dim_x, dim_y):
    cap = sfl.capi
    masks = masks_of(dim_x, dim_y)
    v, c = fields_of(dim_x, dim_y, 3)
    with make(sfl, dim_x, dim_y, masks) as b:
        b.step_n_each(2, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
        got, norm = download_all(sfl, b), b.residual()
        for m, mask in enumerate(masks):
            prm = [EACH[k][m] for k in ("dt", "dx", "iters", "omega")]
            want = rule.step(oracle, *rule.step(oracle, v[m], c[m], mask, *prm)[::3], mask, *prm)
            for name, g, w in zip(NAMES, got, want):
                assert_bit_equal(g[m], w, f"step_n_each: member {m} {name}")
            want_norm = rule.update_norm(want[2], want[1], mask, prm[1])
            assert norm[m:m + 1].view(np.uint32)[0] == want_norm.view(np.uint32), (m, norm[m], want_norm)
            if mask.all():
                assert norm[m:m + 1].view(np.uint32)[0] == 0
        # poisson_solve_each on an uploaded rhs; a NaN in the PRESSURE of a solid cell is zero-filled away
        rhs = np.stack([random_fields(dim_x, dim_y, 60 + m)[2] for m in range(3)])
        p0 = np.zeros_like(rhs)
        p0[masks] = np.nan
        b.upload(cap.FIELD_DIVERGENCE, rhs)
        b.upload(cap.FIELD_PRESSURE, p0)
        b.poisson_solve_each(EACH["dx"], EACH["iters"], EACH["omega"])
        p, norm = b.download(cap.FIELD_PRESSURE), b.residual()
        for m, mask in enumerate(masks):
            want = rule.solve(rhs[m], mask, EACH["dx"][m], EACH["iters"][m], EACH["omega"][m])
            assert_bit_equal(p[m], want, f"poisson_solve_each: member {m}")
            want_norm = rule.update_norm(want, rhs[m], mask, EACH["dx"][m])
            assert norm[m:m + 1].view(np.uint32)[0] == want_norm.view(np.uint32) and not np.isnan(norm[m]), (m, norm[m], want_norm)
        # a NaN in the rhs of a fluid cell is reported; one in the rhs of a solid cell is not
        bad = rhs.copy()
        fluid0 = np.argwhere(~masks[0])
        fj, fi = fluid0[len(fluid0) // 2]
        bad[0, fj, fi] = np.nan
        for m in (1, 2):
            bad[m][masks[m]] = np.nan
        b.upload(cap.FIELD_DIVERGENCE, bad)
        b.poisson_solve_each(EACH["dx"], EACH["iters"], EACH["omega"])
        norm = b.residual()
        assert np.isnan(norm[0]) and not np.isnan(norm[1:]).any(), norm


# ---- 5. flow statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2)] + SHAPES, ids=["2x2"] + IDS)
def test_flow_stats_report_the_rules_divergence(sfl, dim_x, dim_y):
    masks = masks_of(dim_x, dim_y)
    B = len(masks)
    dxs = [0.7 + 0.1 * (m % 4) for m in range(B)]
    with make(sfl, dim_x, dim_y, masks) as b:
        b.step_n(1, DT, DX, ITERS, OMEGA)
        v, c = b.download(sfl.capi.FIELD_VELOCITY), b.download(sfl.capi.FIELD_COLOR)
        uniform, each = b.flow_stats(DX), b.flow_stats(dxs)
        only = b.flow_stats(DX, velocity=True, dye=False)

    def worst(a):
        return np.abs(a).max().astype(np.float32)

    for m in range(B):
        for got, dx in ((uniform[m], DX), (each[m], dxs[m]), (only[m], DX)):
            for name, want in (("max_abs_vx", worst(v[m, ..., 0])), ("max_abs_vy", worst(v[m, ..., 1])),
                               ("max_abs_div", worst(rule.divergence(v[m], masks[m], dx)))):
                assert np.float32(got[name]).view(np.uint32) == want.view(np.uint32), (m, name, got[name], want)
        for got in (uniform[m], each[m]):
            assert list(got["dye_sum"]) == [int(c[m, ..., k].astype(np.uint64).sum()) for k in range(3)], m
        assert not only[m]["dye_sum"].any()


# ---- 6. one mask for all members ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y,kind", [(33, 18, "plate"), (61, 81, "seeded")], ids=["33x18", "61x81"])
def test_a_shared_mask_is_the_same_mask_repeated(sfl, dim_x, dim_y, kind):
    mask = mask_of(kind, dim_x, dim_y)
    with make(sfl, dim_x, dim_y, mask, batch=3) as shared, make(sfl, dim_x, dim_y, np.stack([mask] * 3)) as each:
        assert shared.solids_info() == (True, False) and each.solids_info() == (True, True)
        assert np.array_equal(shared.solids(), each.solids())
        for b in (shared, each):
            b.step_n(2, DT, DX, ITERS, OMEGA)
            b.step_n_each(1, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
        assert_fields_equal(download_all(sfl, shared), download_all(sfl, each), "shared against per member")
        assert np.array_equal(shared.residual().view(np.uint32), each.residual().view(np.uint32))
        assert np.array_equal(shared.flow_stats(DX), each.flow_stats(DX))


# ---- 7. tracers, the recorder and the vorticity view beside solids -------------------------------------------------------
def test_tracers_and_recorders_run_beside_solids(sfl):
    dim_x, dim_y, steps = 33, 18, 4
    masks = masks_of(dim_x, dim_y)
    forces = {0: forces_of(dim_x, dim_y, masks)[0], 2: forces_of(dim_x, dim_y, masks)[2]}   # (a timeline: records in a later step)
    xy = np.random.default_rng(5).uniform(1.0, 16.0, (3, 40, 2)).astype(np.float32)
    vort = sfl.View(sfl.capi.VIEW_VORTICITY, -30.0, 30.0, dx=DX)
    with make(sfl, dim_x, dim_y, masks) as plain, make(sfl, dim_x, dim_y, masks) as dye, make(sfl, dim_x, dim_y, masks) as view:
        # the existing calls, after each step
        plain.set_tracers(xy, follow=False)
        frames, views, trail = [], [], []
        for k in range(steps):
            queue(plain, forces.get(k, []))
            plain.step_n(1, DT, DX, ITERS, OMEGA)
            plain.advance_tracers(DT)
            frames.append(plain.render_members(scaling=2))
            views.append(plain.view_render_members(vort, scaling=2))
            trail.append(plain.tracers())
        want = download_all(sfl, plain)
        # one call each with everything following
        dye.set_tracers(xy, follow=True)
        dye.trail_start(1, steps)
        dye.record_start(every=1, scaling=2, capacity=steps)
        view.record_start(every=1, scaling=2, capacity=steps)
        view.record_view(vort)
        for b in (dye, view):
            for k, records in forces.items():
                queue(b, records, k)
            b.step_n(steps, DT, DX, ITERS, OMEGA)
            assert_fields_equal(download_all(sfl, b), want, "fields beside tracers and a recorder")
        assert np.array_equal(dye.frames(), np.stack(frames)) and np.array_equal(view.frames(), np.stack(views))
        assert np.array_equal(dye.trail().view(np.uint32), np.stack(trail).view(np.uint32))
        # the vorticity view reads the zero velocity of solid cells through its ordinary stencil
        import view_rule
        w = view.view_scalar(sfl.capi.VIEW_VORTICITY, DX)
        for m in range(3):
            assert_bit_equal(w[m], view_rule.vorticity(want[0][m], DX), f"vorticity of member {m}")


# ---- 8. the refusals that need a device ----------------------------------------------------------------------------------
def test_what_does_not_know_solids_is_refused_and_the_batch_steps_on(sfl, oracle):
    dim_x, dim_y = 7, 5
    cap = sfl.capi
    masks = masks_of(dim_x, dim_y)
    v, c = fields_of(dim_x, dim_y, 3)

    def refused(call, *words):
        with pytest.raises(sfl.SflError) as e:
            call()
        assert e.value.code == cap.ERR_STATE, e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    with sfl.BatchSolver(96, 96, 2, large=True) as large:
        refused(lambda: large.set_solids(np.zeros((96, 96), bool)), "sfl_batch_create_large")
        assert large.solids_info() == (False, False)
        large.step_n(1, DT, DX, ITERS, OMEGA)
    div = sfl.View(cap.VIEW_DIVERGENCE, -1.0, 1.0, dx=DX)
    with make(sfl, dim_x, dim_y, masks) as b:
        refused(lambda: b.step_n_until(1, DT, DX, ITERS, OMEGA, tol=1e-3), "sfl_batch_step_n_until", "solid cells set")
        refused(lambda: b.poisson_solve_until(DX, ITERS, OMEGA, tol=1e-3), "sfl_batch_poisson_solve_until", "solid cells set")
        refused(lambda: b.history_start(1, 4), "sfl_batch_history_start", "solid cells set")
        assert b.history_info() == (0, 0, 0)
        refused(lambda: b.view_scalar(cap.VIEW_DIVERGENCE, DX), "sfl_batch_view_scalar", "divergence view")
        refused(lambda: b.view_texels(div), "sfl_batch_view_texels")
        refused(lambda: b.view_render_members(div, scaling=1), "sfl_batch_view_render_members")
        b.record_start(every=1, scaling=1, capacity=2)
        refused(lambda: b.record_view(div), "sfl_batch_record_view", "divergence view")
        b.record_stop()
        # ... and the batch steps on, by the rule
        b.step_n(1, DT, DX, ITERS, OMEGA)
        got = download_all(sfl, b)
        for m, mask in enumerate(masks):
            for name, g, w in zip(NAMES, got, rule.step(oracle, v[m], c[m], mask, DT, DX, ITERS, OMEGA)):
                assert_bit_equal(g[m], w, f"after the refusals: member {m} {name}")
        # a history that is on, or a recorder on the divergence view, refuses a mask; clearing is let through
        b.set_solids(None)
        b.history_start(1, 4)
        refused(lambda: b.set_solids(masks), "a history is on")
        b.history_stop()
        b.record_start(every=1, scaling=1, capacity=2)
        b.record_view(div)
        refused(lambda: b.set_solids(masks), "recorder draws the divergence view")
        assert b.solids_info() == (False, False)
        b.record_stop()
        b.set_solids(masks)
        assert b.solids_info() == (True, True)
