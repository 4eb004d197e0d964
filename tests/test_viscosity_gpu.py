"""Viscosity on the GPU (include/sfl.h "VISCOSITY"; csrc/batch_viscous.hip, csrc/context_viscous.hip) against
tests/viscosity_rule.py -- the header's rule in numpy float32 -- composed with the oracle's advections and, where a mask is
set, with tests/solid_rule.py.  Every comparison is bit for bit.

Batches: 2 x 2, 7 x 5 (one owned cell per thread and colour at most), 61 x 81 (the sketch's grid, up to three) and 96 x 64
(the 6144-cell limit: u0 fills the whole of d and p), five members with nu = 0, three decades and one large value, three
steps with forces, sweeps 1 and 3, without solids, with one mask per member and with a shared one.  Contexts: the shapes and
sweep counts of the CPU tile test -- inside one tile, exactly one, one cell more, ragged tiles -- so that every launch
segmentation (one launch, D, D + 1, three launches) runs on the device too."""
import functools

import numpy as np
import pytest

import solid_rule
import viscosity_rule as rule
from conftest import assert_bit_equal, random_fields
from test_solids_gpu import mask_of
from test_viscosity import D, SHAPES, SWEEPS, TX, TY

pytestmark = pytest.mark.gpu

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 6, 1.9
NAMES = ("velocity", "divergence", "pressure", "colour")
B = 5
NUS = np.array([0.0, 0.003, 0.04, 0.5, 12.0], np.float32)
EACH = dict(dt=[1 / 30.0, 1 / 60.0, 1 / 20.0, 1 / 45.0, 1 / 30.0], dx=[0.7, 1.0, 1.3, 0.9, 0.55], iters=[5, 8, 3, 6, 4],
            omega=[1.9, 1.5, 1.96, 1.7, 1.8])
BATCH_SHAPES = [(2, 2), (7, 5), (61, 81), (96, 64)]
BATCH_IDS = [f"{x}x{y}" for x, y in BATCH_SHAPES]
KINDS = {(7, 5): ("channel", "empty", "isolated", "seeded", "one"), (61, 81): ("disc", "seeded", "empty", "plate", "one"),
         (96, 64): ("seeded", "empty", "one", "disc", "plate")}


@functools.lru_cache(maxsize=None)
def masks_of(dim_x, dim_y, solids):
    """None, one mask per member [B, dim_y, dim_x] or one for all [dim_y, dim_x]."""
    if solids == "none":
        return None
    if (dim_x, dim_y) == (2, 2):   # bit c of the number = cell c is solid
        m = np.array([[(n >> c) & 1 for c in range(4)] for n in (6, 0, 1, 15, 9)], bool).reshape(5, 2, 2)
    else:
        m = np.stack([mask_of(kind, dim_x, dim_y) for kind in KINDS[(dim_x, dim_y)]])
    m = m if solids == "each" else m[0]
    m.setflags(write=False)
    return m


def member_mask(masks, m):
    return None if masks is None else masks[m] if masks.ndim == 3 else masks


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y, batch=B):
    v, c = zip(*(random_fields(dim_x, dim_y, 300 + m, vamp=40.0)[:2] for m in range(batch)))
    v, c = np.stack(v), np.stack(c)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y):
    """step -> [(member, i, j, vx, vy)]: records in steps 0 and 2, two on one cell (the later wins), one outside the grid."""
    out = {0: [], 2: []}
    for m in range(B):
        i, j = (3 * m + 1) % dim_x, (2 * m + 1) % dim_y
        out[0] += [(m, i, j, 30.0, -20.0), (m, i, j, -12.5, 7.25)]
        out[2].append((m, (i + 1) % dim_x, j, 9.0, 11.0))
    out[0].append((0, dim_x, 0, 1.0, 1.0))
    return out


def queue(b, forces):
    for k, recs in forces.items():
        if recs:
            b.queue_forces([r[0] for r in recs], [r[1:3] for r in recs], [r[3:5] for r in recs], k)


@functools.lru_cache(maxsize=None)
def rule_steps(dim_x, dim_y, solids, sweeps, each, steps=3):
    """Every member after `steps` steps of the rule: [(v, div, p, colour)].  Computed once, shared, never written."""
    from oracle import loader
    cpu = loader.port()
    masks = masks_of(dim_x, dim_y, solids)
    v, c = fields_of(dim_x, dim_y)
    forces = forces_of(dim_x, dim_y)
    out = []
    for m in range(B):
        prm = [EACH[k][m] for k in ("dt", "dx", "iters", "omega")] if each else [DT, DX, ITERS, OMEGA]
        state = (v[m], None, None, c[m])
        for k in range(steps):
            mine = [r[1:] for r in forces.get(k, []) if r[0] == m]
            state = rule.step(cpu, state[0], state[3], *prm, nu=NUS[m], sweeps=sweeps, solid=member_mask(masks, m), forces=mine)
        out.append(state)
    return out


def make(sfl, dim_x, dim_y, masks=None, nu=None, sweeps=0):
    b = sfl.BatchSolver(dim_x, dim_y, B)
    v, c = fields_of(dim_x, dim_y)
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)
    if masks is not None:
        b.set_solids(masks)
    if nu is not None:
        b.set_viscosity(nu, sweeps)
    return b


def download_all(sfl, b):
    cap = sfl.capi
    return tuple(b.download(f) for f in (cap.FIELD_VELOCITY, cap.FIELD_DIVERGENCE, cap.FIELD_PRESSURE, cap.FIELD_COLOR))


def assert_members_equal(got, want, what):
    for m, fields in enumerate(want):
        for name, g, w in zip(NAMES, got, fields):
            assert_bit_equal(g[m], w, f"{what}: member {m} {name}")


def assert_fields_equal(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        assert_bit_equal(g, w, f"{what}: {name}")


# ---- batches: step_n and step_n_each against the rule ----------------------------------------------------------------------
@pytest.mark.parametrize("sweeps", [1, 3])
@pytest.mark.parametrize("solids", ["none", "each", "shared"])
@pytest.mark.parametrize("dim_x,dim_y", BATCH_SHAPES, ids=BATCH_IDS)
def test_step_n_and_step_n_each_are_three_steps_of_the_rule(sfl, dim_x, dim_y, solids, sweeps):
    masks = masks_of(dim_x, dim_y, solids)
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, masks, NUS, sweeps) as b:
        nu, s = b.viscosity()
        assert np.array_equal(nu, NUS) and s == sweeps
        queue(b, forces)
        b.step_n(3, DT, DX, ITERS, OMEGA)
        assert_members_equal(download_all(sfl, b), rule_steps(dim_x, dim_y, solids, sweeps, False), "step_n(3)")
        v, c = fields_of(dim_x, dim_y)
        b.upload(sfl.capi.FIELD_VELOCITY, v)
        b.upload(sfl.capi.FIELD_COLOR, c)
        queue(b, forces)
        b.step_n_each(3, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
        want = rule_steps(dim_x, dim_y, solids, sweeps, True)
        assert_members_equal(download_all(sfl, b), want, "step_n_each(3)")
        norm = b.residual()
        for m in range(B):
            mask = member_mask(masks, m)
            mask = np.zeros((dim_y, dim_x), bool) if mask is None else mask
            want_norm = solid_rule.update_norm(want[m][2], want[m][1], mask, EACH["dx"][m])
            assert norm[m:m + 1].view(np.uint32)[0] == want_norm.view(np.uint32), (m, norm[m], want_norm)


@pytest.mark.parametrize("solids", ["none", "each"])
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (96, 64)], ids=["61x81", "96x64"])
def test_a_member_with_nu_zero_equals_the_plain_batchs_member(sfl, dim_x, dim_y, solids):
    masks = masks_of(dim_x, dim_y, solids)
    forces = forces_of(dim_x, dim_y)
    with make(sfl, dim_x, dim_y, masks) as plain, make(sfl, dim_x, dim_y, masks, NUS, 3) as b, \
            make(sfl, dim_x, dim_y, masks, np.float32(0.0), 3) as zeros:
        for x in (plain, b, zeros):
            queue(x, forces)
            x.step_n(2, DT, DX, ITERS, OMEGA)
            x.step_n_each(1, EACH["dt"], EACH["dx"], EACH["iters"], EACH["omega"])
        want, got = download_all(sfl, plain), download_all(sfl, b)
        for name, g, w in zip(NAMES, got, want):
            assert_bit_equal(g[0], w[0], f"member 0 (nu = 0) {name}")
        assert not np.array_equal(got[0][3], want[0][3])   # (a member with a viscosity is another flow)
        # every member at nu = 0: the viscous kernels ran and gave the plain batch's bits
        assert zeros.viscosity()[1] == 3 and not zeros.viscosity()[0].any()
        assert_fields_equal(download_all(sfl, zeros), want, "all members at nu = 0")
        # cleared: the plain batch again
        v, c = fields_of(dim_x, dim_y)
        for x in (plain, b):
            x.upload(sfl.capi.FIELD_VELOCITY, v)
            x.upload(sfl.capi.FIELD_COLOR, c)
        b.set_viscosity(None, 0)
        assert b.viscosity()[1] == 0 and not b.viscosity()[0].any()
        for x in (plain, b):
            queue(x, forces)
            x.step_n(3, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, b), download_all(sfl, plain), "cleared")


def test_the_until_step_and_the_large_batch_are_refused_and_the_batch_steps_on(sfl):
    dim_x, dim_y, cap = 7, 5, sfl.capi

    def refused(call, *words):
        with pytest.raises(sfl.SflError) as e:
            call()
        assert e.value.code == cap.ERR_STATE, e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    with sfl.BatchSolver(96, 96, 2, large=True) as large:
        refused(lambda: large.set_viscosity(0.5, 2), "sfl_batch_create_large", "no room for u0")
        assert large.viscosity()[1] == 0
        large.step_n(1, DT, DX, ITERS, OMEGA)
    with make(sfl, dim_x, dim_y, None, NUS, 1) as b:
        refused(lambda: b.step_n_until(1, DT, DX, ITERS, OMEGA, tol=1e-3), "sfl_batch_step_n_until", "a viscosity set")
        queue(b, forces_of(dim_x, dim_y))
        b.step_n(3, DT, DX, ITERS, OMEGA)
        assert_members_equal(download_all(sfl, b), rule_steps(dim_x, dim_y, "none", 1, False), "after the refusals")


def test_the_recorder_tracers_a_history_and_loads_run_beside_it_unchanged(sfl):
    dim_x, dim_y, steps, sweeps = 61, 81, 3, 3
    masks = masks_of(dim_x, dim_y, "each")
    xy = np.random.default_rng(5).uniform(1.0, 50.0, (B, 40, 2)).astype(np.float32)
    with make(sfl, dim_x, dim_y, masks, NUS, sweeps) as by_hand, make(sfl, dim_x, dim_y, masks, NUS, sweeps) as b:
        by_hand.set_tracers(xy, follow=False)
        frames, trail, loads = [], [], []
        for k in range(steps):
            by_hand.step_n(1, DT, DX, ITERS, OMEGA)
            by_hand.advance_tracers(DT)
            frames.append(by_hand.render_members(scaling=1))
            trail.append(by_hand.tracers())
            loads.append(by_hand.loads())
        b.set_tracers(xy, follow=True)
        b.trail_start(1, steps)
        b.record_start(every=1, scaling=1, capacity=steps)
        b.loads_start(1, steps)
        b.step_n(steps, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, b), download_all(sfl, by_hand), "fields beside the followers")
        assert np.array_equal(b.frames(), np.stack(frames))
        assert np.array_equal(b.trail().view(np.uint32), np.stack(trail).view(np.uint32))
        assert b.loads_history().tobytes() == np.stack(loads).tobytes() and np.stack(loads)["faces"].any()
    # a history (batches without solids): every record is what flow_stats returns after the same step
    with make(sfl, dim_x, dim_y, None, NUS, sweeps) as by_hand, make(sfl, dim_x, dim_y, None, NUS, sweeps) as b:
        stats = []
        for k in range(steps):
            by_hand.step_n(1, DT, DX, ITERS, OMEGA)
            stats.append(by_hand.flow_stats(DX))
        b.history_start(1, steps)
        b.step_n(steps, DT, DX, ITERS, OMEGA)
        assert_fields_equal(download_all(sfl, b), download_all(sfl, by_hand), "fields beside a history")
        rec = b.history()
        for k in range(steps):
            for name in ("max_abs_vx", "max_abs_vy", "max_abs_div", "dye_sum"):
                assert np.array_equal(rec[k][name], stats[k][name]), (k, name)


# ---- contexts ------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def context_fields(dim_x, dim_y):
    v, c, _ = random_fields(dim_x, dim_y, 77, vamp=40.0)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def context(sfl, dim_x, dim_y, mask=None, **kw):
    s = sfl.Solver(dim_x, dim_y, **kw)
    if kw.get("nranks", 1) == 1:
        v, c = context_fields(dim_x, dim_y)
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
    if mask is not None:
        s.set_solids(mask)
    return s


def context_mask(kind, dim_x, dim_y):
    from test_context_solids import mask
    return None if kind is None else mask(kind, dim_x, dim_y)


@pytest.mark.parametrize("kind", [None, "seeded", "plate"])
@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=[f"{x}x{y}" for x, y in SHAPES])
def test_diffuse_velocity_equals_the_rule(sfl, dim_x, dim_y, kind):
    cap, nu, dt = sfl.capi, 0.35, 0.04
    v, _ = context_fields(dim_x, dim_y)
    solid = context_mask(kind, dim_x, dim_y)
    with context(sfl, dim_x, dim_y, solid) as s:
        rhs = random_fields(dim_x, dim_y, 9)[2]
        s.upload(cap.FIELD_DIVERGENCE, rhs)
        s.upload(cap.FIELD_PRESSURE, rhs)
        for sweeps in SWEEPS:
            s.upload(cap.FIELD_VELOCITY, v)
            s.diffuse_velocity(nu, dt, DX, sweeps)
            assert_bit_equal(s.download(cap.FIELD_VELOCITY), rule.diffuse(v, nu, dt, DX, sweeps, solid), f"{kind}, {sweeps} sweeps")
        s.diffuse_velocity(0.0, dt, DX, 3)
        assert_bit_equal(s.download(cap.FIELD_VELOCITY), rule.diffuse(v, nu, dt, DX, SWEEPS[-1], solid), "nu = 0 changes nothing")
        assert s.viscosity() == (0.0, 0), "the operator sets nothing"
        assert_bit_equal(s.download(cap.FIELD_DIVERGENCE), rhs, "the divergence is not touched")
        assert_bit_equal(s.download(cap.FIELD_PRESSURE), rhs, "the pressure is not touched")


@pytest.mark.parametrize("kind", [None, "disc"])
@pytest.mark.parametrize("dim_x,dim_y", [(61, 81), (96, 64)], ids=["61x81", "96x64"])
def test_three_steps_of_a_context_equal_a_batch_member(sfl, dim_x, dim_y, kind):
    v, c = context_fields(dim_x, dim_y)
    solid = None if kind is None else mask_of(kind, dim_x, dim_y)
    nu, sweeps = 0.3, D + 2   # (the context: two launches and the third buffer; the member: ten sweeps in LDS)
    with context(sfl, dim_x, dim_y, solid) as s, sfl.BatchSolver(dim_x, dim_y, 2) as b:
        b.upload(sfl.capi.FIELD_VELOCITY, np.stack([v, v]))
        b.upload(sfl.capi.FIELD_COLOR, np.stack([c, c]))
        if solid is not None:
            b.set_solids(solid)
        b.set_viscosity(nu, sweeps)
        s.set_viscosity(nu, sweeps)
        assert s.viscosity() == (np.float32(nu), sweeps)
        for x in (s, b):
            if x is s:
                x.queue_forces([(3, 4)], [(25.0, -15.0)], 1)
            else:
                x.queue_forces([0, 1], [(3, 4), (3, 4)], [(25.0, -15.0), (25.0, -15.0)], 1)
            x.step_n(3, DT, DX, ITERS, OMEGA)
        got, want = download_all(sfl, s), download_all(sfl, b)
        for name, g, w in zip(NAMES, got, want):
            assert_bit_equal(g, w[1], f"context against member: {name}")


@pytest.mark.parametrize("kind", [None, "plate"])
def test_three_steps_of_a_context_of_ragged_tiles_equal_the_rule(sfl, oracle, kind):
    dim_x, dim_y = 2 * TX + 3, TY - 1
    v, c = context_fields(dim_x, dim_y)
    solid = context_mask(kind, dim_x, dim_y)
    nu, sweeps = 0.3, D + 1
    with context(sfl, dim_x, dim_y, solid) as s:
        s.set_viscosity(nu, sweeps)
        s.queue_forces([(TX, 4)], [(25.0, -15.0)], 1)
        s.step_n(3, DT, DX, ITERS, OMEGA)
        state = (v, None, None, c)
        for k in range(3):
            state = rule.step(oracle, state[0], state[3], DT, DX, ITERS, OMEGA, nu=nu, sweeps=sweeps, solid=solid,
                              forces=[(TX, 4, 25.0, -15.0)] if k == 1 else [])
        assert_fields_equal(download_all(sfl, s), state, "step_n(3)")


def test_a_cleared_viscosity_gives_the_plain_contexts_bits(sfl):
    dim_x, dim_y = 257, 130
    with context(sfl, dim_x, dim_y) as plain, context(sfl, dim_x, dim_y) as s:
        s.set_viscosity(0.3, 2)
        s.step_n(1, DT, DX, ITERS, OMEGA)
        v, c = context_fields(dim_x, dim_y)
        s.upload(sfl.capi.FIELD_VELOCITY, v)
        s.upload(sfl.capi.FIELD_COLOR, c)
        s.set_viscosity(0.0, 2)
        assert s.viscosity() == (0.0, 0)
        for x in (plain, s):
            x.step_n(3, DT, DX, ITERS, OMEGA)   # (with the step seams back on)
        assert_fields_equal(download_all(sfl, s), download_all(sfl, plain), "cleared")


def test_a_slab_and_a_transport_are_refused(sfl):
    cap = sfl.capi
    with context(sfl, 64, 512, nranks=2) as slab:
        for call in (lambda: slab.set_viscosity(0.3, 2), lambda: slab.diffuse_velocity(0.3, DT, DX, 2)):
            with pytest.raises(cap.SflError, match="whole-domain contexts only") as e:
                call()
            assert e.value.code == cap.ERR_STATE
        assert slab.viscosity() == (0.0, 0)
    with context(sfl, TX + 1, TY + 1) as s:
        s.set_viscosity(0.3, 2)
        for call in (s.comm_emulate, s.comm_emulate_rccl, lambda: s.comm_attach(bytes(256)), lambda: sfl.Solver.link_group([s])):
            with pytest.raises(cap.SflError, match="a viscosity set") as e:
                call()
            assert e.value.code == cap.ERR_STATE
        s.set_viscosity(0.0, 0)
        sfl.Solver.link_group([s])   # a group of one: the context has a transport now
        for call in (lambda: s.set_viscosity(0.3, 2), lambda: s.diffuse_velocity(0.3, DT, DX, 2)):
            with pytest.raises(cap.SflError, match="transport attached") as e:
                call()
            assert e.value.code == cap.ERR_STATE
