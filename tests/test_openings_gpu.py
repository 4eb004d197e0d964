"""Openings on the rim of a batch member's grid on the GPU (include/sfl.h "OPENINGS"; csrc/batch_openings.hip) against
tests/opening_rule.py -- the header's rule in numpy float32, itself anchored on tests/solid_rule.py by tests/test_openings.py.
Every comparison is bit for bit.

Shapes: 7 x 5 (one owned cell per thread and colour), 61 x 81 (the sketch's grid, up to three) and 64 x 96 (the 6144-cell limit);
3 x 3, the smallest grid that holds an opening (a rim cell that is no corner), with members of its own (set "c") at 0, 1 and 3
iterations.
Batches of four and five members with a DIFFERENT map and mask each.  The maps: west in / east out, south in / north out, all
four sides, outflow only, inflow only (run with 3 iterations: its Neumann problem is incompatible and the solve drifts), a slot
of one side, openings on solid rim cells (ignored) and none.  The masks: none, a disc, a channel (solid top and bottom rows,
which also puts openings on solid cells), a seeded 30 %.  Iterations 0, 1, 7, 8, 9 and 19."""
import functools

import numpy as np
import pytest

import load_rule
import opening_rule as rule
import solid_rule
import value_cases
from conftest import assert_bit_equal, random_fields
from test_solids_gpu import NAMES, assert_fields_equal, assert_members_equal, download_all, mask_of, queue

pytestmark = pytest.mark.gpu

DT, DX, OMEGA = 1 / 30.0, 0.7, 1.9
IN, OUT = rule.INFLOW, rule.OUTFLOW
SHAPES = [(7, 5), (61, 81), (64, 96)]


# ---- the maps and the masks --------------------------------------------------------------------------------------------
def map_of(kind, dim_x, dim_y):
    m = np.zeros((dim_y, dim_x), np.uint8)
    if kind in ("west_east", "four", "on_solid"):
        m[1:-1, 0], m[1:-1, -1] = IN, OUT
    if kind in ("south_north", "four", "on_solid"):
        m[0, 1:-1], m[-1, 1:-1] = IN, OUT
    if kind == "out_only":
        m[1:-1, -1] = m[-1, 1:-1] = OUT
    elif kind == "in_only":
        m[1:-1, 0] = IN
    elif kind == "slot":   # the west side whole, a slot of the east side
        m[1:-1, 0] = IN
        m[dim_y // 3 + 1:(2 * dim_y) // 3 + 1, -1] = OUT
    else:
        assert kind in ("west_east", "south_north", "four", "on_solid", "empty"), kind
    return m


def solid_of(kind, dim_x, dim_y):
    if kind == "walls":   # the channel: its top and bottom rows solid
        s = np.zeros((dim_y, dim_x), bool)
        s[0] = s[-1] = True
        return s
    return mask_of("empty" if kind == "none" else kind, dim_x, dim_y)


# (map, mask, inflow) of every member: every map and every mask occurs, the empty map beside a mask and beside none
SETS = {"a": [("west_east", "none", (3.5, 0.0)), ("four", "disc", (2.0, 1.5)), ("slot", "seeded", (-0.0, 0.0)),
              ("on_solid", "walls", (1.25, -0.5)), ("empty", "channel", (9.0, 9.0))],
        "b": [("south_north", "none", (0.0, 2.5)), ("out_only", "seeded", (7.0, 7.0)), ("in_only", "disc", (1.5, 0.0)),
              ("empty", "none", (4.0, 4.0))],
        # 3 x 3: every opening is ONE cell between two corners; "one" makes the centre solid, "walls" leaves a channel of 3 x 1
        "c": [("west_east", "none", (3.5, 0.0)), ("south_north", "none", (0.0, 2.5)), ("four", "none", (2.0, 1.5)),
              ("four", "one", (1.25, -0.5)), ("west_east", "walls", (-0.0, 0.75))]}


@functools.lru_cache(maxsize=None)
def members_of(name, dim_x, dim_y):
    """(maps uint8[B, dim_y, dim_x], masks bool[B, dim_y, dim_x], inflow float32[B, 2]); shared, never written."""
    maps = np.stack([map_of(k, dim_x, dim_y) for k, _, _ in SETS[name]])
    masks = np.stack([solid_of(k, dim_x, dim_y) for _, k, _ in SETS[name]])
    inflow = np.array([u for _, _, u in SETS[name]], np.float32)
    for a in (maps, masks, inflow):
        a.setflags(write=False)
    return maps, masks, inflow


def test_the_members_hold_the_cases_they_are_there_for():
    for dim_x, dim_y in SHAPES:
        maps, masks, _ = members_of("a", dim_x, dim_y)
        (_, _, os_, on), out = rule.sides(maps[3], masks[3])
        assert not os_.any() and not on.any() and maps[3][0].any() and out.any(), "openings on solid rim cells do not count"
        assert not maps[4].any() and masks[4].any() and rule.inflow_cells(maps[1], masks[1]).sum() > 2
        slot = maps[2][:, -1] == OUT
        assert 0 < slot.sum() < dim_y - 2
        maps, masks, _ = members_of("b", dim_x, dim_y)
        assert not (maps[2] == OUT).any() and not (maps[1] == IN).any() and not maps[3].any() and not masks[3].any()
    maps, masks, _ = members_of("c", 3, 3)
    for m in range(len(maps)):   # at least one inflow and one outflow cell that counts in every member, and a fluid cell without one
        assert rule.inflow_cells(maps[m], masks[m]).any() and rule.sides(maps[m], masks[m])[1].any() and (~masks[m] & (maps[m] == 0)).any()
    assert masks[3][1, 1] and masks[3].sum() == 1 and (~masks[4]).sum() == 3 and not maps[4][0].any() and not maps[4][-1].any()
    n = solid_rule.count_present(mask_of("seeded", 61, 81))
    assert all((n[:, 0] == k).any() or (n[:, -1] == k).any() for k in (1, 2, 3)), "rim cells of every present count carry an opening"


@functools.lru_cache(maxsize=None)
def fields_of(dim_x, dim_y, batch):
    v, c = zip(*(random_fields(dim_x, dim_y, 300 + m, vamp=40.0)[:2] for m in range(batch)))
    v, c = np.stack(v), np.stack(c)
    v.setflags(write=False)
    c.setflags(write=False)
    return v, c


def forces_of(dim_x, dim_y, maps, masks):
    """step -> [(member, i, j, vx, vy)]: in steps 0 and 2; on an inflow cell (no effect), on an outflow cell, on a fluid cell
    twice (the later wins), on a solid cell, outside the grid."""
    out = {0: [], 2: []}
    for m in range(len(maps)):
        fluid = np.argwhere(~masks[m] & (maps[m] == 0))
        j, i = fluid[len(fluid) // 3]
        out[0] += [(m, int(i), int(j), 30.0, -20.0), (m, int(i), int(j), -12.5, 7.25)]
        for kind, step in ((IN, 0), (OUT, 2), (IN, 2)):
            cells = np.argwhere((maps[m] == kind) & ~masks[m])
            if len(cells):
                j, i = cells[len(cells) // 2]
                out[step].append((m, int(i), int(j), 55.0, 66.0))
        solid = np.argwhere(masks[m])
        if len(solid):
            j, i = solid[len(solid) // 2]
            out[2].append((m, int(i), int(j), 5.0, 6.0))
    out[0].append((0, dim_x, 0, 1.0, 1.0))
    return out


@functools.lru_cache(maxsize=None)
def rule_steps(name, dim_x, dim_y, iters, steps=3):
    """The members after `steps` steps of the rule with the forces of forces_of.  Computed once, shared, never written."""
    from oracle import loader
    cpu = loader.port()
    maps, masks, inflow = members_of(name, dim_x, dim_y)
    v, c = fields_of(dim_x, dim_y, len(maps))
    forces = forces_of(dim_x, dim_y, maps, masks)
    out = []
    for m in range(len(maps)):
        state = (v[m], None, None, c[m])
        for k in range(steps):
            mine = [r[1:] for r in forces.get(k, []) if r[0] == m]
            state = rule.step(cpu, state[0], state[3], masks[m], maps[m], inflow[m], DT, DX, iters, OMEGA, mine)
        out.append(state)
    return out


def make(sfl, dim_x, dim_y, batch, maps=None, inflow=(0.0, 0.0), masks=None, fields=None):
    """A batch with the shape's fields uploaded and, unless None, the masks and the maps set."""
    b = sfl.BatchSolver(dim_x, dim_y, batch)
    v, c = fields_of(dim_x, dim_y, batch) if fields is None else fields
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)
    if masks is not None:
        b.set_solids(masks)
    if maps is not None:
        b.set_openings(maps, inflow)
    return b


def reload(sfl, b, dim_x, dim_y, batch):
    v, c = fields_of(dim_x, dim_y, batch)
    b.upload(sfl.capi.FIELD_VELOCITY, v)
    b.upload(sfl.capi.FIELD_COLOR, c)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- 1. step_n against the rule ------------------------------------------------------------------------------------------
CASES = [(3, 3, "c", it) for it in (0, 1, 3)] + [(7, 5, "a", it) for it in (0, 1, 7, 8, 9, 19)] + \
    [(7, 5, "b", 3), (61, 81, "a", 8), (61, 81, "b", 3), (64, 96, "a", 19), (64, 96, "b", 9)]


@pytest.mark.parametrize("dim_x,dim_y,name,iters", CASES, ids=[f"{x}x{y}-{n}-i{it}" for x, y, n, it in CASES])
def test_three_steps_are_three_steps_of_the_rule(sfl, dim_x, dim_y, name, iters):
    maps, masks, inflow = members_of(name, dim_x, dim_y)
    B = len(maps)
    forces = forces_of(dim_x, dim_y, maps, masks)
    want = rule_steps(name, dim_x, dim_y, iters)
    with make(sfl, dim_x, dim_y, B, maps, inflow, masks) as b:
        live_in = int(sum(rule.inflow_cells(maps[m], masks[m]).sum() for m in range(B)))
        live_out = int(sum(rule.sides(maps[m], masks[m])[1].sum() for m in range(B)))
        assert b.openings_info() == (True, True, True, live_in, live_out)
        got_maps, got_inflow = b.openings()
        assert np.array_equal(got_maps, maps) and np.array_equal(bits(got_inflow), bits(inflow))
        assert b.solids_info() == (True, True) and np.array_equal(b.solids(), masks), "the solids are what they were"
        for k, records in forces.items():
            queue(b, records, k)
        b.step_n(3, DT, DX, iters, OMEGA)
        once = download_all(sfl, b)
        assert_members_equal(once, want, "step_n(3)")
        # ... and step_n(1) called three times gives the same bits; the other order of setting too
        reload(sfl, b, dim_x, dim_y, B)
        b.set_solids(None)
        b.set_solids(masks)
        for k in range(3):
            queue(b, forces.get(k, []))
            b.step_n(1, DT, DX, iters, OMEGA)
        assert_fields_equal(download_all(sfl, b), once, "step_n(1) x 3")


# ---- 2. no opening: the bits of the batch without openings ---------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "solids"])
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (61, 81)], ids=["7x5", "61x81"])
def test_an_empty_map_and_a_cleared_map_give_the_bits_of_the_batch_without_openings(sfl, dim_x, dim_y, masked):
    maps, masks, inflow = members_of("a", dim_x, dim_y)
    B, iters = len(maps), 7
    masks = masks if masked else None
    records = [(m, 2, 2, 11.0, -3.0) for m in range(B)]

    def run(b):
        queue(b, records)
        b.step_n(2, DT, DX, iters, OMEGA)
        b.step_n_each(1, [DT] * B, [DX] * B, [iters + m for m in range(B)], [OMEGA] * B)
        return download_all(sfl, b), b.residual(), b.flow_stats(DX)

    with make(sfl, dim_x, dim_y, B, masks=masks) as plain, make(sfl, dim_x, dim_y, B, np.zeros_like(maps), inflow, masks) as empty, \
            make(sfl, dim_x, dim_y, B, maps, inflow, masks) as cleared:
        want = run(plain)
        assert empty.openings_info() == (True, True, True, 0, 0)
        got = run(empty)
        assert_fields_equal(got[0], want[0], "an empty map")
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
        other = run(cleared)
        assert not np.array_equal(other[0][0], want[0][0]), "a member with openings is another flow"
        reload(sfl, cleared, dim_x, dim_y, B)
        cleared.set_openings(None)
        assert cleared.openings_info() == (False, False, False, 0, 0) and not cleared.openings()[0].any()
        got = run(cleared)
        assert_fields_equal(got[0], want[0], "a cleared map")
        assert np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])


# ---- 3. per-member parameters: one batch per member ----------------------------------------------------------------------
EACH = dict(dt=[1 / 30.0, 1 / 60.0, 1 / 20.0, 1 / 45.0, 1 / 30.0], dx=[0.7, 1.0, 1.3, 0.37, 1.0], iters=[5, 8, 3, 9, 0], omega=[1.9, 1.5, 1.96, 1.7, 1.9])


@pytest.mark.parametrize("dim_x,dim_y,name", [(7, 5, "a"), (61, 81, "a"), (64, 96, "b")], ids=["7x5", "61x81", "64x96"])
def test_step_n_each_with_per_member_inflow_equals_one_batch_per_member(sfl, oracle, dim_x, dim_y, name):
    maps, masks, inflow = members_of(name, dim_x, dim_y)
    B = len(maps)
    v, c = fields_of(dim_x, dim_y, B)
    prm = {k: EACH[k][:B] for k in EACH}
    with make(sfl, dim_x, dim_y, B, maps, inflow, masks) as b:
        b.step_n_each(2, prm["dt"], prm["dx"], prm["iters"], prm["omega"])
        got, norm = download_all(sfl, b), b.residual()
    for m in range(B):
        mine = [prm[k][m] for k in ("dt", "dx", "iters", "omega")]
        with make(sfl, dim_x, dim_y, 1, maps[m], inflow[m], masks[m], (v[m:m + 1], c[m:m + 1])) as one:
            assert one.openings_info()[1:3] == (False, False)
            one.step_n(1, *mine)
            one.step_n_each(1, *[[x] for x in mine])
            single, single_norm = download_all(sfl, one), one.residual()
        for field, g, w in zip(NAMES, got, single):
            assert_bit_equal(g[m], w[0], f"member {m} against a batch of its own: {field}")
        assert bits(norm[m:m + 1])[0] == bits(single_norm)[0], (m, norm[m], single_norm)
        # ... and both are the rule's
        first = rule.step(oracle, v[m], c[m], masks[m], maps[m], inflow[m], *mine)
        want = rule.step(oracle, first[0], first[3], masks[m], maps[m], inflow[m], *mine)
        for field, g, w in zip(NAMES, got, want):
            assert_bit_equal(g[m], w, f"step_n_each: member {m} {field}")
        want_norm = rule.update_norm(want[2], want[1], masks[m], maps[m], mine[1])
        assert bits(norm[m:m + 1])[0] == want_norm.view(np.uint32), (m, norm[m], want_norm)


# ---- 4. the operators one by one -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y,name,iters", [(3, 3, "c", 0), (3, 3, "c", 1), (3, 3, "c", 3), (7, 5, "a", 9), (7, 5, "b", 3), (61, 81, "a", 19),
                                                    (61, 81, "b", 1), (64, 96, "a", 7), (64, 96, "b", 8)],
                         ids=["3x3-i0", "3x3-i1", "3x3-i3", "7x5-a", "7x5-b", "61x81-a", "61x81-b", "64x96-a", "64x96-b"])
def test_the_solves_and_the_statistics_follow_the_rule(sfl, dim_x, dim_y, name, iters):
    cap = sfl.capi
    maps, masks, inflow = members_of(name, dim_x, dim_y)
    B = len(maps)
    rhs = np.stack([random_fields(dim_x, dim_y, 60 + m)[2] for m in range(B)])
    dxs, its, oms = EACH["dx"][:B], [iters + m for m in range(B)], EACH["omega"][:B]
    with make(sfl, dim_x, dim_y, B, maps, inflow, masks) as b:
        v = b.download(cap.FIELD_VELOCITY)
        b.upload(cap.FIELD_DIVERGENCE, rhs)
        p0 = np.zeros_like(rhs)
        p0[masks] = np.nan   # (zero-filled away)
        b.upload(cap.FIELD_PRESSURE, p0)
        b.poisson_solve(DX, iters, OMEGA)
        p = b.download(cap.FIELD_PRESSURE)
        for m in range(B):
            assert_bit_equal(p[m], rule.solve(rhs[m], masks[m], maps[m], DX, iters, OMEGA), f"poisson_solve: member {m}")
        b.poisson_solve_each(dxs, its, oms)
        p, norm = b.download(cap.FIELD_PRESSURE), b.residual()
        for m in range(B):
            want = rule.solve(rhs[m], masks[m], maps[m], dxs[m], its[m], oms[m])
            assert_bit_equal(p[m], want, f"poisson_solve_each: member {m}")
            want_norm = rule.update_norm(want, rhs[m], masks[m], maps[m], dxs[m])
            assert bits(norm[m:m + 1])[0] == want_norm.view(np.uint32), (m, norm[m], want_norm)
        # the solves impose no inflow and touch no velocity
        assert_bit_equal(b.download(cap.FIELD_VELOCITY), v, "the velocity behind the solves")
        uniform, each = b.flow_stats(DX), b.flow_stats(dxs)

    def worst(a):
        return np.abs(a).max().astype(np.float32)

    for m in range(B):
        for got, dx in ((uniform[m], DX), (each[m], dxs[m])):
            for field, want in (("max_abs_vx", worst(v[m, ..., 0])), ("max_abs_vy", worst(v[m, ..., 1])),
                                ("max_abs_div", worst(rule.divergence(v[m], masks[m], maps[m], dx)))):
                assert np.float32(got[field]).view(np.uint32) == want.view(np.uint32), (m, field, got[field], want)


def test_a_uniform_flow_passes_through_the_open_channel(sfl):
    """The fixed point of tests/test_openings.py on the device: no divergence, no pressure, every velocity bit kept; the closed
    batch reports max|div| = U on the same field."""
    dim_x, dim_y, U = 61, 41, np.float32(3.5)
    solid, open = solid_of("walls", dim_x, dim_y), map_of("west_east", dim_x, dim_y)
    v = np.zeros((2, dim_y, dim_x, 2), np.float32)
    v[:, ~solid, 0] = U
    c = fields_of(dim_x, dim_y, 2)[1]
    with make(sfl, dim_x, dim_y, 2, open, (U, 0.0), solid, (v, c)) as b:
        assert b.openings_info() == (True, False, False, 2 * (dim_y - 2), 2 * (dim_y - 2))
        assert all(np.float32(s["max_abs_div"]).view(np.uint32) == 0 for s in b.flow_stats(1.0))
        b.step_n(1, 0.0, 1.0, 5, OMEGA)
        got = download_all(sfl, b)
        assert_bit_equal(got[0], v, "velocity")
        assert not got[1].view(np.uint32).any() and not (got[2].view(np.uint32) & 0x7FFFFFFF).any()
        b.set_openings(None)
        assert all(np.float32(s["max_abs_div"]) == U for s in b.flow_stats(1.0))


# ---- 5. a shared map, and the inflow changed without the map -------------------------------------------------------------
def test_a_shared_map_is_the_map_repeated_and_set_inflow_changes_the_speed_alone(sfl, oracle):
    dim_x, dim_y, B, iters = 61, 81, 3, 8
    open, solid = map_of("four", dim_x, dim_y), mask_of("disc", dim_x, dim_y)
    sweep = np.array([[1.0, 0.0], [2.5, 0.5], [4.0, -1.0]], np.float32)
    v, c = fields_of(dim_x, dim_y, B)
    with make(sfl, dim_x, dim_y, B, open, (2.0, 1.0), solid) as shared, make(sfl, dim_x, dim_y, B, np.stack([open] * B), np.stack([[2.0, 1.0]] * B), solid) as each:
        assert shared.openings_info()[:3] == (True, False, False) and each.openings_info()[:3] == (True, True, True)
        assert shared.openings_info()[3:] == each.openings_info()[3:]
        for b in (shared, each):
            b.step_n(2, DT, DX, iters, OMEGA)
        assert_fields_equal(download_all(sfl, shared), download_all(sfl, each), "shared against per member")
        assert np.array_equal(shared.flow_stats(DX), each.flow_stats(DX))
        # one batch as a sweep over the tunnel speed
        reload(sfl, shared, dim_x, dim_y, B)
        shared.set_inflow(sweep)
        assert shared.openings_info()[:3] == (True, False, True) and np.array_equal(shared.openings()[1], sweep)
        shared.step_n(1, DT, DX, iters, OMEGA)
        got = download_all(sfl, shared)
        for m in range(B):
            for field, g, w in zip(NAMES, got, rule.step(oracle, v[m], c[m], solid, open, sweep[m], DT, DX, iters, OMEGA)):
                assert_bit_equal(g[m], w, f"the sweep: member {m} {field}")


# ---- 6. loads beside openings --------------------------------------------------------------------------------------------
def test_loads_next_to_openings_are_the_rule_of_the_loads_on_the_downloaded_pressure(sfl):
    dim_x, dim_y, B = 61, 81, 3
    open, solid = map_of("west_east", dim_x, dim_y), mask_of("disc", dim_x, dim_y)
    with make(sfl, dim_x, dim_y, B, open, (3.5, 0.0), solid) as b:
        b.step_n(2, DT, DX, 9, OMEGA)
        p, got = b.download(sfl.capi.FIELD_PRESSURE), b.loads()
    for m in range(B):
        want = load_rule.loads(p[m], solid)
        assert got[m].tobytes() == want.tobytes(), (m, got[m], want)
    assert any(got[m]["fx"].any() for m in range(B))


# ---- 7. values at the bottom of the float range --------------------------------------------------------------------------
VALUES = [("tiny", None, (2.0 ** -140, 0.0)), ("zeros", None, (-0.0, 0.0)), ("quiescent", value_cases.AMPLITUDES[1], (3e-36, 0.0))]


@pytest.mark.parametrize("texture,amplitude,inflow", VALUES, ids=[v[0] for v in VALUES])
def test_the_value_classes_run_through_the_step_and_the_inflow_keeps_its_bits(sfl, oracle, texture, amplitude, inflow):
    dim_x, dim_y, iters, dx = 61, 81, 6, 0.37
    t = value_cases.texture(texture, dim_x, dim_y, amplitude)
    open, solid = map_of("west_east", dim_x, dim_y), mask_of("disc", dim_x, dim_y)
    inflow = np.array(inflow, np.float32)
    state, want = (t.v, None, None, t.dye), []
    for k in range(3):
        state = rule.step(oracle, state[0], state[3], solid, open, inflow, DT, dx, iters, OMEGA, t.forces if k == 0 else ())
        want.append(state)
    # the guards, on the rule alone: the case is one of its class
    if texture == "zeros":
        assert value_cases.negative_zeros(want[0][1]) >= 1 and value_cases.negative_zeros(want[0][2]) >= 1
    else:
        assert min(value_cases.denormals(a) for a in want[-1][:3]) >= 100, [value_cases.denormals(a) for a in want[-1][:3]]
    with make(sfl, dim_x, dim_y, 2, open, inflow, solid, (np.stack([t.v] * 2), np.stack([t.dye] * 2))) as b:
        assert np.array_equal(bits(b.openings()[1]), bits(np.stack([inflow] * 2))), "the inflow keeps its bits"
        for k in range(3):
            queue(b, [(m,) + tuple(r) for m in range(2) for r in (t.forces if k == 0 else ())])
            b.step_n(1, DT, dx, iters, OMEGA)
            got = download_all(sfl, b)
            for m in range(2):
                for field, g, w in zip(NAMES, got, want[k]):
                    assert_bit_equal(g[m], w, f"{texture}: step {k} member {m} {field}")


# ---- 8. the refusals that need a device ----------------------------------------------------------------------------------
def test_what_does_not_know_openings_is_refused_and_the_batch_steps_on(sfl, oracle):
    dim_x, dim_y, iters = 7, 5, 7
    cap = sfl.capi
    maps, _, inflow = members_of("a", dim_x, dim_y)
    masks = np.zeros(maps.shape, bool)   # (no solids: with them set, their own refusals of the same calls come first)
    B = len(maps)
    v, c = fields_of(dim_x, dim_y, B)

    def refused(call, *words, code=cap.ERR_STATE):
        with pytest.raises(sfl.SflError) as e:
            call()
        assert e.value.code == code, e.value
        for word in words:
            assert word in str(e.value), (word, str(e.value))

    with sfl.BatchSolver(96, 96, 2, large=True) as large:
        refused(lambda: large.set_openings(map_of("west_east", 96, 96), (1.0, 0.0)), "sfl_batch_create_large")
        assert large.openings_info() == (False, False, False, 0, 0)
        large.step_n(1, DT, DX, iters, OMEGA)
    div = sfl.View(cap.VIEW_DIVERGENCE, -1.0, 1.0, dx=DX)
    with make(sfl, dim_x, dim_y, B, maps, inflow) as b:
        bad = maps.copy()
        bad[1, 0, 0] = IN
        refused(lambda: b.set_openings(bad, inflow), "map 1, cell (0, 0)", "is a corner", code=cap.ERR_INVALID)
        bad[1, 0, 0], bad[2, 2, 3] = 0, OUT
        refused(lambda: b.set_openings(bad, inflow), "map 2, cell (3, 2)", "interior cell", code=cap.ERR_INVALID)
        bad[2, 2, 3], bad[0, 1, 0] = 0, 3
        refused(lambda: b.set_openings(bad, inflow), "cell (0, 1) holds 3", code=cap.ERR_INVALID)
        refused(lambda: b.set_openings(maps, (np.nan, 0.0)), "must be finite", code=cap.ERR_INVALID)
        refused(lambda: b.set_inflow(np.full((B, 2), np.inf, np.float32)), "must be finite", code=cap.ERR_INVALID)
        refused(lambda: b.step_n_until(1, DT, DX, iters, OMEGA, tol=1e-3), "sfl_batch_step_n_until", "openings set")
        refused(lambda: b.poisson_solve_until(DX, iters, OMEGA, tol=1e-3), "sfl_batch_poisson_solve_until", "openings set")
        refused(lambda: b.history_start(1, 4), "sfl_batch_history_start", "openings set")
        assert b.history_info() == (0, 0, 0)
        refused(lambda: b.view_scalar(cap.VIEW_DIVERGENCE, DX), "sfl_batch_view_scalar", "divergence view")
        refused(lambda: b.view_texels(div), "sfl_batch_view_texels")
        b.record_start(every=1, scaling=1, capacity=2)
        refused(lambda: b.record_view(div), "sfl_batch_record_view", "divergence view")
        b.record_stop()
        refused(lambda: b.set_viscosity(0.1, 2), "sfl_batch_set_viscosity", "openings set")
        assert b.openings_info()[:3] == (True, True, True) and np.array_equal(b.openings()[0], maps)
        # ... and the batch steps on, by the rule
        b.step_n(1, DT, DX, iters, OMEGA)
        got = download_all(sfl, b)
        for m in range(B):
            for field, g, w in zip(NAMES, got, rule.step(oracle, v[m], c[m], masks[m], maps[m], inflow[m], DT, DX, iters, OMEGA)):
                assert_bit_equal(g[m], w, f"after the refusals: member {m} {field}")
        # what is on first refuses a map; clearing is let through
        b.set_openings(None)
        refused(lambda: b.set_inflow((1.0, 0.0)), "no openings set")
        b.history_start(1, 4)
        refused(lambda: b.set_openings(maps, inflow), "a history is on")
        b.history_stop()
        b.record_start(every=1, scaling=1, capacity=2)
        b.record_view(div)
        refused(lambda: b.set_openings(maps, inflow), "recorder draws the divergence view")
        b.record_stop()
        b.set_viscosity(0.1, 2)
        refused(lambda: b.set_openings(maps, inflow), "viscosity is set")
        assert b.openings_info() == (False, False, False, 0, 0)
        b.set_openings(None)
        b.set_viscosity(None, 0)
        b.set_openings(maps, inflow)
        assert b.openings_info()[:3] == (True, True, True)
        b.step_n(1, DT, DX, iters, OMEGA)
