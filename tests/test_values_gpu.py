"""Denormal, quiescent and signed-zero fields in every compute kernel written since the SOR kernels: the textures of
tests/value_cases.py through batches, contexts, stopping rules and readers, against the oracle and the rules, bit for bit.
No comparison here has a tolerance.  Every expected field comes from value_cases.expected and its kin, which assert their
guard first (enough denormal cells, negative zeros present), so that no case goes vacuous; tests/test_values.py asserts the
same guards without a GPU, pins the yardsticks to the compiled reference on these inputs and shows that a flush anywhere
changes what is compared here.

Which test launches which kernel file on a denormal-bearing texture (the quiescent and the tiny members):

  small_grid.hip, small_grid_core.h, small_step_body.inc   test_contexts_step_by_the_oracle[plain-61x81] (the one-launch
                                                           step); test_a_context_stops_at_the_rules_iteration[sketch]
  batch_grid.hip                                           test_small_batches[*-step_n], [*-each] (a launch per step)
  batch_play.hip                                           test_small_batches[*-replay], [*-each-replay] (the timeline in one launch)
  batch_large.hip, large_member_core.h                     test_large_batches, test_batches_stop_at_the_rules_iteration[large],
                                                           test_stopped_steps_of_a_batch[96x96]
  batch_solids.hip                                         test_batches_with_solids_and_viscosity[*-solids], [*-both]
  batch_viscous.hip                                        test_batches_with_solids_and_viscosity[*-viscous], [*-both]
  batch_member.h                                           the step body of the two files above: their tests (member_step and
                                                           apply_member: every batch test here)
  context_solids.hip, sor_solid_tile.h                     test_contexts_step_by_the_oracle[masked-*],
                                                           test_the_operators_one_by_one[disc], test_a_context_stops_...[masked]
  context_viscous.hip, diffuse_tile.h                      test_contexts_step_by_the_oracle[viscous-*], test_diffuse_velocity
  the _until checks                                        test_batches_stop_at_the_rules_iteration, test_stopped_steps_of_a_batch
  update_norm.hip                                          test_a_context_stops_at_the_rules_iteration[general], [masked]
  history.hip                                              test_a_history_beside_the_steps
  field_distance.hip                                       test_distances_to_a_flushed_copy, test_distance_between_zeros_of_both_signs
  tracers.hip                                              test_tracers_follow_and_sample
  (the general kernels -- the stencil kernels, both advections, the fused solve, the step seams -- are held to these textures
  by test_contexts_step_by_the_oracle[plain-130x70 ... plain-300x141] and test_the_operators_one_by_one[None] as well.)"""
import numpy as np
import pytest

import solid_rule
import value_cases as vc
from conftest import assert_bit_equal
from test_batch_params import assert_report_equal, update_norm
from test_context_solids import D as SOLID_D
from test_ensemble_gpu import assert_distance, yardstick as distance_yardstick
from test_solids_gpu import mask_of
from test_tracers_gpu import assert_same

pytestmark = pytest.mark.gpu

F = np.float32
FV, FC, FDIV, FP = 0, 1, 2, 3       # SFL_FIELD_VELOCITY, SFL_FIELD_COLOR, SFL_FIELD_DIVERGENCE, SFL_FIELD_PRESSURE
NAMES = ("velocity", "divergence", "pressure", "colour")
CONTEXT_CASES = vc.context_cases()


def tag(case):
    return f"{case.name} {case.amplitude or ''} {case.dim_x}x{case.dim_y}"


# ---- plumbing ------------------------------------------------------------------------------------------------------------
def load_batch(b, cases):
    """Velocity and dye of every member, and every member's records on the timeline."""
    textures = [vc.texture(c.name, c.dim_x, c.dim_y, c.amplitude) for c in cases]
    b.upload(FV, np.stack([t.v for t in textures]))
    b.upload(FC, np.stack([t.dye for t in textures]))
    for step in range(vc.STEPS):
        recs = [(m, r) for m, c in enumerate(cases) for r in vc.forces_of(c, step)]
        if recs:
            b.queue_forces([m for m, _ in recs], [r[:2] for _, r in recs], [r[2:] for _, r in recs], step)


def load_context(s, case):
    t = vc.texture(case.name, case.dim_x, case.dim_y, case.amplitude)
    s.upload(FV, t.v)
    s.upload(FC, t.dye)
    for step in range(vc.STEPS):
        recs = vc.forces_of(case, step)
        if recs:
            s.queue_forces([r[:2] for r in recs], [r[2:] for r in recs], step)


def fields_of(x):
    return [x.download(f) for f in (FV, FDIV, FP, FC)]


def assert_members(got, cases, what):
    for m, case in enumerate(cases):
        for name, g, w in zip(NAMES, got, vc.expected(case)[-1]):
            assert_bit_equal(g[m], w, f"{what}: member {m} ({tag(case)}) {name}")


def params_of(sfl, cases):
    return sfl.member_params(len(cases), [c.dt for c in cases], [c.dx for c in cases], [c.iters for c in cases], [c.omega for c in cases])


def run_batch(sfl, b, cases, each):
    if each:
        b.step_n_each(vc.STEPS, params_of(sfl, cases))
    else:
        b.step_n(vc.STEPS, vc.DT, vc.DX, vc.ITERS, vc.OMEGA)


# ---- batches ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", list(vc.SMALL_CALLS))
@pytest.mark.parametrize("dim_x,dim_y", vc.SMALL_SHAPES, ids=[f"{x}x{y}" for x, y in vc.SMALL_SHAPES])
def test_small_batches(sfl, dim_x, dim_y, call):
    """step_n with the records in step 0 only (a launch per step), with one more in step 1 (the timeline replayed in one
    launch) and step_n_each with every member's own dt, dx, iters and omega, both ways: all four fields of every member."""
    cases = vc.batch_cases(dim_x, dim_y, **vc.SMALL_CALLS[call])
    with sfl.BatchSolver(dim_x, dim_y, len(cases)) as b:
        load_batch(b, cases)
        assert b.forces_pending()[1] == (1 if "replay" in call else 0)
        run_batch(sfl, b, cases, "each" in call)
        assert_members(fields_of(b), cases, f"{dim_x}x{dim_y} {call}")
        if "each" in call:
            for m, case in enumerate(cases):
                _, d, p, _ = vc.expected(case)[-1]
                assert_report_equal(b.residual()[m], update_norm(p, d, case.dx), f"member {m} ({tag(case)}): the update norm")


@pytest.mark.parametrize("call", list(vc.LARGE_CALLS))
@pytest.mark.parametrize("dim_x,dim_y", vc.LARGE_SHAPES, ids=[f"{x}x{y}" for x, y in vc.LARGE_SHAPES])
def test_large_batches(sfl, dim_x, dim_y, call):
    cases = vc.batch_cases(dim_x, dim_y, **vc.LARGE_CALLS[call])
    with sfl.BatchSolver(dim_x, dim_y, len(cases), large=True) as b:
        assert b.large
        load_batch(b, cases)
        run_batch(sfl, b, cases, call == "each")
        assert_members(fields_of(b), cases, f"large {dim_x}x{dim_y} {call}")
        if call == "each":
            for m, case in enumerate(cases):
                _, d, p, _ = vc.expected(case)[-1]
                assert_report_equal(b.residual()[m], update_norm(p, d, case.dx), f"member {m} ({tag(case)}): the update norm")


@pytest.mark.parametrize("variant", list(vc.RULED_VARIANTS))
@pytest.mark.parametrize("dim_x,dim_y", vc.RULED_SHAPES, ids=[f"{x}x{y}" for x, y in vc.RULED_SHAPES])
def test_batches_with_solids_and_viscosity(sfl, dim_x, dim_y, variant):
    """Solids alone (a disc or a seeded mask per member), viscosity alone (3 sweeps, one member at nu = 0) and both."""
    cases = vc.batch_cases(dim_x, dim_y, **vc.RULED_VARIANTS[variant])
    with sfl.BatchSolver(dim_x, dim_y, len(cases)) as b:
        load_batch(b, cases)
        if cases[0].mask is not None:
            b.set_solids(np.stack([vc.solid_of(c) for c in cases]))
            assert {c.mask for c in cases} == {"disc", "seeded"}
        if variant != "solids":
            nus = np.array([c.nu for c in cases], F)
            assert (nus == 0).any() or dim_x * dim_y < vc.SKETCH
            b.set_viscosity(nus, vc.SWEEPS)
        b.step_n(vc.STEPS, vc.DT, vc.DX, vc.ITERS, vc.OMEGA)
        assert_members(fields_of(b), cases, f"{dim_x}x{dim_y} {variant}")


# ---- stopping rules with denormal tolerances -------------------------------------------------------------------------------
UNTIL_BATCHES = {"7x9": (vc.UNTIL_SMALL, False), "sketch": (vc.UNTIL_SKETCH, False), "large": (vc.UNTIL_LARGE, True)}


@pytest.mark.parametrize("which", list(UNTIL_BATCHES))
def test_batches_stop_at_the_rules_iteration(sfl, which):
    """poisson_solve_until with tolerances of 1e-40, 1e-42 and 0.0 on right-hand sides of 2^-110 to 2^-122: the iterations,
    the reported norm and the pressure are the rule's, whose norm passes 1.2e-38 long before it stops."""
    members, large = UNTIL_BATCHES[which]
    dim_x, dim_y = members[0][:2]
    for u in members:
        vc.until_guard(u)
    with sfl.BatchSolver(dim_x, dim_y, len(members), large=large) as b:
        b.upload(FDIV, np.stack([vc.until_rhs(u) for u in members]))
        b.poisson_solve_until(1.0, [u.cap for u in members], [u.omega for u in members], [u.tol for u in members], [u.every for u in members])
        p, its, res = b.download(FP), b.iterations(), b.residual()
    for m, u in enumerate(members):
        k, want_p, norm = vc.until_answer(u)
        print(u, "k", its[m], "want", k, "norm", res[m], "want", norm)
        assert tuple(its[m]) == (k, k), f"member {m} {u}: iterations {its[m]}, the rule's {k} (on a flushed norm {vc.until_answer(u, True)[0]})"
        assert_report_equal(res[m], norm, f"member {m} {u}: the norm")
        assert_bit_equal(p[m], want_p, f"member {m} {u}: the pressure at k = {k}")


@pytest.mark.parametrize("dim_x,dim_y,large", vc.UNTIL_STEP_SHAPES, ids=[f"{x}x{y}" for x, y, _ in vc.UNTIL_STEP_SHAPES])
def test_stopped_steps_of_a_batch(sfl, dim_x, dim_y, large):
    """step_n_until over two steps: every member's fields, its iterations (last, sum) and its norm are the rule's."""
    members = vc.until_step_members(dim_x, dim_y)
    cases = [c for c, _, _ in members]
    for member in members:
        vc.until_step_guard(*member)
    with sfl.BatchSolver(dim_x, dim_y, len(members), large=large) as b:
        load_batch(b, cases)
        b.step_n_until(vc.UNTIL_STEPS, params_of(sfl, cases), tol=sfl.member_stops(len(members), [t for _, t, _ in members], [e for _, _, e in members]))
        got, its, res = fields_of(b), b.iterations(), b.residual()
    for m, (case, tol, every) in enumerate(members):
        ks, us, state = vc.until_steps(case, tol, every)
        assert tuple(its[m]) == (ks[-1], sum(ks)), f"member {m} ({tag(case)}): iterations {its[m]}, the rule's {ks}"
        assert_report_equal(res[m], us[-1], f"member {m} ({tag(case)}): the norm")
        for name, g, w in zip(NAMES, got, state):
            assert_bit_equal(g[m], w, f"member {m} ({tag(case)}) {name}")


UNTIL_CONTEXTS = {"sketch": vc.UNTIL_SKETCH, "general": vc.UNTIL_GENERAL, "masked": vc.UNTIL_MASKED}


@pytest.mark.parametrize("which", list(UNTIL_CONTEXTS))
def test_a_context_stops_at_the_rules_iteration(sfl, which):
    """Solver.poisson_solve_until on 61 x 81 (one workgroup), 130 x 70 (the general kernels) and 130 x 70 with a disc."""
    for u in UNTIL_CONTEXTS[which]:
        vc.until_guard(u)
        k, want_p, norm = vc.until_answer(u)
        with sfl.Solver(u.dim_x, u.dim_y) as s:
            if u.mask is not None:
                s.set_solids(mask_of(u.mask, u.dim_x, u.dim_y))
            s.upload(FDIV, vc.until_rhs(u))
            got_k, got_u = s.poisson_solve_until(1.0, u.cap, u.omega, tol=u.tol, every=u.every)
            p, again = s.download(FP), s.residual(1.0)
        print(u, "k", got_k, "want", k, "norm", got_u, "want", norm)
        assert got_k == k, f"{u}: {got_k} iterations, the rule's {k} (on a flushed norm {vc.until_answer(u, True)[0]})"
        assert_report_equal(got_u, norm, f"{u}: the norm")
        assert_report_equal(again, norm, f"{u}: residual()")
        assert_bit_equal(p, want_p, f"{u}: the pressure at k = {k}")


# ---- contexts ----------------------------------------------------------------------------------------------------------------
CONTEXT_OPTIONS = {
    "plain-61x81": [{}],
    "plain-130x70": [{"OPT_SMALL_GRID": 0, "OPT_ADVECT_KERNEL": 1}, {"OPT_SMALL_GRID": 0, "OPT_ADVECT_KERNEL": 2}],
    "plain-160x128": [{}],
    "plain-300x141": [{"OPT_STEP_SEAMS": 1}, {"OPT_STEP_SEAMS": 0}],
}


@pytest.mark.parametrize("what", list(CONTEXT_CASES))
def test_contexts_step_by_the_oracle(sfl, what):
    """Three steps of every texture in one step_n call: the one-launch step (61 x 81), the general kernels with either
    advection (130 x 70), the tiled advections (160 x 128), with and without step seams (300 x 141), the masked solve of
    one and of three launches, and the viscous step with and without a mask."""
    for case in CONTEXT_CASES[what]:
        want = vc.expected(case)[-1]
        for options in CONTEXT_OPTIONS.get(what, [{}]):
            with sfl.Solver(case.dim_x, case.dim_y) as s:
                for name, value in options.items():
                    s.set_option(getattr(sfl.capi, name), value)
                if case.mask is not None:
                    s.set_solids(vc.solid_of(case))
                if case.nu:
                    s.set_viscosity(case.nu, case.sweeps)
                load_context(s, case)
                s.step_n(vc.STEPS, case.dt, case.dx, case.iters, case.omega)
                s.synchronize()
                if case.mask is not None:
                    assert s.last_solve_info()["launches"] == -(-case.iters // SOLID_D)
                for name, g, w in zip(NAMES, fields_of(s), want):
                    assert_bit_equal(g, w, f"{what} {options} ({tag(case)}) {name}")


@pytest.mark.parametrize("mask", [None, "disc"])
@pytest.mark.parametrize("sweeps", [vc.SWEEPS, 9])
def test_diffuse_velocity(sfl, sweeps, mask):
    """The diffusion as an operator of its own, of one launch and of two."""
    dim_x, dim_y = 130, 70
    for name, amplitude in vc.context_textures(dim_x, dim_y, False, mask is not None):
        v, want = vc.diffusion_answer(name, amplitude, dim_x, dim_y, sweeps, mask)
        with sfl.Solver(dim_x, dim_y) as s:
            if mask is not None:
                s.set_solids(mask_of(mask, dim_x, dim_y))
            s.upload(FV, v)
            s.diffuse_velocity(vc.NU, vc.DT, vc.DX, sweeps)
            assert_bit_equal(s.download(FV), want, f"{name} {amplitude}: {sweeps} sweeps, mask {mask}")


@pytest.mark.parametrize("mask", [None, "disc"])
def test_the_operators_one_by_one(sfl, mask):
    """calculate_divergence, poisson_solve and subtract_gradient at 130 x 70 and dx 0.37, each against the oracle's or the
    solids' rule's on what the one before left."""
    dim_x, dim_y = 130, 70
    for name, amplitude in vc.context_textures(dim_x, dim_y, False, mask is not None):
        for k, (v, d, p, w) in enumerate(vc.operator_answers(name, amplitude, dim_x, dim_y, mask)):
            what = f"{name} {amplitude} velocity {k}, mask {mask}"
            with sfl.Solver(dim_x, dim_y) as s:
                if mask is not None:
                    s.set_solids(mask_of(mask, dim_x, dim_y))
                s.upload(FV, v)
                s.calculate_divergence(vc.DX)
                assert_bit_equal(s.download(FDIV), d, f"{what}: calculate_divergence")
                s.poisson_solve(vc.DX, vc.ITERS, vc.OMEGA)
                assert_bit_equal(s.download(FP), p, f"{what}: poisson_solve")
                want_norm = update_norm(p, d, vc.DX) if mask is None else solid_rule.update_norm(p, d, mask_of(mask, dim_x, dim_y), vc.DX)
                assert_report_equal(s.residual(vc.DX), want_norm, f"{what}: residual")
                s.subtract_gradient(vc.DX)
                assert_bit_equal(s.download(FV), w, f"{what}: subtract_gradient")


# ---- readers on these fields -------------------------------------------------------------------------------------------------
def flushed_copy(state):
    """(v, dye, p) of a result and of its flushed copy."""
    v, _, p, c = state
    return (v, c, p), (vc.flushed(v), c, vc.flushed(p))


def assert_denormal_distance(want, what):
    for name in ("max_abs_dvx", "max_abs_dvy", "max_abs_dp"):
        assert 0 < want[name] < vc.TINY, f"{what}: the expected {name} {want[name]!r} is no denormal"
    assert want["velocity_cells_differ"] > 0 and want["pressure_cells_differ"] > 0 and want["dye_cells_differ"] == 0, what


def test_distances_to_a_flushed_copy(sfl):
    """Solver.distance (130 x 70) and BatchSolver.distance (61 x 81, pairwise) between a result and its flushed copy: the
    maxima are themselves denormals, the counts the numbers of denormal cells."""
    for case in CONTEXT_CASES["plain-130x70"]:
        if case.name == "zeros":
            continue
        a, b = flushed_copy(vc.expected(case)[-1])
        want = distance_yardstick(a, b)
        assert_denormal_distance(want, tag(case))
        with sfl.Solver(case.dim_x, case.dim_y) as s, sfl.Solver(case.dim_x, case.dim_y) as t:
            for x, held in ((s, a), (t, b)):
                for field, array in zip((FV, FC, FP), held):
                    x.upload(field, array)
            assert_distance(s.distance(t), want, f"context {tag(case)}")
            assert_distance(t.distance(s), distance_yardstick(b, a), f"context {tag(case)}, the other way round")
    cases = [c for c in vc.batch_cases(61, 81) if c.name in ("quiescent", "tiny")]
    pairs = [flushed_copy(vc.expected(c)[-1]) for c in cases]
    with sfl.BatchSolver(61, 81, len(cases)) as s, sfl.BatchSolver(61, 81, len(cases)) as t:
        for x, side in ((s, 0), (t, 1)):
            for k, field in enumerate((FV, FC, FP)):
                x.upload(field, np.stack([pair[side][k] for pair in pairs]))
        got = s.distance(ref=t)
        for m, (a, b) in enumerate(pairs):
            want = distance_yardstick(a, b)
            assert_denormal_distance(want, f"member {m}")
            assert_distance(got[m], want, f"batch member {m} ({tag(cases[m])})")


def test_distance_between_zeros_of_both_signs(sfl):
    """A +-0 field against its all-+0.0f copy: max |a - b| is +0.0f, and the cells that differ are those that hold a -0.0f."""
    for dim_x, dim_y, batch in ((130, 70, False), (61, 81, True)):
        t = vc.texture("zeros", dim_x, dim_y)
        p = np.where(t.rhs == 0, t.rhs, F(0.0)).astype(F)      # the +-0 of the right-hand side without its spike
        a, b = (t.v, t.dye, p), (np.zeros_like(t.v), t.dye, np.zeros_like(p))
        want = distance_yardstick(a, b)
        assert want["pressure_cells_differ"] == vc.negative_zeros(p) > 0
        assert want["velocity_cells_differ"] == int(np.signbit(t.v).any(axis=-1).sum()) > 0
        for name in ("max_abs_dvx", "max_abs_dvy", "max_abs_dp"):
            assert F(want[name]).view(np.uint32) == 0, "+0.0f"
        make = (lambda: sfl.BatchSolver(dim_x, dim_y, 1)) if batch else (lambda: sfl.Solver(dim_x, dim_y))
        with make() as s, make() as o:
            for x, held in ((s, a), (o, b)):
                for field, array in zip((FV, FC, FP), held):
                    x.upload(field, array[None] if batch else array)
            got = s.distance(ref=o)[0] if batch else s.distance(o)
            assert_distance(got, want, f"zeros {dim_x}x{dim_y}")
            for name in ("max_abs_dvx", "max_abs_dvy", "max_abs_dp"):
                assert F(got[name]).view(np.uint32) == 0, f"{name}: +0.0f, got {got[name]!r}"


@pytest.mark.parametrize("dim_x,dim_y,large", [(61, 81, False), (96, 96, True)], ids=["61x81", "96x96-large"])
def test_a_history_beside_the_steps(sfl, dim_x, dim_y, large):
    """A history with every = 1 beside step_n_each: each record is what flow_stats and residual return after that step on a
    twin stepped one step at a time, the fields are the rules', and the figures recorded are themselves denormals."""
    cases = vc.batch_cases(dim_x, dim_y, each=True)
    prm = params_of(sfl, cases)
    with sfl.BatchSolver(dim_x, dim_y, len(cases), large=large) as b, sfl.BatchSolver(dim_x, dim_y, len(cases), large=large) as twin:
        load_batch(b, cases)
        load_batch(twin, cases)
        b.history_start(1, vc.STEPS)
        b.step_n_each(vc.STEPS, prm)
        records = b.history()
        assert records.shape == (vc.STEPS, len(cases))
        assert_members(fields_of(b), cases, "with a history on")
        for step in range(vc.STEPS):
            twin.step_n_each(1, prm)
            stats, norms = twin.flow_stats(prm["dx"]), twin.residual()
            for m, case in enumerate(cases):
                rec, what = records[step, m], f"step {step}, member {m} ({tag(case)})"
                v, d, p, _ = vc.expected(case)[step]
                for name in ("max_abs_vx", "max_abs_vy", "max_abs_div"):
                    assert_report_equal(rec[name], stats[m][name], f"{what}: {name}")
                assert_report_equal(rec["max_abs_vx"], np.abs(v[..., 0]).max(), f"{what}: max |v.x| of the rule's field")
                assert_report_equal(rec["max_abs_vy"], np.abs(v[..., 1]).max(), f"{what}: max |v.y| of the rule's field")
                assert rec["dye_sum"].tolist() == stats[m]["dye_sum"].tolist(), what
                assert_report_equal(rec["update_norm"], norms[m], f"{what}: update_norm")
                assert_report_equal(rec["update_norm"], update_norm(p, d, case.dx), f"{what}: the update norm of the rule's fields")
                assert (int(rec["iterations"]), int(rec["step"])) == (case.iters, step + 1), what
                assert_report_equal(rec["dt"], F(case.dt), f"{what}: dt")
                assert_report_equal(rec["dx"], F(case.dx), f"{what}: dx")
                if case.name == "tiny":
                    assert 0 < update_norm(p, d, case.dx) < vc.TINY, f"{what}: the update norm to be recorded is a denormal"


def test_tracers_follow_and_sample(sfl):
    """64 tracers that follow the three steps, then sample_tracers of the velocity, the pressure and the divergence: on a
    context of 130 x 70 and on the small batch, against tests/tracer_rule.py."""
    for case in CONTEXT_CASES["plain-130x70"]:
        start, xy, samples = vc.tracer_answer(case)
        with sfl.Solver(case.dim_x, case.dim_y) as s:
            load_context(s, case)
            s.set_tracers(start, follow=True)
            s.step_n(vc.STEPS, case.dt, case.dx, case.iters, case.omega)
            assert_same(s.tracers(), xy, f"context {tag(case)}: the positions")
            for field, want in zip((FV, FP, FDIV), samples):
                assert_same(s.sample_tracers(field, False), want, f"context {tag(case)}: field {field}")
            for name, g, w in zip(NAMES, fields_of(s), vc.expected(case)[-1]):
                assert_bit_equal(g, w, f"context {tag(case)} with tracers: {name}")
    cases = vc.batch_cases(61, 81)
    answers = [vc.tracer_answer(c) for c in cases]
    with sfl.BatchSolver(61, 81, len(cases)) as b:
        load_batch(b, cases)
        b.set_tracers(np.stack([a[0] for a in answers]), follow=True)
        b.step_n(vc.STEPS, vc.DT, vc.DX, vc.ITERS, vc.OMEGA)
        got = b.tracers()
        sampled = [b.sample_tracers(field, False) for field in (FV, FP, FDIV)]
        assert_members(fields_of(b), cases, "with tracers")
    for m, (_, xy, samples) in enumerate(answers):
        assert_same(got[m], xy, f"member {m} ({tag(cases[m])}): the positions")
        for k, want in enumerate(samples):
            assert_same(sampled[k][m], want, f"member {m} ({tag(cases[m])}): sample {k}")
