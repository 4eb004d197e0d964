"""Denormal, quiescent and signed-zero fields, the CPU side: the guards of tests/value_cases.py on every case that
tests/test_values_gpu.py steps; the oracle pinned to the compiled reference on these textures; the rules' anchors on them;
and the liveness of every case that claims denormals -- a yardstick whose intermediate fields, or whose norm, are flushed must
give other bits, or stop elsewhere, than the real one.  The tile cores of the masked solve and of the diffusion run on these
textures in tests/test_context_solids.py and tests/test_viscosity.py.  Every comparison is bit for bit."""
import numpy as np
import pytest

import solid_rule
import value_cases as vc
import viscosity_rule
from conftest import assert_bit_equal
from test_batch_until import oracle_step, rule, sor_iteration
from test_solids_gpu import mask_of

F = np.float32
NAMES = ("velocity", "divergence", "pressure", "colour")
PIN_SHAPES = [(2, 2), (7, 9), (61, 81), (130, 70)]
EVERY_AMPLITUDE = sorted({a for viscous in (False, True) for masked in (False, True) for a in vc.amplitudes(viscous, masked)})
ALL_CASES = vc.all_cases()
UNTILS = [u for group in vc.UNTIL_CLASSES.values() for u in group]


def case_id(c):
    return "-".join(str(x) for x in c if x is not None and x is not False)


# ---- the helpers and numpy itself ----------------------------------------------------------------------------------------
def test_numpy_does_not_flush_and_the_helpers_count_what_they_say():
    assert vc.numpy_keeps_denormals()
    a = np.array([0.0, -0.0, 1e-39, -1e-45, vc.TINY, -vc.TINY, 1.0, np.nan], F)
    assert (vc.denormals(a), vc.negative_zeros(a), vc.positive_zeros(a)) == (2, 1, 1)
    got = vc.flushed(a)
    assert_bit_equal(got[:7], np.array([0.0, -0.0, 0.0, -0.0, vc.TINY, -vc.TINY, 1.0], F), "flushed")
    assert np.isnan(got[7]) and vc.denormals(got) == 0 and vc.negative_zeros(got) == 2


def test_the_textures_are_what_they_are_called():
    for dim_x, dim_y in PIN_SHAPES:
        for a in EVERY_AMPLITUDE:
            t = vc.texture("quiescent", dim_x, dim_y, a)
            assert not t.v.any() and len(t.forces) == 2 and t.forces[1][:2] == (1, 1) and t.forces[0][:2] == (dim_x // 2, dim_y // 2)
            assert all(abs(f) >= vc.TINY for rec in t.forces for f in rec[2:]), "the records themselves are normal numbers"
            assert np.count_nonzero(t.rhs) in (2, 7, 8) and abs(float(t.rhs.astype(np.float64).sum())) < 1e-6 * a
        t = vc.texture("tiny", dim_x, dim_y)
        assert vc.denormals(t.v) >= 1 and vc.denormals(t.rhs) >= 1 and np.abs(t.v).max() <= F(40) * vc.SCALE
        t = vc.texture("zeros", dim_x, dim_y)
        assert not t.v.any() and np.count_nonzero(t.rhs) == 1
        if dim_x * dim_y >= 63:
            assert vc.negative_zeros(t.v) and vc.positive_zeros(t.v) and vc.negative_zeros(t.rhs) and vc.positive_zeros(t.rhs)
        for name in ("tiny", "zeros", "dense"):
            dye = vc.texture(name, dim_x, dim_y).dye
            assert dye.dtype == np.uint32 and dye.max() < 0xFF000000 and (dim_x * dim_y < 63 or dye.max() >= 2 ** 31)


# ---- the guards, for every case the GPU file steps -----------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=case_id)
def test_the_guard_of_every_case_the_gpu_file_steps(case):
    print(case, vc.guard(case))


def test_the_cases_cover_every_shape_and_rule_with_every_texture():
    names = {(c.name, c.dim_x, c.dim_y, c.mask is not None, c.nu != 0) for c in ALL_CASES}
    for shape in ((61, 81), (96, 64), (96, 96), (128, 128), (130, 70), (160, 128), (300, 141)):
        for name in ("quiescent", "tiny", "zeros"):
            assert (name, *shape, False, False) in names, (name, shape)
    for masked, viscous in ((True, False), (False, True), (True, True)):
        assert ("quiescent", 61, 81, masked, viscous) in names and ("tiny", 7, 9, masked, viscous) in names
    assert not any(c.name == "quiescent" and c.dim_x * c.dim_y < vc.SKETCH for c in ALL_CASES)
    assert {c.amplitude for c in ALL_CASES if c.name == "quiescent" and c.nu} == set(vc.AMPLITUDES)


def test_the_signed_zeros_are_where_the_rules_put_them(oracle):
    dim_x, dim_y = 61, 81
    t = vc.texture("zeros", dim_x, dim_y)
    u = oracle.advect_vec2f(t.v, t.v, F(vc.DT), True)
    print("advected velocity: -0.0f", vc.negative_zeros(u), "+0.0f", vc.positive_zeros(u))
    assert vc.negative_zeros(u) >= 1 and vc.positive_zeros(u) >= 1 and not u.any()
    for i, j, fx, fy in t.forces:
        u[j, i] = (fx, fy)
    d = oracle.divergence(u, F(vc.DX))
    p = oracle.poisson_solve(d, F(vc.DX), 4, F(vc.OMEGA))
    masked = solid_rule.divergence(u, mask_of("disc", dim_x, dim_y), vc.DX)
    print("-0.0f in d", vc.negative_zeros(d), "in p after four iterations", vc.negative_zeros(p), "in the masked d", vc.negative_zeros(masked))
    assert vc.negative_zeros(d) >= 1 and vc.negative_zeros(p) >= 1 and vc.negative_zeros(masked) >= 1
    for solid in (None, mask_of("disc", dim_x, dim_y)):
        w = viscosity_rule.diffuse(t.v, vc.NU, vc.DT, vc.DX, vc.SWEEPS, solid)
        fluid = np.ones((dim_y, dim_x), bool) if solid is None else ~solid
        assert vc.negative_zeros(w[fluid]) == 0 and vc.positive_zeros(w[fluid]) == 2 * fluid.sum(), "a diffusion leaves +0.0f alone"


# ---- the oracle is pinned to the compiled reference on these textures ---------------------------------------------------
def pin(oracle, reference, name, amplitude=None):
    for dim_x, dim_y in PIN_SHAPES:
        t = vc.texture(name, dim_x, dim_y, amplitude)
        what = f"{name} {amplitude} {dim_x}x{dim_y}"
        case = vc.Case(name, amplitude, dim_x, dim_y)
        held = [(t.v, t.dye, t.rhs)] + [(s[0], s[3], s[2]) for s in vc.rule_steps(case)]   # the start and every step's fields
        for k, (v, c, scalar) in enumerate(held):
            for no_slip in (True, False):
                assert_bit_equal(oracle.advect_vec2f(v, v, F(vc.DT), no_slip), reference.advect_vec2f(v, v, F(vc.DT), no_slip), f"{what} [{k}]: advect_vec2f")
                assert_bit_equal(oracle.advect_vec3uq32(c, v, F(vc.DT), no_slip), reference.advect_vec3uq32(c, v, F(vc.DT), no_slip), f"{what} [{k}]: advect_vec3uq32")
            for dx in (F(vc.DX), F(1.0)):
                assert_bit_equal(oracle.divergence(v, dx), reference.divergence(v, dx), f"{what} [{k}]: divergence")
                assert_bit_equal(oracle.subtract_gradient(v, scalar, dx), reference.subtract_gradient(v, scalar, dx), f"{what} [{k}]: gradient")
                for rhs in (t.rhs, oracle.divergence(v, dx)):
                    for iters in (6, 40):
                        assert_bit_equal(oracle.poisson_solve(rhs, dx, iters, F(vc.OMEGA)), reference.poisson_solve(rhs, dx, iters, F(vc.OMEGA)),
                                         f"{what} [{k}]: poisson_solve x {iters}")
            got, want = oracle.step(v, c, F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA)), reference.step(v, c, F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA))
            for field, g, w in zip(NAMES, got, want):
                assert_bit_equal(g, w, f"{what} [{k}]: a whole step, {field}")
        # ... and the three forced steps composed from the reference's own operators
        so, sr = (t.v, None, None, t.dye), (t.v, None, None, t.dye)
        for k in range(vc.STEPS):
            so = viscosity_rule.step(oracle, so[0], so[3], F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA), forces=vc.forces_of(case, k))
            sr = viscosity_rule.step(reference, sr[0], sr[3], F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA), forces=vc.forces_of(case, k))
            for field, g, w in zip(NAMES, so, sr):
                assert_bit_equal(g, w, f"{what}: forced step {k}, {field}")


@pytest.mark.parametrize("amplitude", EVERY_AMPLITUDE)
def test_the_oracle_is_the_reference_on_the_quiescent_texture(oracle, reference, amplitude):
    pin(oracle, reference, "quiescent", amplitude)


def test_the_oracle_is_the_reference_on_the_tiny_texture(oracle, reference):
    pin(oracle, reference, "tiny")


def test_the_oracle_is_the_reference_on_the_signed_zeros(oracle, reference):
    pin(oracle, reference, "zeros")


# ---- the rules' anchors on these textures ----------------------------------------------------------------------------------
ANCHORS = [("quiescent", a) for a in EVERY_AMPLITUDE] + [("tiny", None), ("zeros", None)]


@pytest.mark.parametrize("name,amplitude", ANCHORS)
@pytest.mark.parametrize("dim_x,dim_y", [(7, 9), (61, 81), (130, 70)])
def test_the_rules_without_a_mask_and_without_viscosity_are_the_oracles_step(oracle, dim_x, dim_y, name, amplitude):
    t = vc.texture(name, dim_x, dim_y, amplitude)
    case = vc.Case(name, amplitude, dim_x, dim_y)
    empty = np.zeros((dim_y, dim_x), bool)
    state = (t.v, None, None, t.dye)
    for k in range(vc.STEPS):
        forces = vc.forces_of(case, k)
        args = (state[0], state[3], F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA))
        want = oracle_step(oracle, *args, [((i, j), (fx, fy)) for i, j, fx, fy in forces])
        if not forces:
            for field, g, w in zip(NAMES, oracle.step(*args), want):
                assert_bit_equal(g, w, f"step {k}: the composed step against the oracle's own, {field}")
        solids = solid_rule.step(oracle, state[0], state[3], empty, F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA), forces)
        viscous = viscosity_rule.step(oracle, *args, nu=0.0, sweeps=vc.SWEEPS, forces=forces)
        for field, s, v, w in zip(NAMES, solids, viscous, want):
            assert_bit_equal(s, w, f"step {k}: solid_rule.step with an empty mask, {field}")
            assert_bit_equal(v, w, f"step {k}: viscosity_rule.step with nu = 0, {field}")
        state = want
    for field, g, w in zip(NAMES, vc.rule_steps(case)[-1], state):
        assert_bit_equal(g, w, f"value_cases.rule_steps, {field}")
    # with a mask and nu = 0 the viscous rule is the solids' rule
    disc = mask_of("disc", dim_x, dim_y)
    got = viscosity_rule.step(oracle, t.v, t.dye, F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA), 0.0, vc.SWEEPS, disc, t.forces)
    for field, g, w in zip(NAMES, got, solid_rule.step(oracle, t.v, t.dye, disc, F(vc.DT), F(vc.DX), vc.ITERS, F(vc.OMEGA), t.forces)):
        assert_bit_equal(g, w, f"viscosity_rule.step with nu = 0 and a disc, {field}")


@pytest.mark.parametrize("name,amplitude", ANCHORS)
def test_the_numpy_iteration_is_the_oracles_on_these_right_hand_sides(oracle, name, amplitude):
    for dim_x, dim_y in ((7, 9), (61, 81)):
        d = vc.texture(name, dim_x, dim_y, amplitude).rhs
        empty = np.zeros((dim_y, dim_x), bool)
        for dx, omega in ((1.0, 1.5), (vc.DX, vc.OMEGA)):
            p = np.zeros_like(d)
            for k in range(1, 13):
                want = oracle.sor_iterate(p, d, F(dx), 1, F(omega))
                got = sor_iteration(p, d, dx, omega)
                if name == "zeros":   # gs_target seeds its sum with +0.0f, so 0 + x loses the sign of a zero (solid_rule.py seeds with
                    # -0.0f for that reason): equal as numbers, and no test here reads a sign from it -- the stopping rule takes |.|
                    assert np.array_equal(got, want) and not np.isnan(want).any(), f"{dim_x}x{dim_y} dx {dx}: sor_iteration {k}"
                else:
                    assert_bit_equal(got, want, f"{dim_x}x{dim_y} dx {dx}: sor_iteration {k}")
                assert_bit_equal(solid_rule.iterate(p, d, empty, dx, 1, omega), want, f"{dim_x}x{dim_y} dx {dx}: solid_rule.iterate {k}")
                p = want
            assert_bit_equal(p, oracle.poisson_solve(d, F(dx), 12, F(omega)), "twelve iterations are the solve")


@pytest.mark.parametrize("u", UNTILS, ids=case_id)
def test_the_stopping_rule_restated_here_is_the_batches(oracle, u):
    d = vc.until_rhs(u)
    k, p, norm = vc.until_answer(u)
    if u.mask is None:
        wk, wp, wn = rule(d, 1.0, u.cap, u.omega, u.tol, u.every)
        assert k == wk and norm.view(np.uint32) == F(wn).view(np.uint32)
        assert_bit_equal(p, wp, "the pressure of test_batch_until.rule")
        assert_bit_equal(p, oracle.poisson_solve(d, F(1.0), k, F(u.omega)), f"the oracle's pressure at k = {k}")
    else:
        solid = mask_of(u.mask, u.dim_x, u.dim_y)
        assert_bit_equal(p, solid_rule.solve(d, solid, 1.0, k, u.omega), f"solid_rule.solve at k = {k}")
        assert norm.view(np.uint32) == F(solid_rule.update_norm(p, d, solid, 1.0)).view(np.uint32)
        empty = vc.until(d, 1.0, 12, u.omega, u.tol, u.every, np.zeros_like(solid))    # an empty mask: the plain rule
        plain = rule(d, 1.0, 12, u.omega, u.tol, u.every)
        assert empty[0] == plain[0] and empty[2].view(np.uint32) == F(plain[2]).view(np.uint32)
        assert_bit_equal(empty[1], plain[1], "an empty mask")


# ---- liveness: a flush anywhere shows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in ALL_CASES if c.name in ("quiescent", "tiny")], ids=case_id)
def test_steps_from_a_flushed_velocity_leave_other_bits(case):
    real, other = vc.rule_steps(case)[-1], vc.rule_steps(case, flush=True)[-1]
    differ = [int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))) for a, b in zip(real, other)]
    print(case, "words that differ in (v, d, p, dye):", differ)
    assert min(differ[:3]) >= 1, f"{case}: a velocity flushed between the steps goes unseen: {differ}"


@pytest.mark.parametrize("name,amplitude", [("quiescent", 1e-38), ("quiescent", 3e-39), ("tiny", None)])
def test_a_flush_between_iterations_or_sweeps_leaves_other_bits(oracle, name, amplitude):
    dim_x, dim_y = 61, 81
    t = vc.texture(name, dim_x, dim_y, amplitude)
    for solid in (None, mask_of("disc", dim_x, dim_y)):
        p = q = np.zeros_like(t.rhs)
        for _ in range(vc.ITERS):
            step = (lambda x: sor_iteration(x, t.rhs, vc.DX, vc.OMEGA)) if solid is None else (lambda x: solid_rule.iterate(x, t.rhs, solid, vc.DX, 1, vc.OMEGA))
            p, q = step(p), vc.flushed(step(q))
        assert vc.denormals(p) >= 30 and (p != q).any(), "a solve flushed between its iterations goes unseen"
        v = np.array(t.v)
        for i, j, fx, fy in t.forces:
            v[j, i] = (fx, fy)
        if solid is not None:
            v[solid] = 0.0
        real = viscosity_rule.diffuse(v, vc.NU, vc.DT, vc.DX, vc.SWEEPS, solid)
        a, c = viscosity_rule.coefficients(vc.NU, vc.DT, vc.DX)
        other = v
        for _ in range(vc.SWEEPS):
            for colour in (0, 1):
                other = vc.flushed(viscosity_rule.sweep_colour(other, v, a, c, colour, solid))
        assert vc.denormals(real) >= 30 and (real != other).any(), "a diffusion flushed between its sweeps goes unseen"


@pytest.mark.parametrize("u", UNTILS, ids=case_id)
def test_a_flushed_norm_stops_the_solve_elsewhere(u):
    k, kf = vc.until_guard(u)
    want = [c for c, group in vc.UNTIL_CLASSES.items() if u in group]
    print(u, "the rule stops at", k, vc.until_answer(u)[2], "on a flushed norm at", kf)
    assert [vc.until_class(u)] == want
    if want == ["early"]:
        assert 0 < k < u.cap and k % u.every == 0 and vc.until_answer(u)[2] <= F(u.tol)
    else:
        assert k == u.cap and (u.cap - kf <= 12 or u.dim_x * u.dim_y < vc.SKETCH), "the cap lies just above the flushed k"
    assert 0 < vc.until_answer(u)[2] < vc.TINY, "the norm the rule ends with is a denormal"


@pytest.mark.parametrize("dim_x,dim_y,large", vc.UNTIL_STEP_SHAPES)
def test_the_stopped_steps_are_stopped_by_denormal_norms(dim_x, dim_y, large):
    for case, tol, every in vc.until_step_members(dim_x, dim_y):
        print(case, tol, every, vc.until_step_guard(case, tol, every))


# ---- what the readers' and the operators' tests of the GPU file compare with holds what it claims -----------------------------
def test_the_operators_diffusions_tracers_and_distances_hold_what_they_claim():
    dim_x, dim_y = 130, 70
    for mask in (None, "disc"):
        for name, amplitude in vc.context_textures(dim_x, dim_y, False, mask is not None):
            print(name, amplitude, mask, [(vc.denormals(d), vc.denormals(p)) for _, d, p, _ in vc.operator_answers(name, amplitude, dim_x, dim_y, mask)])
            one, two = (vc.diffusion_answer(name, amplitude, dim_x, dim_y, sweeps, mask)[1] for sweeps in (vc.SWEEPS, 9))
            assert name == "zeros" or (one != two).any(), "nine sweeps are not three"
    for case in vc.context_cases()["plain-130x70"] + vc.batch_cases(61, 81):
        _, xy, samples = vc.tracer_answer(case)
        print(case, "denormal samples of (v, p, d):", [vc.denormals(s) for s in samples])
        v, _, p, _ = vc.expected(case)[-1]
        if case.name in ("quiescent", "tiny"):   # the distance to a flushed copy is the largest denormal the field holds
            for a in (v[..., 0], v[..., 1], p):
                assert 0 < np.abs(a - vc.flushed(a)).max() < vc.TINY and vc.denormals(a) >= 100
