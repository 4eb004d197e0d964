"""Batches whose members stop their pressure solve at a tolerance (sfl_batch_step_n_until, sfl_batch_poisson_solve_until)
and the iteration counts they leave (sfl_batch_iterations).

The contract under test (include/sfl.h, sfl_member_stop): member m runs its solve until the first checkpoint k in {0,
every, 2 every, ...}, k < cap, whose update norm u_k is <= tol or a NaN, else to the cap; it is left with, bit for bit,
the reference's poisson_solve(d, dx, k, omega); residual()[m] is u_k of that pressure and iterations()[m] is k.  The
yardstick is a numpy restatement of that rule (`rule` below) built on gs_target / update_norm of test_batch_params.py,
itself pinned against the oracle by a CPU test.  All comparisons are bit for bit; a NaN is matched by any NaN.

Right-hand sides are zero-mean (d - d.mean() of seeded standard normals) or real divergences of a step: under the
all-Neumann stencil a right-hand side with a mean never converges -- its update norm plateaus -- and every member would
hit its cap.  Each GPU test first asserts ON THE YARDSTICK ALONE that its members fall into the classes it is about:
early (0 < k < cap), cap (k = cap > 0), zero (k = 0) and NaN (stopped by a NaN)."""
import ctypes as C
import re

import numpy as np
import pytest

import test_batch_params as bp
from conftest import assert_bit_equal
from test_batch_params import BATCH_SHAPES, DTS, DXS, FIELDS, OMEGAS, assert_report_equal, gs_target, update_norm

UNTIL_SYMBOLS = ["sfl_batch_step_n_until", "sfl_batch_poisson_solve_until", "sfl_batch_iterations"]
# the parameter points of the GPU tests are drawn from these (and DTS, DXS, OMEGAS) with a fixed seed
CAPS, TOLS, EVERYS = (0, 1, 33, 120, 300), (0.1, 1e-2, 1e-3, -1.0, np.inf), (1, 4, 7)


# ---- the yardstick: numpy restatement of the rule -----------------------------------------------------
def sor_iteration(p, d, dx, omega):
    """One red-black iteration, numpy_sor's update (test_batch_params.py)."""
    f = np.float32
    jj, ii = np.indices(d.shape)
    with np.errstate(all="ignore"):
        for colour in (0, 1):
            g = gs_target(p, d, dx)
            p = np.where(((ii + jj) & 1) == colour, (f(1) - f(omega)) * p + f(omega) * g, p).astype(np.float32)
    return p


def rule(d, dx, cap, omega, tol, every):
    """-> (k, the pressure of exactly k iterations from zero, u_k): the stopping rule of include/sfl.h."""
    tol, p, k = np.float32(tol), np.zeros_like(d), 0
    while k < cap:
        if k % every == 0:
            u = np.float32(update_norm(p, d, dx))
            if tol >= 0 and (u <= tol or np.isnan(u)):     # IEEE float comparison; a negative tol stops nothing
                return k, p, u
        p = sor_iteration(p, d, dx, omega)
        k += 1
    return k, p, np.float32(update_norm(p, d, dx))


def classify(k, cap, u):
    return "zero" if k == 0 else "nan" if (k < cap and np.isnan(u)) else "early" if k < cap else "cap"


def zero_mean(dim_x, dim_y, seed):
    d = np.random.default_rng(seed).standard_normal((dim_y, dim_x))
    return (d - d.mean()).astype(np.float32)


def oracle_step(oracle, v, c, dt, dx, iters, omega, forces=()):
    """One sim step composed from the oracle's operators (ino:252-287 order) so that forces fit in between; without
    forces it IS oracle.step (pinned below).  Returns (v, div, p, colour)."""
    va = oracle.advect_vec2f(v, v, np.float32(dt), True)
    for (i, j), vel in forces:                              # queue order: the last write wins; outside cells are skipped
        if 0 <= i < v.shape[1] and 0 <= j < v.shape[0]:
            va[j, i] = vel
    div = oracle.divergence(va, np.float32(dx))
    with np.errstate(all="ignore"):
        p = oracle.poisson_solve(div, np.float32(dx), int(iters), np.float32(omega))
    vn = oracle.subtract_gradient(va, p, np.float32(dx))
    return vn, div, p, oracle.advect_vec3uq32(c, vn, np.float32(dt), False)


def yardstick_step(oracle, v, c, prm, stop, forces=()):
    """The step by the rule: its divergence from a step of no iterations, k from the rule, the state from a step of k."""
    div = oracle_step(oracle, v, c, prm["dt"], prm["dx"], 0, prm["omega"], forces)[1]
    k, _, u = rule(div, prm["dx"], int(prm["iters"]), prm["omega"], stop["tol"], int(stop["every"]))
    return k, u, oracle_step(oracle, v, c, prm["dt"], prm["dx"], k, prm["omega"], forces)


# ---- CPU ----------------------------------------------------------------------------------------------
def test_the_three_symbols_are_exported_and_bound(sfl):
    lib = sfl.capi.lib()
    for name in UNTIL_SYMBOLS:
        assert hasattr(lib, name), name
        assert name in sfl.capi.SIGNATURES, name
        assert getattr(lib, name).argtypes == sfl.capi.SIGNATURES[name][1]
    for name in ("step_n_until", "poisson_solve_until", "iterations"):
        assert hasattr(sfl.BatchSolver, name), name


def test_member_stop_is_eight_bytes(sfl):
    ms = sfl.capi.MemberStop
    assert C.sizeof(ms) == 8
    assert [(n, getattr(ms, n).offset) for n, _ in ms._fields_] == [("tol", 0), ("every", 4)]


def test_a_null_batch_is_refused_by_all_three(sfl):
    lib = sfl.capi.lib()
    prm, stops, out = (sfl.capi.MemberParams * 2)(), (sfl.capi.MemberStop * 2)(), (C.c_int32 * 4)()
    for call in (lambda: lib.sfl_batch_step_n_until(None, 1, prm, stops),
                 lambda: lib.sfl_batch_poisson_solve_until(None, prm, stops),
                 lambda: lib.sfl_batch_iterations(None, 0, 2, out, 16)):
        assert call() == sfl.capi.ERR_INVALID
        assert "NULL" in lib.sfl_last_error().decode()


def test_member_stops_broadcasts_into_the_c_layout(sfl):
    want = np.dtype([("tol", "<f4"), ("every", "<i4")])
    a = sfl.member_stops(5, 1e-3)                                    # a scalar (and the default) broadcast
    assert a.dtype == want and a.dtype.itemsize == 8 and a.shape == (5,) and a.flags["C_CONTIGUOUS"]
    assert [a.dtype.fields[n][1] for n in ("tol", "every")] == [0, 4]
    assert np.all(a["tol"] == np.float32(1e-3)) and np.all(a["every"] == 4)
    b = sfl.member_stops(3, [0.1, -1.0, np.inf], [1, 4, 7])          # sequences kept
    assert_bit_equal(b["tol"], np.array([0.1, -1.0, np.inf], np.float32))
    assert b["every"].tolist() == [1, 4, 7]
    c = sfl.member_stops(4, 1e-2, every=np.arange(1, 5))             # mixed
    assert np.all(c["tol"] == np.float32(1e-2)) and c["every"].tolist() == [1, 2, 3, 4]
    assert c.tobytes() == b"".join(bytes(sfl.capi.MemberStop(r["tol"], r["every"])) for r in c)
    for bad in (dict(tol=[0.1, 0.2]), dict(tol=0.1, every=[1, 2, 3, 4, 5]), dict(tol=[]), dict(tol=np.ones((3, 1)))):
        with pytest.raises(ValueError):
            sfl.member_stops(3, **bad)


@pytest.mark.parametrize("dim_x,dim_y,dx,cap,omega,tol,every,what", [
    (61, 81, 1.0, 400, 1.9, 1e-2, 1, "early"), (61, 81, 1.0, 400, 1.9, 1e-2, 7, "early"),
    (61, 81, 0.5, 400, 1.96, 1e-3, 4, "early"), (61, 81, 1.0, 60, 1.0, 1e-3, 4, "cap"),
    (3, 3, 1.0, 400, 1.9, 1e-2, 4, "early"), (2, 2, 2.0, 400, 1.96, 1e-3, 7, "early"),
    (257, 23, 1.0, 50, 1.9, 1e-2, 1, "cap"), (61, 81, 1.0, 33, 1.9, -1.0, 1, "cap"),
    (61, 81, 1.0, 33, 1.9, np.inf, 4, "zero"), (61, 81, 1.0, 0, 1.9, 1e-2, 4, "zero")])
def test_the_yardstick_leaves_the_oracles_pressure_of_the_k_it_finds(oracle, dim_x, dim_y, dx, cap, omega, tol, every, what):
    """The pressure the numpy rule stops with IS the oracle's poisson_solve at the k it reports, bit for bit; its norm is
    update_norm of that pressure; k is the rule's: a checkpoint below the cap that passes while no earlier one did."""
    d = zero_mean(dim_x, dim_y, 3 + dim_x)
    k, p, u = rule(d, dx, cap, omega, tol, every)
    assert classify(k, cap, u) == what, (k, u)
    assert_bit_equal(p, oracle.poisson_solve(d, np.float32(dx), k, np.float32(omega)), f"the rule's pressure at k = {k}")
    assert_report_equal(u, update_norm(p, d, dx), "the rule's norm")
    if k < cap:
        assert k % every == 0 and u <= np.float32(tol)
    norms = [np.float32(update_norm(oracle.poisson_solve(d, np.float32(dx), j, np.float32(omega)), d, dx))
             for j in range(0, min(k, cap), every)]
    assert all(not n <= np.float32(tol) for n in norms), "an earlier checkpoint already passed"


def test_the_yardstick_sees_a_diverging_member_at_its_first_nan_checkpoint(oracle):
    d = np.random.default_rng(3 + 61).standard_normal((81, 61)).astype(np.float32)     # NOT zero-mean, omega 2.5
    found = {}
    for every in (1, 4, 7):
        k, p, u = rule(d, 1.0, 300, 2.5, 1e-3, every)
        assert classify(k, 300, u) == "nan" and k % every == 0, (every, k, u)
        found[every] = k
        with np.errstate(all="ignore"):
            before = update_norm(oracle.poisson_solve(d, 1.0, k - every, np.float32(2.5)), d, 1.0)
        assert not np.isnan(before) and before > 1e-3, "the checkpoint before must not have stopped it"
    assert found[1] <= found[4] < found[1] + 4 and found[1] <= found[7] < found[1] + 7
    k, _, u = rule(d, 1.0, 300, 2.5, -1.0, 4)
    assert k == 300 and np.isnan(u), "a negative tol runs a diverged member to its cap"


def test_the_composed_step_is_the_oracles_step(oracle):
    v, c, _ = bp.member_fields(61, 81, 77, 40.0)
    for iters in (0, 9):
        got, want = oracle_step(oracle, v, c, 1 / 30.0, 0.5, iters, 1.9), oracle.step(v, c, 1 / 30.0, 0.5, iters, 1.9)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(got[k], want[k], f"{name}, {iters} iterations")


# ---- GPU ----------------------------------------------------------------------------------------------
def draw_params(sfl, batch, seed):
    rng = np.random.default_rng(seed)
    pick = lambda values: [values[k] for k in rng.integers(0, len(values), batch)]
    prm = sfl.member_params(batch, pick(DTS), pick(DXS), pick(CAPS), pick(OMEGAS))
    return prm, sfl.member_stops(batch, pick(TOLS), pick(EVERYS))


def assert_counts_and_reports(b, ks, sums, got_d, got_p, prm, what):
    its, res = b.iterations(), b.residual()
    assert its.dtype == np.int32 and its.shape == (len(prm), 2) and res.shape == (len(prm),)
    for m in range(len(prm)):
        assert (its[m, 0], its[m, 1]) == (ks[m], sums[m]), f"{what}, member {m} ({prm[m]}): iterations {its[m]}, want {ks[m], sums[m]}"
        assert_report_equal(res[m], update_norm(got_p[m], got_d[m], prm["dx"][m]), f"{what}, member {m} ({prm[m]})")


# what the drawn members of a batch of 37 are, per shape, on the yardstick (a CPU run of `rule`; asserted before the GPU
# is asked anything): thin and long shapes never reach 1e-2 within 300 iterations
SOLVE_CLASSES_37 = {(2, 2): {"early", "cap", "zero"}, (3, 3): {"early", "cap", "zero"}, (61, 81): {"early", "cap", "zero"},
                    (80, 60): {"early", "cap", "zero"}, (78, 78): {"early", "cap", "zero"}, (128, 48): {"early", "cap", "zero"},
                    (257, 23): {"early", "cap", "zero"}, (2047, 3): {"cap", "zero"}, (2, 3072): {"cap", "zero"}}


@pytest.mark.gpu
@pytest.mark.parametrize("dim_x,dim_y", BATCH_SHAPES)
@pytest.mark.parametrize("batch", [1, 3, 37])
def test_every_member_equals_the_oracle_at_the_yardsticks_own_k(sfl, oracle, dim_x, dim_y, batch):
    fields = [bp.member_fields(dim_x, dim_y, 2000 * batch + 11 * m + dim_x) for m in range(batch)]
    d = [zero_mean(dim_x, dim_y, 3000 * batch + 13 * m + dim_x) for m in range(batch)]
    prm, stops = draw_params(sfl, batch, 100 * batch + dim_x)
    want = [rule(d[m], prm["dx"][m], int(prm["iters"][m]), prm["omega"][m], stops["tol"][m], int(stops["every"][m]))
            for m in range(batch)]
    classes = {classify(k, int(prm["iters"][m]), u) for m, (k, _, u) in enumerate(want)}
    print(f"{dim_x} x {dim_y} x {batch}: k = {[w[0] for w in want]}, classes {sorted(classes)}")
    if batch == 37:
        assert SOLVE_CLASSES_37[(dim_x, dim_y)] <= classes, classes
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        bp.upload_members(b, fields)
        b.upload(2, np.stack(d))
        b.poisson_solve_until(prm["dx"], prm["iters"], prm["omega"], stops["tol"], stops["every"])
        p = b.download(3)
        for m, (k, _, _) in enumerate(want):
            assert_bit_equal(p[m], oracle.poisson_solve(d[m], prm["dx"][m], k, prm["omega"][m]),
                             f"solve, member {m} ({prm[m]}, {stops[m]}) at k = {k}")
        ks = [w[0] for w in want]
        assert_counts_and_reports(b, ks, ks, b.download(2), p, prm, "after poisson_solve_until")
        b.step_n_until(1, prm, tol=stops)            # ready-made arrays
        got = bp.download_all(b)
        steps = [yardstick_step(oracle, v, c, prm[m], stops[m]) for m, (v, c, _) in enumerate(fields)]
        for m, (k, _, state) in enumerate(steps):
            for f, name in enumerate(FIELDS):
                assert_bit_equal(got[f][m], state[f], f"{name}, member {m} ({prm[m]}, {stops[m]}) at k = {k}")
        ks = [s[0] for s in steps]
        assert_counts_and_reports(b, ks, ks, got[1], got[2], prm, "after step_n_until")


@pytest.mark.gpu
def test_three_steps_with_forces_follow_the_rule_step_by_step(sfl, oracle):
    dim_x, dim_y, batch = 61, 81, 257
    fields = [bp.member_fields(dim_x, dim_y, 5000 + m, 40.0) for m in range(batch)]
    prm, stops = draw_params(sfl, batch, 257)
    state = [(v, None, None, c) for v, c, _ in fields]
    last, total, seen = [0] * batch, [0] * batch, set()
    for step in range(3):                                          # the yardstick goes step by step
        for m in range(batch):
            forces = bp.FORCES_257.get(m, ()) if step == 0 else ()
            k, u, state[m] = yardstick_step(oracle, state[m][0], state[m][3], prm[m], stops[m], forces)
            last[m], total[m] = k, total[m] + k
            seen.add(classify(k, int(prm["iters"][m]), u))
    print("classes over the three steps:", sorted(seen), "sum of iterations", sum(total))
    assert {"early", "cap", "zero"} <= seen
    assert any(total[m] != 3 * last[m] for m in range(batch)), "some member's count must change from step to step"
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        bp.upload_members(b, fields)
        bp.queue_257(b)
        b.step_n_until(3, prm["dt"], prm["dx"], prm["iters"], prm["omega"], stops["tol"], stops["every"])
        got = bp.download_all(b)
        for m in range(batch):
            for f, name in enumerate(FIELDS):
                assert_bit_equal(got[f][m], state[m][f], f"{name}, member {m} ({prm[m]}, {stops[m]})")
        assert_counts_and_reports(b, last, total, got[1], got[2], prm, "after three steps")


@pytest.mark.gpu
def test_a_negative_tol_for_every_member_is_the_each_call(sfl):
    dim_x, dim_y, batch = 61, 81, 19
    fields = [bp.member_fields(dim_x, dim_y, 7000 + m, 40.0) for m in range(batch)]
    forces = ([0, 7, 7, 18], [(30, 40), (5, 5), (5, 5), (60, 80)], [(55.0, -35.0), (1.0, 2.0), (-3.0, 4.0), (9.0, 9.0)])
    prm = bp.draw_params(sfl, batch, 19)
    every = [(1, 4, 7)[m % 3] for m in range(batch)]
    with sfl.BatchSolver(dim_x, dim_y, batch) as until, sfl.BatchSolver(dim_x, dim_y, batch) as each:
        for b in (until, each):
            bp.upload_members(b, fields)
            b.queue_forces(*forces)
        until.step_n_until(3, prm, tol=-1.0, every=every)
        each.step_n_each(3, prm)
        got, want = bp.download_all(until), bp.download_all(each)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(got[k], want[k], f"{name}: step_n_until with tol = -1 against step_n_each")
        assert_bit_equal(until.residual(), each.residual(), "the report")
        assert until.iterations().tolist() == [[int(q), 3 * int(q)] for q in prm["iters"]]
        for b in (until, each):
            b.upload(2, np.stack([f[2] for f in fields]))          # (not zero-mean: nothing here converges anyway)
        until.poisson_solve_until(prm, tol=-1.0, every=every)
        each.poisson_solve_each(prm)
        assert_bit_equal(until.download(3), each.download(3), "pressure: poisson_solve_until with tol = -1")
        assert_bit_equal(until.residual(), each.residual(), "the report after the solve")
        assert until.iterations().tolist() == [[int(q), int(q)] for q in prm["iters"]]


@pytest.mark.gpu
def test_a_diverging_member_stops_at_its_first_nan_and_leaves_its_neighbours_alone(sfl, oracle):
    dim_x, dim_y, cap = 61, 81, 300
    rng = np.random.default_rng(8)
    # (omega, tol, every, zero-mean rhs?) -- members 0, 2, 4, 6 are the healthy neighbours; 5 diverges and never stops
    cases = [(1.9, 1e-2, 4, True), (2.5, 1e-3, 1, False), (1.96, 1e-3, 7, True), (2.5, 1e-3, 4, False),
             (1.9, 1e-3, 1, True), (2.5, -1.0, 4, False), (1.0, 1e-3, 4, True), (2.5, 1e-2, 7, False)]
    batch = len(cases)
    d = np.stack([zero_mean(dim_x, dim_y, 40 + m) if c[3] else rng.standard_normal((dim_y, dim_x)).astype(np.float32)
                  for m, c in enumerate(cases)])
    want = [rule(d[m], 1.0, cap, c[0], c[1], c[2]) for m, c in enumerate(cases)]
    classes = [classify(k, cap, u) for k, _, u in want]
    print("k:", [w[0] for w in want], classes)
    assert classes == ["early", "nan", "early", "nan", "early", "cap", "cap", "nan"]
    assert np.isnan(want[5][2]), "the member that never stops reports the NaN of its cap"
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.upload(2, d)
        b.poisson_solve_until(1.0, cap, [c[0] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
        p, res, its = b.download(3), b.residual(), b.iterations()
    print("update norms:", res, "iterations:", its[:, 0])
    for m, (k, wp, u) in enumerate(want):
        assert tuple(its[m]) == (k, k), f"member {m} {cases[m]}: iterations {its[m]}, the yardstick's {k}"
        if classes[m] in ("nan", "cap") and cases[m][0] == 2.5:
            assert np.isnan(res[m]), f"member {m}: a diverged member reports a NaN, got {res[m]!r}"
        else:
            assert_bit_equal(p[m], oracle.poisson_solve(d[m], 1.0, k, np.float32(cases[m][0])), f"pressure, member {m} {cases[m]}")
        if np.all(np.isfinite(wp)):
            assert_bit_equal(p[m], wp, f"pressure against the rule's, member {m}")
        assert_report_equal(res[m], update_norm(p[m], d[m], 1.0), f"member {m} {cases[m]}")


@pytest.mark.gpu
def test_when_the_iterations_are_valid_and_what_is_refused(sfl):
    dim_x, dim_y, batch = 61, 81, 8
    fields = [bp.member_fields(dim_x, dim_y, 9000 + m, 40.0) for m in range(batch)]
    prm, stops = draw_params(sfl, batch, 9)
    lib, cap = sfl.capi.lib(), sfl.capi
    pp = lambda a: a.ctypes.data_as(C.POINTER(cap.MemberParams))
    sp = lambda a: a.ctypes.data_as(C.POINTER(cap.MemberStop))

    def stale(b):
        with pytest.raises(sfl.SflError) as e:
            b.iterations()
        assert e.value.code == cap.ERR_STATE
        assert "_until" in str(e.value)      # the message says which call to make

    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        stale(b)                                                   # a fresh batch
        bp.upload_members(b, fields)
        b.step_n_until(0, prm, tol=stops)            # n == 0 launches nothing: still nothing to report
        stale(b)
        with pytest.raises(sfl.SflError):
            b.residual()
        b.step_n_until(1, prm, tol=stops)
        first, first_res = b.iterations(), b.residual()
        assert np.all(first[:, 0] == first[:, 1]) and np.all(first[:, 0] <= prm["iters"])
        b.step_n_until(0, prm, tol=stops)            # ... and leaves the reports as they were
        assert b.iterations().tolist() == first.tolist()
        assert_bit_equal(b.residual(), first_res, "the update norm after n == 0")
        b.step_n_each(1, prm)                                      # an *_each call: a norm, no iterations
        stale(b)
        b.residual()
        b.poisson_solve_until(prm, tol=stops)
        its = b.iterations()
        b.step_n(1, 1 / 30.0, 1.0, 5, 1.96)
        stale(b)
        b.poisson_solve_until(prm, tol=stops)
        b.poisson_solve(1.0, 5, 1.96)
        stale(b)
        b.poisson_solve_until(prm, tol=stops)
        b.poisson_solve_each(prm)
        stale(b)
        b.poisson_solve_until(prm, tol=stops)
        b.upload(3, np.zeros((1, dim_y, dim_x), np.float32), first=2)   # an upload of the pressure
        stale(b)
        b.poisson_solve_until(prm, tol=stops)
        b.upload(2, fields[0][2][None])                            # ... or of the divergence
        stale(b)
        b.poisson_solve_until(prm, tol=stops)
        b.upload(0, fields[0][0][None])                            # velocity and dye are not what the counts are about
        its = b.iterations()
        # ranges and byte counts as residual checks them
        assert b.iterations(3, 2).tolist() == its[3:5].tolist()
        assert b.iterations(batch, 0).shape == (0, 2)
        out = (C.c_int32 * (2 * batch + 2))()
        h = b._h
        for args in ((-1, 1, 8), (0, batch + 1, 8 * (batch + 1)), (batch - 1, 2, 16), (0, -1, 0), (0, 2, 8), (0, 2, 24)):
            assert lib.sfl_batch_iterations(h, args[0], args[1], out, args[2]) == cap.ERR_INVALID, args
        assert lib.sfl_batch_iterations(h, 0, 2, None, 16) == cap.ERR_INVALID
        assert lib.sfl_batch_step_n_until(h, 1, None, sp(stops)) == cap.ERR_INVALID and "NULL" in lib.sfl_last_error().decode()
        assert lib.sfl_batch_step_n_until(h, 1, pp(prm), None) == cap.ERR_INVALID and "NULL" in lib.sfl_last_error().decode()
        assert lib.sfl_batch_poisson_solve_until(h, None, sp(stops)) == cap.ERR_INVALID
        assert lib.sfl_batch_poisson_solve_until(h, pp(prm), None) == cap.ERR_INVALID
        assert lib.sfl_batch_step_n_until(h, -1, pp(prm), sp(stops)) == cap.ERR_INVALID
        assert b.iterations().tolist() == its.tolist(), "the counts survive refused calls"
        # every = 0, a NaN tol, iters = -1: refused, naming the first such member; every field and the force queue untouched
        bp.upload_members(b, fields)
        b.queue_forces([5, 2], [(30, 40), (7, 9)], [(50.0, -20.0), (4.0, 4.0)])
        before = bp.download_all(b)
        bad_every, bad_tol, bad_iters, bad_all = stops.copy(), stops.copy(), prm.copy(), stops.copy()
        bad_every["every"][3], bad_every["every"][6] = 0, -2
        bad_tol["tol"][4] = np.nan
        bad_iters["iters"][5], bad_iters["iters"][6] = -1, -7
        bad_all["every"][7], bad_all["tol"][6] = 0, np.nan
        for p_, s_, member in ((prm, bad_every, 3), (prm, bad_tol, 4), (bad_iters, stops, 5), (bad_iters, bad_all, 5)):
            for call in (lambda: b.step_n_until(1, p_, tol=s_), lambda: b.poisson_solve_until(p_, tol=s_),
                         lambda: b.step_n_until(0, p_, tol=s_)):
                with pytest.raises(sfl.SflError) as e:
                    call()
                assert e.value.code == cap.ERR_INVALID and re.search(rf"member {member}\b", str(e.value)), str(e.value)
        after = bp.download_all(b)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(after[k], before[k], f"{name} after refused calls")
        b.step_n_until(1, prm, tol=-1.0, every=4)         # looks unforced, applies the forces queued before
        got = bp.download_all(b)
        with sfl.BatchSolver(dim_x, dim_y, batch) as e:            # (tol = -1 is step_n_each: the test above)
            for f, a in zip((0, 2, 3, 1), before):
                e.upload(f, a)
            e.queue_forces([5, 2], [(30, 40), (7, 9)], [(50.0, -20.0), (4.0, 4.0)])
            e.step_n_each(1, prm)
            want = bp.download_all(e)
        for k, name in enumerate(FIELDS):
            assert_bit_equal(got[k], want[k], f"{name} after a refused call: the queued forces were kept")
        assert not np.array_equal(got[0][5], before[0][5])
        with pytest.raises(ValueError):
            b.step_n_until(1, prm[:4], tol=stops)    # ready-made arrays of another batch's length
        with pytest.raises(ValueError):
            b.step_n_until(1, prm, tol=stops[:4])


@pytest.mark.gpu
def test_stops_and_counts_of_members_beyond_four_gigabytes_of_one_field(sfl, oracle):
    """61 x 81 x 73000 members: the dye alone is 4.33 GB (> 2^32 bytes).  Members 0 and B - 1 get stop records of their own."""
    dim_x, dim_y, batch = 61, 81, 73000
    assert batch * dim_x * dim_y * 12 > 2 ** 32
    forces = {0: [((30, 40), (40.0, -25.0))], batch - 1: [((12, 70), (-33.0, 18.0)), ((13, 70), (5.0, 5.0))]}
    prm = sfl.member_params(batch, 1 / 30.0, 1.0, 20, 1.96)
    stops = sfl.member_stops(batch, 1e-3, 4)
    for m, (dt, dx, iters, omega, tol, every) in ((0, (1 / 60.0, 0.5, 300, 1.9, 1e-2, 7)), (batch - 1, (0.1, 2.0, 120, 1.5, 0.1, 1))):
        prm["dt"][m], prm["dx"][m], prm["iters"][m], prm["omega"][m] = dt, dx, iters, omega
        stops["tol"][m], stops["every"][m] = tol, every
    v0, c0 = oracle.setup_fields(dim_x, dim_y)
    checked = (0, 1, batch - 2, batch - 1)
    want = {m: yardstick_step(oracle, v0, c0, prm[m], stops[m], forces.get(m, ())) for m in checked}
    print({m: (w[0], w[1]) for m, w in want.items()})
    assert [classify(want[m][0], int(prm["iters"][m]), want[m][1]) for m in checked] == ["early", "zero", "zero", "early"]
    with sfl.BatchSolver(dim_x, dim_y, batch) as b:
        b.setup_sketch_fields()
        for m, fs in forces.items():
            b.queue_forces([m] * len(fs), [f[0] for f in fs], [f[1] for f in fs])
        b.step_n_until(1, prm, tol=stops)
        got = {m: [b.download(f, m, 1)[0] for f in (0, 2, 3, 1)] for m in checked}
        tail_res, head_res = b.residual(batch - 2, 2), b.residual(0, 2)
        tail_its, head_its = b.iterations(batch - 2, 2), b.iterations(0, 2)
    for m, res, its in ((0, head_res[0], head_its[0]), (1, head_res[1], head_its[1]),
                        (batch - 2, tail_res[0], tail_its[0]), (batch - 1, tail_res[1], tail_its[1])):
        k, _, state = want[m]
        assert tuple(its) == (k, k), f"member {m}: iterations {its}, the yardstick's {k}"
        assert_report_equal(res, update_norm(got[m][2], got[m][1], prm["dx"][m]), f"member {m}")
        for f, name in enumerate(FIELDS[:3]):
            assert_bit_equal(got[m][f], state[f], f"{name}, member {m}")
    assert tail_res[1] > 0 and head_res[0] > 0                # the forced members have something to report
    # The sketch's start holds saturated dye (UINT32_MAX), outside the range in which the oracle's narrowing is defined
    # (include/sfl.h, sfl_setup_sketch_fields: it saturates here, the checker's x86 conversion wraps to 0).  So the dye,
    # and the other three fields once more, are held against a context that runs the yardstick's k iterations, as
    # test_batch_params.py does for this batch.
    with sfl.Solver(dim_x, dim_y) as s:
        for m, fields in got.items():
            s.setup_sketch_fields()
            if m in forces:
                s.queue_forces(np.array([f[0] for f in forces[m]], np.int32), np.array([f[1] for f in forces[m]], np.float32))
            s.step_n(1, prm["dt"][m], prm["dx"][m], want[m][0], prm["omega"][m])
            s.synchronize()
            for f, name in enumerate(FIELDS):
                assert_bit_equal(fields[f], s.download((0, 2, 3, 1)[f]), f"{name}, member {m} against a context")
