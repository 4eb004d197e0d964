"""Openings on the rim of a batch member's grid, the CPU side (include/sfl.h "OPENINGS"): the rule as tests/opening_rule.py
restates it, anchored on tests/solid_rule.py (no opening: the solids' bits); the fixed point of a uniform channel flow and the
disc run of the issue's prototype; the five calls as the binding sees them; every refusal that needs no device; and the host
unit (csrc/openings.cpp and its hooks in the step, solve, statistics, history, view, viscosity and solids calls) run through
by tests/cpp/openings_driver.cpp over a runtime that lives on the host.  tests/test_openings_gpu.py has the kernels."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import opening_rule as rule
import solid_rule
from conftest import ROOT, assert_bit_equal, random_fields
from test_context_solids import D, TX, TY
from test_solids import ring, seeded_mask
from test_solids_gpu import mask_of

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 7, 1.9
FOUR = ("sfl_set_openings", "sfl_set_inflow", "sfl_openings_info", "sfl_openings_download")
FIVE = ("sfl_batch_set_openings", "sfl_batch_set_inflow", "sfl_batch_openings_info", "sfl_batch_openings_download", "sfl_batch_inflow_download")


def tunnel(dim_x, dim_y):
    """West column inflow, east column outflow, the corners closed."""
    m = np.zeros((dim_y, dim_x), np.uint8)
    m[1:-1, 0] = rule.INFLOW
    m[1:-1, -1] = rule.OUTFLOW
    return m


def channel_walls(dim_x, dim_y):
    s = np.zeros((dim_y, dim_x), bool)
    s[0] = s[-1] = True
    return s


# ---- the anchor: no opening gives the solids' bits -----------------------------------------------------------------------
def masks_for(dim_x, dim_y):
    return {"none": np.zeros((dim_y, dim_x), bool), "ring": ring(dim_x - 2, dim_y - 2), "seeded": seeded_mask(dim_x, dim_y, 5),
            "disc": mask_of("disc", dim_x, dim_y), "channel": mask_of("channel", dim_x, dim_y)}


@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (33, 18), (61, 81)])
def test_with_an_all_zero_map_the_rule_is_the_solids_rule_bit_for_bit(oracle, dim_x, dim_y):
    v, c, s = random_fields(dim_x, dim_y, 11, vamp=40.0)
    none = np.zeros((dim_y, dim_x), np.uint8)
    for name, solid in masks_for(dim_x, dim_y).items():
        assert_bit_equal(rule.divergence(v, solid, none, DX), solid_rule.divergence(v, solid, DX), f"divergence {name}")
        p = solid_rule.solve(s, solid, DX, 3, OMEGA)
        assert_bit_equal(rule.iterate(p, s, solid, none, DX, 4, OMEGA), solid_rule.iterate(p, s, solid, DX, 4, OMEGA), f"iterate {name}")
        assert rule.update_norm(p, s, solid, none, DX).view(np.uint32) == solid_rule.update_norm(p, s, solid, DX).view(np.uint32), name
        assert_bit_equal(rule.gradient(v, p, solid, none, DX), solid_rule.gradient(v, p, solid, DX), f"gradient {name}")
        forces = [(2, 2, 3.0, -2.0), (0, 1, 5.0, 6.0)]
        got = rule.step(oracle, v, c, solid, none, (9.0, 9.0), DT, DX, ITERS, OMEGA, forces)
        want = solid_rule.step(oracle, v, c, solid, DT, DX, ITERS, OMEGA, forces)
        for field, a, b in zip(("velocity", "divergence", "pressure", "colour"), got, want):
            assert_bit_equal(a, b, f"step {name}: {field}")


def test_an_opening_on_a_solid_cell_does_not_count(oracle):
    dim_x, dim_y = 9, 7
    v, c, _ = random_fields(dim_x, dim_y, 3, vamp=10.0)
    solid = np.zeros((dim_y, dim_x), bool)
    solid[:, 0] = solid[:, -1] = True
    got = rule.step(oracle, v, c, solid, tunnel(dim_x, dim_y), (4.0, 1.0), DT, DX, ITERS, OMEGA)
    want = solid_rule.step(oracle, v, c, solid, DT, DX, ITERS, OMEGA)
    for a, b in zip(got, want):
        assert_bit_equal(a, b, "every opening lies on a solid cell")
    assert not rule.inflow_cells(tunnel(dim_x, dim_y), solid).any()


# ---- the fixed point: a uniform flow passes through an open channel ------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(7, 9), (61, 41), (61, 81)])
def test_a_uniform_flow_in_an_open_channel_is_a_fixed_point_bit_for_bit(dim_x, dim_y):
    U = np.float32(3.5)
    solid, open = channel_walls(dim_x, dim_y), tunnel(dim_x, dim_y)
    v = np.zeros((dim_y, dim_x, 2), np.float32)
    v[~solid, 0] = U
    d = rule.divergence(v, solid, open, 1.0)
    assert not d.view(np.uint32).any(), "the divergence is +0.0f in every cell"
    p = rule.solve(d, solid, open, 1.0, 5, 1.9)
    assert not (p.view(np.uint32) & 0x7FFFFFFF).any(), "five iterations leave p = 0"
    assert_bit_equal(rule.gradient(v, p, solid, open, 1.0), v, "the gradient leaves every velocity bit")
    closed = solid_rule.divergence(v, solid, 1.0)
    assert np.abs(closed).max() == U, "the closed rule sees a wall at both ends"


# ---- the disc run of the prototype ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(61, 41), (61, 81)])
def test_a_disc_in_the_open_channel_converges_and_passes_the_flux(oracle, dim_x, dim_y):
    """Six steps at dt = 0 from rest, 200 iterations each at omega 1.9: the update norm of successive 40-iteration blocks falls
    within every step, and after the sixth step at least 0.98 of the flux that enters leaves (the prototype: 0.989)."""
    solid = channel_walls(dim_x, dim_y)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    solid |= (i - dim_x // 4) ** 2 + (j - dim_y // 2) ** 2 <= (dim_y // 8) ** 2
    open, inflow = tunnel(dim_x, dim_y), (3.5, 0.0)
    v = np.zeros((dim_y, dim_x, 2), np.float32)
    for step in range(6):
        u = v.copy()
        u[rule.inflow_cells(open, solid)] = inflow
        u[solid] = 0.0
        d = rule.divergence(u, solid, open, 1.0)
        p, norms = np.zeros((dim_y, dim_x), np.float32), []
        for _ in range(5):
            p = rule.iterate(p, d, solid, open, 1.0, 40, 1.9)
            norms.append(float(rule.update_norm(p, d, solid, open, 1.0)))
        assert all(b < a for a, b in zip(norms, norms[1:])), (step, norms)
        v = rule.gradient(u, p, solid, open, 1.0)
    into, out = rule.flux(v, open, solid)
    assert into > 0 and out / into >= 0.98, (into, out, out / into)
    assert out / into < 1.02


# ---- the map's checks, restated ------------------------------------------------------------------------------------------
def test_the_rules_own_check_of_a_map():
    m = np.zeros((5, 7), np.uint8)
    assert rule.check_map(m) is None and rule.check_map(tunnel(7, 5)) is None
    for (j, i), v in (((0, 0), 1), ((4, 6), 2), ((2, 3), 1), ((0, 3), 3)):
        bad = m.copy()
        bad[j, i] = v
        assert rule.check_map(bad) == (i, j)


# ---- the binding and the header ------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pb, pf, pl = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_float), C.POINTER(C.c_int64)
    want = {"sfl_batch_set_openings": [vp, pb, i, pf, i], "sfl_batch_set_inflow": [vp, pf, i], "sfl_batch_openings_info": [vp, pi, pi, pi, pl, pl],
            "sfl_batch_openings_download": [vp, i, i, pb, sz], "sfl_batch_inflow_download": [vp, i, i, pf, sz]}
    want.update({"sfl_set_openings": [vp, pb, C.c_float, C.c_float], "sfl_set_inflow": [vp, C.c_float, C.c_float],
                 "sfl_openings_info": [vp, pi, pf, pf, pl, pl], "sfl_openings_download": [vp, pb, sz]})
    assert set(want) == set(FIVE + FOUR)
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for line in ("SFL_API int sfl_batch_set_openings(sfl_batch *b, const uint8_t *open, int per_member, const float *inflow, int inflow_per_member);",
                 "SFL_API int sfl_batch_set_inflow(sfl_batch *b, const float *inflow, int per_member);",
                 "SFL_API int sfl_batch_openings_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes);",
                 "SFL_API int sfl_batch_inflow_download(sfl_batch *b, int first, int count, float *host, size_t bytes);",
                 "SFL_API int sfl_set_openings(sfl_context *ctx, const uint8_t *open, float inflow_x, float inflow_y);",
                 "SFL_API int sfl_set_inflow(sfl_context *ctx, float inflow_x, float inflow_y);",
                 "SFL_API int sfl_openings_download(sfl_context *ctx, uint8_t *host, size_t bytes);",
                 "#define SFL_OPEN_INFLOW  1", "#define SFL_OPEN_OUTFLOW 2"):
        assert line in header, line
    assert (sfl.OPEN_INFLOW, sfl.OPEN_OUTFLOW) == (1, 2) == (cap.OPEN_INFLOW, cap.OPEN_OUTFLOW) == (rule.INFLOW, rule.OUTFLOW)
    for name in ("set_openings", "set_inflow", "openings", "openings_info"):
        assert callable(getattr(sfl.BatchSolver, name, None)) and callable(getattr(sfl.Solver, name, None)), name
    assert lib.sfl_abi_version() == 1


def test_the_header_states_the_rule_and_names_the_honoured_and_the_refused_calls():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    start, end = header.index("/* --- OPENINGS:"), header.index("/* A batch is used from one thread at a time")
    assert start > header.index("SFL_API int sfl_batch_viscosity_download("), "the section comes behind the VISCOSITY declarations"
    section = header[start:end]
    for words in ("rim cell\n * that is no corner", "only where the cell is fluid", "2a. inflow", "-own.x for W, +own.x for E, -own.y for S, +own.y for N",
                  "n = present + 1 if the open neighbour is an OUTFLOW", "n = 4: -0.25f", "contributes -0.0f", "update norm uses the same k",
                  "an outflow neighbour's pressure is +0.0f", "An inflow without any outflow is accepted", "the solve drifts",
                  "sfl_batch_step_n and\n * sfl_batch_step_n_each", "sfl_batch_residual", "sfl_batch_solids_info still reports",
                  "sfl_batch_create_large", "sfl_batch_step_n_until", "sfl_batch_history_start", "SFL_VIEW_DIVERGENCE", "sfl_batch_set_viscosity",
                  "argument checks come first", "NOT THERE", "per-cell inflow profile", "flux diagnostic"):
        assert words in section, words
    for name in FIVE:
        assert f"SFL_API int {name}(" in section, name
    # the contexts' section: behind the batches' calls, naming its calls and its refusals, without restating the arithmetic
    ctx = section[section.index("/* --- OPENINGS OF A CONTEXT"):]
    assert section.index("/* --- OPENINGS OF A CONTEXT") > section.index("SFL_API int sfl_batch_inflow_download(")
    for words in ("sfl_step, sfl_step_n", "ONE UNFUSED SEQUENCE", "compact list", "never impose the inflow", "sfl_calculate_divergence, sfl_poisson_solve, sfl_poisson_continue, sfl_subtract_gradient",
                  "sfl_residual, sfl_poisson_solve_until, sfl_flow_stats, sfl_history_*", "k set up from n", 'sfl_solids_info still reports "not set"',
                  "nranks != 1", "transport attached", "sfl_comm_attach", "sfl_group_link", "SFL_VIEW_DIVERGENCE", "sfl_set_viscosity", "argument checks come first"):
        assert words in ctx, words
    assert "n = present + 1" not in ctx, "the arithmetic is stated once, in the section above"
    for name in FOUR:
        assert f"SFL_API int {name}(sfl_context *ctx" in ctx, name
    # the sections in front are still there, each with its first declaration behind it
    for title, call in (("--- SOLIDS:", "sfl_batch_set_solids"), ("--- SOLIDS OF A CONTEXT", "sfl_set_solids"), ("--- LOADS:", "sfl_batch_set_bodies"),
                        ("--- VISCOSITY:", "sfl_set_viscosity")):
        assert header.index(title) < header.index(f"SFL_API int {call}(") < start, title


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    """(A corner cell, an interior cell, a value of 3, a per-member NaN and the downloads' sizes need a handle to be wrong about:
    the host driver below has them.)"""
    lib, cap = sfl.capi.lib(), sfl.capi
    m, w, n = (C.c_uint8 * 12)(), C.c_int(5), C.c_int64(5)
    good, nan, inf = (C.c_float * 2)(1.0, 0.0), (C.c_float * 2)(1.0, float("nan")), (C.c_float * 2)(float("inf"), 0.0)
    refusals = [
        (lambda: lib.sfl_batch_set_openings(None, m, 2, good, 0), "sfl_batch_set_openings: per_member must be 0 or 1 (got 2)"),
        (lambda: lib.sfl_batch_set_openings(None, m, 0, good, -1), "sfl_batch_set_openings: inflow_per_member must be 0 or 1 (got -1)"),
        (lambda: lib.sfl_batch_set_openings(None, m, 0, nan, 0), "sfl_batch_set_openings: the inflow velocity must be finite (member 0: (1, nan))"),
        (lambda: lib.sfl_batch_set_openings(None, m, 0, inf, 0), "sfl_batch_set_openings: the inflow velocity must be finite (member 0: (inf, 0))"),
        (lambda: lib.sfl_batch_set_openings(None, m, 0, good, 0), "sfl_batch_set_openings: batch is NULL"),
        (lambda: lib.sfl_batch_set_openings(None, None, 0, None, 0), "sfl_batch_set_openings: batch is NULL"),
        (lambda: lib.sfl_batch_set_inflow(None, good, 3), "sfl_batch_set_inflow: per_member must be 0 or 1 (got 3)"),
        (lambda: lib.sfl_batch_set_inflow(None, nan, 0), "sfl_batch_set_inflow: the inflow velocity must be finite"),
        (lambda: lib.sfl_batch_set_inflow(None, good, 0), "sfl_batch_set_inflow: batch is NULL"),
        (lambda: lib.sfl_batch_openings_info(None, C.byref(w), C.byref(w), C.byref(w), C.byref(n), C.byref(n)), "sfl_batch_openings_info: batch is NULL"),
        (lambda: lib.sfl_batch_openings_download(None, 0, 1, m, 12), "sfl_batch_openings_download: batch is NULL"),
        (lambda: lib.sfl_batch_inflow_download(None, 0, 1, good, 8), "sfl_batch_inflow_download: batch is NULL"),
        (lambda: lib.sfl_set_openings(None, m, float("nan"), 0.0), "sfl_set_openings: the inflow velocity must be finite (got (nan, 0))"),
        (lambda: lib.sfl_set_openings(None, m, 1.0, float("-inf")), "sfl_set_openings: the inflow velocity must be finite (got (1, -inf))"),
        (lambda: lib.sfl_set_openings(None, m, 1.0, 0.0), "sfl_set_openings: ctx is NULL"),
        (lambda: lib.sfl_set_openings(None, None, float("nan"), 0.0), "sfl_set_openings: ctx is NULL"),
        (lambda: lib.sfl_set_inflow(None, float("nan"), 0.0), "sfl_set_inflow: the inflow velocity must be finite"),
        (lambda: lib.sfl_set_inflow(None, 1.0, 0.0), "sfl_set_inflow: ctx is NULL"),
        (lambda: lib.sfl_openings_info(None, C.byref(w), None, None, C.byref(n), C.byref(n)), "sfl_openings_info: ctx is NULL"),
        (lambda: lib.sfl_openings_download(None, m, 12), "sfl_openings_download: ctx is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert w.value == 5 and n.value == 5


def test_the_python_front_end_checks_shape_and_dtype_before_the_library_sees_the_map(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        Fake().set_openings(np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        Fake().set_openings(np.zeros((3, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        Fake().set_openings(np.zeros((3, 4), bool))
    with pytest.raises(ValueError, match="inflow of shape"):
        Fake().set_openings(np.zeros((3, 4), np.uint8), inflow=(1.0, 2.0, 3.0))
    with pytest.raises(ValueError, match="inflow of shape"):
        Fake().set_inflow(np.zeros((3, 2), np.float32))

    class FakeContext(sfl.Solver):
        def __init__(self):
            self._h, self._lib = None, None
            self.dim_x, self.dim_y = 4, 3

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        FakeContext().set_openings(np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        FakeContext().set_openings(np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="inflow of shape"):
        FakeContext().set_openings(np.zeros((3, 4), np.uint8), inflow=(1.0,))
    with pytest.raises(ValueError, match="inflow of shape"):
        FakeContext().set_inflow((1.0, 2.0, 3.0))


# ---- the host unit and the tile core -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "openings.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(cpp, "openings_driver")


def tiles(tmp_path, dim_x, dim_y, d, cases):
    """The driver's tile mode on (mask kind, map kind, iters) cases of one shape: the pressures, and the masks and maps they were solved with."""
    from test_openings_gpu import map_of, solid_of
    src, dst = tmp_path / "cases.bin", tmp_path / "p.bin"
    with open(src, "wb") as f:
        for mask_kind, map_kind, iters in cases:
            f.write(np.array([dim_x, dim_y, iters], np.int32).tobytes())
            f.write(np.array([DX, OMEGA], np.float32).tobytes())
            f.write(np.ascontiguousarray(d, np.float32).tobytes())
            f.write(solid_of(mask_kind, dim_x, dim_y).astype(np.uint8).tobytes())
            f.write(map_of(map_kind, dim_x, dim_y).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} cases solved tile by tile (TX {TX}, TY {TY}, D {D})" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.float32).reshape(len(cases), dim_y, dim_x)
    return [(got[k], solid_of(m, dim_x, dim_y), map_of(o, dim_x, dim_y)) for k, (m, o, _) in enumerate(cases)]


TILE_SHAPES = [(7, 5), (TX, TY), (TX + 1, TY + 1), (2 * TX + 3, TY - 1), (257, 130)]   # the shapes of tests/test_context_solids.py
TILE_PAIRS = [("none", "west_east"), ("disc", "four"), ("seeded", "out_only"), ("walls", "on_solid"), ("channel", "slot"), ("seeded", "in_only"), ("disc", "empty")]


@pytest.mark.parametrize("dim_x,dim_y", TILE_SHAPES, ids=[f"{x}x{y}" for x, y in TILE_SHAPES])
def test_the_tile_core_run_on_the_host_solves_by_the_rule(tmp_path, dim_x, dim_y):
    """csrc/sor_solid_tile.h with csrc/sor_open_tile.h's set-up of k, tile by tile with the launch segmentation of the host code, at
    shapes that straddle the tile and iteration counts that straddle a launch: the rule's solve bit for bit."""
    d = (random_fields(dim_x, dim_y, 31)[2] * np.float32(7.5)).astype(np.float32)
    cases = [(m, o, iters) for m, o in TILE_PAIRS for iters in (0, 1, D - 1, D, D + 1, 2 * D + 3)]
    for (got, solid, open_map), (m, o, iters) in zip(tiles(tmp_path, dim_x, dim_y, d, cases), cases):
        assert_bit_equal(got, rule.solve(d, solid, open_map, DX, iters, OMEGA), f"{dim_x}x{dim_y} {m} {o} iters {iters}")


VALUE_TEXTURES = [("quiescent", 1e-38), ("tiny", None), ("zeros", None)]


@pytest.mark.parametrize("name,amplitude", VALUE_TEXTURES, ids=[t[0] for t in VALUE_TEXTURES])
@pytest.mark.parametrize("dim_x,dim_y", [(TX + 1, TY + 1), (257, 130)], ids=["one-more-than-a-tile", "257x130"])
def test_the_tile_core_on_right_hand_sides_at_the_bottom_of_the_float_range(tmp_path, dim_x, dim_y, name, amplitude):
    """The quiescent, the tiny and the signed-zero texture of tests/value_cases.py through the same program: the first two keep
    100 denormal cells in the rule's pressure, the third leaves negative zeros in it."""
    import value_cases
    d = value_cases.texture(name, dim_x, dim_y, amplitude).rhs
    cases = [(m, o, iters) for m, o in TILE_PAIRS[:4] for iters in (D - 1, 2 * D + 3)]
    for (got, solid, open_map), (m, o, iters) in zip(tiles(tmp_path, dim_x, dim_y, d, cases), cases):
        want = rule.solve(d, solid, open_map, DX, iters, OMEGA)
        if name == "zeros":
            assert value_cases.negative_zeros(want) >= 1, (m, o, iters)
        else:
            assert value_cases.denormals(want) >= 100, (m, o, iters, value_cases.denormals(want))
        assert_bit_equal(got, want, f"{name} {dim_x}x{dim_y} {m} {o} iters {iters}")


def test_the_host_side_of_the_openings():
    """`make -C tests/cpp -f openings.mk`: tests/cpp/openings_driver.cpp, a stand-alone program (a plain build, no sanitizer).
    The open codes the device is handed for a hand-written map, with and without a mask, in either order of setting; which
    launcher each call picks and with which member stride; the inflow as staged and as changed; clearing restores the old
    launchers; every SFL_ERR_INVALID refusal that needs a handle (a corner, an interior cell, a value of 3, a per-member NaN,
    wrong download sizes) and every SFL_ERR_STATE refusal, each with its message and with nothing staged or launched; the
    solids' code bytes untouched; destroy with openings set leaves no allocation."""
    r = subprocess.run([driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
