"""Viscosity, the CPU side (include/sfl.h "VISCOSITY"): the six calls as the binding sees them; every refusal that needs
no device; the rule itself in numpy (tests/viscosity_rule.py); the tile core of the contexts' diffusion
(csrc/diffuse_tile.h) run on the host by tests/cpp/viscosity_driver.cpp, one workgroup's tile after the other, against the
rule bit for bit -- which checks the halo depth, the shrinking valid region of the temporal blocking and the u0 of a
diffusion of several launches without a GPU; and the host units (csrc/context_viscous.cpp, csrc/viscous.cpp and their
hooks in the step, the batches' step calls and the transports) run through by the same program over a runtime that lives
on the host.  tests/test_viscosity_gpu.py has the kernels."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import value_cases
import viscosity_rule as rule
from conftest import ROOT, assert_bit_equal, random_fields
from test_context_solids import MASKS, mask

CPP = os.path.join(ROOT, "tests", "cpp")
NU, DT, DX = 0.35, 0.04, 0.7
SIX = ("sfl_set_viscosity", "sfl_viscosity_info", "sfl_diffuse_velocity", "sfl_batch_set_viscosity", "sfl_batch_viscosity_info",
       "sfl_batch_viscosity_download")


def tile_shape():
    """TX, TY and D as csrc/diffuse_tile.h states them."""
    text = open(os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "diffuse_tile.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("kTX", "kTY", "kD"))


TX, TY, D = tile_shape()
# smaller than one tile; exactly one; one cell more each way; three tiles wide and one row short of a tile; 5 x 5 ragged tiles
SHAPES = [(7, 5), (TX, TY), (TX + 1, TY + 1), (2 * TX + 3, TY - 1), (257, 130)]
SWEEPS = [0, 1, D - 1, D, D + 1, 2 * D + 3]


# ---- the binding and the header ------------------------------------------------------------------------------------------
def test_the_six_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, sz, i, f, pi, pf = C.c_void_p, C.c_size_t, C.c_int, C.c_float, C.POINTER(C.c_int), C.POINTER(C.c_float)
    want = {"sfl_set_viscosity": [vp, f, i], "sfl_viscosity_info": [vp, pf, pi], "sfl_diffuse_velocity": [vp, f, f, f, i],
            "sfl_batch_set_viscosity": [vp, pf, i, i], "sfl_batch_viscosity_info": [vp, pi, pi, pi],
            "sfl_batch_viscosity_download": [vp, i, i, pf, sz]}
    assert set(want) == set(SIX)
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for line in ("SFL_API int sfl_set_viscosity(sfl_context *ctx, float nu, int sweeps);",
                 "SFL_API int sfl_viscosity_info(sfl_context *ctx, float *nu, int *sweeps);",
                 "SFL_API int sfl_diffuse_velocity(sfl_context *ctx, float nu, float dt, float dx, int sweeps);",
                 "SFL_API int sfl_batch_set_viscosity(sfl_batch *b, const float *nu, int per_member, int sweeps);",
                 "SFL_API int sfl_batch_viscosity_info(sfl_batch *b, int *set, int *per_member, int *sweeps);",
                 "SFL_API int sfl_batch_viscosity_download(sfl_batch *b, int first, int count, float *host, size_t bytes);"):
        assert line in header, line
    for name in ("set_viscosity", "viscosity", "diffuse_velocity"):
        assert callable(getattr(sfl.Solver, name, None)), name
    for name in ("set_viscosity", "viscosity"):
        assert callable(getattr(sfl.BatchSolver, name, None)), name
    assert lib.sfl_abi_version() == 1


def test_the_header_names_the_honoured_and_the_refused_calls_and_leaves_the_other_sections_alone():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    start, end = header.index("/* --- VISCOSITY:"), header.index("/* A batch is used from one thread at a time")
    assert start > header.index("SFL_API int sfl_loads_read("), "the section comes behind the LOADS declarations"
    section = header[start:end]
    for words in ("ITEM 3a OF A STEP", "SKIPPED WHOLE", "nu == 0.0f", "sweeps == 0", "a = (nu * dt) / (dx * dx)", "c = 1.0f / (1.0f + 4.0f * a)",
                  "u.q = (u0.q + a * (((W.q + E.q) + S.q) + N.q)) * c", "OUTSIDE THE DOMAIN contributes -u.q", "SOLID neighbour", "never updated",
                  "(i + j) & 1 == 0", "-ffp-contract=off",
                  "sfl_batch_step_n and sfl_batch_step_n_each", "one launch per step", "render, recorder, envelope, distance, tracers, views",
                  "histories and loads", "sfl_step and sfl_step_n", "ONE UNFUSED", "No step seams", "sfl_diffuse_velocity", "third velocity-sized buffer",
                  "SFL_ERR_NOMEM", "sfl_batch_create_large", "no room for u0", "sfl_batch_step_n_until", "nranks != 1", "transport attached",
                  "sfl_comm_attach, sfl_comm_emulate, sfl_comm_emulate_rccl and sfl_group_link", "argument checks come first",
                  "NOT THERE", "a viscous part of the\n * loads", "diffusion of the dye", "on slabs", "in the _until calls"):
        assert words in section, words
    for name in SIX:
        assert f"SFL_API int {name}(" in section, name
    assert "#define SFL_ABI_VERSION 1" in header
    # every other byte of the header is the parent commit's, where git can show it
    r = subprocess.run(["git", "-C", ROOT, "show", "HEAD:include/sfl.h"], capture_output=True, text=True) if shutil.which("git") else None
    if r is not None and r.returncode == 0 and "--- VISCOSITY:" not in r.stdout:
        assert header[:start] + header[end:] == r.stdout


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    """(Per-member nu, the download's sizes and every SFL_ERR_STATE refusal need a handle to be wrong about: the host driver
    below has them.)"""
    lib, cap = sfl.capi.lib(), sfl.capi
    nu, s, w = C.c_float(5), C.c_int(5), C.c_int(5)
    good, neg, nan = (C.c_float * 1)(0.5), (C.c_float * 1)(-0.5), (C.c_float * 1)(float("nan"))
    refusals = [
        (lambda: lib.sfl_set_viscosity(None, 0.5, 2), "sfl_set_viscosity: ctx is NULL"),
        (lambda: lib.sfl_set_viscosity(None, 0.0, 0), "sfl_set_viscosity: ctx is NULL"),
        (lambda: lib.sfl_set_viscosity(None, -0.5, 2), "sfl_set_viscosity: nu must be >= 0 and not a NaN (got -0.5)"),
        (lambda: lib.sfl_set_viscosity(None, float("nan"), 2), "sfl_set_viscosity: nu must be >= 0 and not a NaN (got nan)"),
        (lambda: lib.sfl_set_viscosity(None, 0.5, -1), "sfl_set_viscosity: sweeps must be >= 0 (got -1)"),
        (lambda: lib.sfl_viscosity_info(None, C.byref(nu), C.byref(s)), "sfl_viscosity_info: ctx is NULL"),
        (lambda: lib.sfl_diffuse_velocity(None, 0.5, 0.1, 1.0, 2), "sfl_diffuse_velocity: ctx is NULL"),
        (lambda: lib.sfl_diffuse_velocity(None, -1.0, 0.1, 1.0, 2), "sfl_diffuse_velocity: nu must be >= 0 and not a NaN (got -1)"),
        (lambda: lib.sfl_diffuse_velocity(None, float("nan"), 0.1, 1.0, 2), "sfl_diffuse_velocity: nu must be >= 0 and not a NaN"),
        (lambda: lib.sfl_diffuse_velocity(None, 0.5, 0.1, 1.0, -2), "sfl_diffuse_velocity: sweeps must be >= 0 (got -2)"),
        (lambda: lib.sfl_batch_set_viscosity(None, good, 0, 2), "sfl_batch_set_viscosity: batch is NULL"),
        (lambda: lib.sfl_batch_set_viscosity(None, None, 0, 0), "sfl_batch_set_viscosity: batch is NULL"),
        (lambda: lib.sfl_batch_set_viscosity(None, good, 2, 2), "sfl_batch_set_viscosity: per_member must be 0 or 1 (got 2)"),
        (lambda: lib.sfl_batch_set_viscosity(None, good, -1, 2), "sfl_batch_set_viscosity: per_member must be 0 or 1 (got -1)"),
        (lambda: lib.sfl_batch_set_viscosity(None, good, 0, -3), "sfl_batch_set_viscosity: sweeps must be >= 0 (got -3)"),
        (lambda: lib.sfl_batch_set_viscosity(None, neg, 0, 2), "sfl_batch_set_viscosity: nu must be >= 0 and not a NaN (got -0.5)"),
        (lambda: lib.sfl_batch_set_viscosity(None, nan, 0, 2), "sfl_batch_set_viscosity: nu must be >= 0 and not a NaN (got nan)"),
        (lambda: lib.sfl_batch_viscosity_info(None, C.byref(s), C.byref(w), None), "sfl_batch_viscosity_info: batch is NULL"),
        (lambda: lib.sfl_batch_viscosity_download(None, 0, 1, good, 4), "sfl_batch_viscosity_download: batch is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert nu.value == 5 and s.value == 5 and w.value == 5


def test_the_python_front_end_checks_the_shape_of_nu_before_the_library_sees_it(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 5

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        Fake().set_viscosity(np.zeros(4, np.float32), 2)
    with pytest.raises(ValueError, match="shape"):
        Fake().set_viscosity(np.zeros((5, 1), np.float32), 2)


# ---- the rule itself -----------------------------------------------------------------------------------------------------
def test_nu_zero_or_no_sweeps_return_the_input_with_its_bits():
    v = random_fields(9, 7, 3)[0]
    v[2, 3] = (-0.0, 0.0)
    v[0, 0] = (-0.0, -0.0)
    for nu, sweeps in ((0.0, 4), (NU, 0), (-0.0, 2)):
        got = rule.diffuse(v, nu, DT, DX, sweeps)
        assert got is v
        assert_bit_equal(got, v.copy(), f"nu {nu} sweeps {sweeps}")
    assert np.signbit(v[2, 3, 0]) and np.signbit(v[0, 0]).all()
    # ... whereas a zero coefficient computed through would have lost the sign: the reason the item is skipped whole
    # (-0.0f + 0.0f * a positive sum = +0.0f)
    a, c = np.float32(0.0), np.float32(1.0)
    ones = np.ones((3, 3, 2), np.float32)
    ones[1, 1] = -0.0
    through = rule.sweep_colour(ones.copy(), ones.copy(), a, c, 0, None)
    assert np.signbit(ones[1, 1]).all() and not np.signbit(through[1, 1]).any()


def test_the_coefficients_are_rounded_operation_by_operation():
    a, c = rule.coefficients(NU, DT, DX)
    f = np.float32
    assert a.dtype == np.float32 and c.dtype == np.float32
    assert a == f(f(f(NU) * f(DT)) / f(f(DX) * f(DX))) and c == f(f(1) / f(f(1) + f(f(4) * a)))
    assert rule.coefficients(0.5, 1.0, 1.0) == (f(0.5), f(1.0) / f(3.0))


def test_the_sweeps_contract_as_derived():
    """With a = 0.5 every row of the iteration has weight at most 4 a c = 2 / 3 (at the rim a ghost is the cell itself, with
    the same weight), so the update max|u_k+1 - u_k| shrinks by 2 / 3 per sweep: (2 / 3)^60 = 3e-11 of max|u0|, and what is
    left after k = 60 sweeps is float32 rounding.  The bound 1e-5 max|u0| is derived, not measured."""
    v = random_fields(61, 81, 11)[0]
    nu, dt, dx = 0.5, 1.0, 1.0
    a, c = rule.coefficients(nu, dt, dx)
    assert a == np.float32(0.5)
    u60, u61 = rule.diffuse(v, nu, dt, dx, 60), rule.diffuse(v, nu, dt, dx, 61)
    update = np.abs(u61 - u60).max()
    print(f"max|u61 - u60| = {update:.3e}, bound {1e-5 * np.abs(v).max():.3e}")
    assert update <= 1e-5 * np.abs(v).max()


def test_a_solid_cell_is_never_written_and_is_read_as_it_is():
    dim_x, dim_y = 13, 9
    v = random_fields(dim_x, dim_y, 5)[0]
    solid = mask("seeded", dim_x, dim_y)
    assert solid.any() and not solid.all()
    got = rule.diffuse(v, NU, DT, DX, 3, solid)
    assert_bit_equal(got[solid], v[solid], "solid cells")
    assert (got[~solid] != v[~solid]).any()
    # read as what it holds: another value in a solid cell changes its fluid neighbours
    j, i = np.argwhere(solid)[0]
    other = v.copy()
    other[j, i] += 5.0
    changed = rule.diffuse(other, NU, DT, DX, 1, solid) != rule.diffuse(v, NU, DT, DX, 1, solid)
    changed[j, i] = False
    assert changed.any()
    # all solid: nothing moves
    assert_bit_equal(rule.diffuse(v, NU, DT, DX, 2, np.ones((dim_y, dim_x), bool)), v, "all solid")


# ---- the host unit and the tile core -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    subprocess.run(["make", "-C", CPP, "-f", "viscosity.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "viscosity_driver")


def test_the_host_side_of_the_viscosity():
    """`make -C tests/cpp -f viscosity.mk`: tests/cpp/viscosity_driver.cpp, a stand-alone program (a plain build, no sanitizer).
    The unfused sequence of a viscous step in order, with and without solids; ceil(sweeps / D) launches with the right last
    k, the same u0 in all of them and the last one's buffer made the velocity; no third buffer at sweeps <= D; every
    SFL_ERR_STATE refusal with its message and nothing launched; clearing restores the old launches; the batches' table
    and launches; destroy leaves no allocation."""
    r = subprocess.run([driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=[f"{x}x{y}" for x, y in SHAPES])
def test_the_tile_core_run_on_the_host_diffuses_by_the_rule(tmp_path, dim_x, dim_y):
    """Every mask (and none) at every sweep count of one shape in one run of the driver: the velocity, the mask, the shape,
    sweeps, nu, dt and dx go in through a file, the diffusion runs tile by tile with the launch segmentation of the host
    code, the velocity comes back."""
    v = random_fields(dim_x, dim_y, 41)[0]
    cases = [(kind, sweeps) for kind in [None] + MASKS for sweeps in SWEEPS]
    src, dst = tmp_path / "cases.bin", tmp_path / "u.bin"
    with open(src, "wb") as f:
        for kind, sweeps in cases:
            f.write(np.array([dim_x, dim_y, sweeps, kind is not None], np.int32).tobytes())
            f.write(np.array([NU, DT, DX], np.float32).tobytes())
            f.write(v.tobytes())
            if kind is not None:
                f.write(mask(kind, dim_x, dim_y).astype(np.uint8).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} cases diffused tile by tile (TX {TX}, TY {TY}, D {D})" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.float32).reshape(len(cases), dim_y, dim_x, 2)
    for k, (kind, sweeps) in enumerate(cases):
        solid = None if kind is None else mask(kind, dim_x, dim_y)
        assert_bit_equal(got[k], rule.diffuse(v, NU, DT, DX, sweeps, solid), f"{dim_x}x{dim_y} {kind} sweeps {sweeps}")


VALUE_SHAPES = [(TX + 1, TY + 1), (257, 130)]
VALUE_TEXTURES = [("quiescent", 1e-30), ("tiny", None)]


@pytest.mark.parametrize("name,amplitude", VALUE_TEXTURES, ids=[t[0] for t in VALUE_TEXTURES])
@pytest.mark.parametrize("dim_x,dim_y", VALUE_SHAPES, ids=[f"{x}x{y}" for x, y in VALUE_SHAPES])
def test_the_tile_core_on_velocities_at_the_bottom_of_the_float_range(tmp_path, dim_x, dim_y, name, amplitude):
    """The quiescent texture of tests/value_cases.py with its two records written in -- the diffusion spreads them through
    the denormals into cells that are still zero -- and the tiny one, denormal throughout, through the same file and the
    same program.  Every mask with a fluid cell (and none) keeps 100 denormal components."""
    v = value_cases.held_velocities(name, amplitude, dim_x, dim_y)[0]
    cases = [(kind, sweeps) for kind in [None] + MASKS for sweeps in (D - 1, 2 * D + 3)]
    src, dst = tmp_path / "cases.bin", tmp_path / "u.bin"
    with open(src, "wb") as f:
        for kind, sweeps in cases:
            f.write(np.array([dim_x, dim_y, sweeps, kind is not None], np.int32).tobytes())
            f.write(np.array([NU, DT, DX], np.float32).tobytes())
            f.write(v.tobytes())
            if kind is not None:
                f.write(mask(kind, dim_x, dim_y).astype(np.uint8).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} cases diffused tile by tile (TX {TX}, TY {TY}, D {D})" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.float32).reshape(len(cases), dim_y, dim_x, 2)
    for k, (kind, sweeps) in enumerate(cases):
        want = rule.diffuse(v, NU, DT, DX, sweeps, None if kind is None else mask(kind, dim_x, dim_y))
        assert kind == "all" or value_cases.denormals(want) >= 100, (kind, sweeps, value_cases.denormals(want))
        assert_bit_equal(got[k], want, f"{name} {dim_x}x{dim_y} {kind} sweeps {sweeps}")


def test_the_shapes_straddle_the_tile():
    """The lists are derived from TX, TY and D where they can be; the fixed shapes must keep their place should the tile change."""
    assert 2 <= TX <= 128 and 2 <= TY <= 64 and D >= 2
    assert any(x < TX and y < TY for x, y in SHAPES) and (TX + 1, TY + 1) in SHAPES
    assert any(x > 2 * TX and x % TX and y > 2 * TY and y % TY for x, y in SHAPES), "several ragged tiles both ways"
    for dim_x, dim_y in SHAPES[2:]:
        m = mask("plate", dim_x, dim_y)
        assert m[:, TX - 1].any() and m[:, TX].any(), "the plate lies across a tile edge"
