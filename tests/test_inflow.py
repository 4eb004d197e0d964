"""Inflow profiles and the flux through the openings, the CPU side (include/sfl.h "INFLOW PROFILES AND FLUX"): the eight calls
as the header declares and the binding sees them; the rule as tests/inflow_rule.py restates it, anchored on
tests/opening_rule.py (a uniform profile: the bits of no profile) and on integers computed by hand; every refusal that needs no
device; and the host unit (csrc/inflow.cpp and its hooks in csrc/openings.cpp) with the shared flux header (csrc/open_flux.h)
run through by tests/cpp/inflow_driver.cpp over a runtime that lives on the host.  tests/test_inflow_gpu.py and
tests/test_context_inflow_gpu.py have the kernels."""
import ctypes as C
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

import inflow_rule as rule
import opening_rule
from conftest import ROOT, assert_bit_equal, random_fields
from test_openings import channel_walls, tunnel

DT, DX, ITERS, OMEGA = 1 / 30.0, 0.7, 7, 1.9
CONTEXT = ("sfl_set_inflow_profile", "sfl_inflow_profile_info", "sfl_inflow_profile_download", "sfl_openings_flux")
BATCH = ("sfl_batch_set_inflow_profile", "sfl_batch_inflow_profile_info", "sfl_batch_inflow_profile_download", "sfl_batch_openings_flux")


def parabola(dim_y, peak, first=1, last=None):
    """((0, j), (u(j), 0)) for the west cells of rows first .. last: u = peak * 4 s (1 - s), s across those rows."""
    last = dim_y - 2 if last is None else last
    height = last - first + 1
    return [((0, j), (np.float32(peak * 4.0 * ((j - first + 0.5) / height) * (1.0 - (j - first + 0.5) / height)), np.float32(0.0)))
            for j in range(first, last + 1)]


# ---- the header and the binding ------------------------------------------------------------------------------------------
def test_the_eight_calls_are_declared_exported_and_bound(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pf, pl, px = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_int64), C.POINTER(cap.OpenFlux)
    want = {"sfl_set_inflow_profile": [vp, pi, pf, i], "sfl_inflow_profile_info": [vp, pi], "sfl_inflow_profile_download": [vp, pi, pf, i],
            "sfl_openings_flux": [vp, px], "sfl_batch_set_inflow_profile": [vp, pi, pi, pf, i], "sfl_batch_inflow_profile_info": [vp, pi, pl],
            "sfl_batch_inflow_profile_download": [vp, i, pi, pf, i, pi], "sfl_batch_openings_flux": [vp, i, i, px, sz]}
    assert set(want) == set(CONTEXT + BATCH)
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for line in ("SFL_API int sfl_set_inflow_profile(sfl_context *ctx, const int *cells_ij, const float *vel_xy, int n);",
                 "SFL_API int sfl_inflow_profile_info(sfl_context *ctx, int *records);",
                 "SFL_API int sfl_inflow_profile_download(sfl_context *ctx, int *cells_ij, float *vel_xy, int capacity);",
                 "SFL_API int sfl_openings_flux(sfl_context *ctx, struct sfl_open_flux *out);",
                 "SFL_API int sfl_batch_set_inflow_profile(sfl_batch *b, const int *members, const int *cells_ij, const float *vel_xy, int n);",
                 "SFL_API int sfl_batch_inflow_profile_info(sfl_batch *b, int *set, int64_t *records);",
                 "SFL_API int sfl_batch_inflow_profile_download(sfl_batch *b, int member, int *cells_ij, float *vel_xy, int capacity, int *records);",
                 "SFL_API int sfl_batch_openings_flux(sfl_batch *b, int first, int count, struct sfl_open_flux *host, size_t bytes);"):
        assert line in header, line
    for name in ("set_inflow_profile", "inflow_profile", "openings_flux"):
        assert callable(getattr(sfl.BatchSolver, name, None)) and callable(getattr(sfl.Solver, name, None)), name
    assert callable(sfl.openings_flux_xy)
    assert lib.sfl_abi_version() == 1


def test_the_record_has_the_headers_layout_in_every_binding(sfl):
    offsets = {"inflow": 0, "outflow": 8, "exp2": 16, "max_abs_n": 20, "inflow_cells": 24, "outflow_cells": 28, "nonfinite": 32, "reserved": 36}
    for dtype in (sfl.OPEN_FLUX_DTYPE, rule.FLUX_DTYPE):
        assert dtype.itemsize == 40 and {n: dtype.fields[n][1] for n in dtype.names} == offsets
    assert sfl.OPEN_FLUX_DTYPE == rule.FLUX_DTYPE
    assert C.sizeof(sfl.capi.OpenFlux) == 40 and {n: getattr(sfl.capi.OpenFlux, n).offset for n, _ in sfl.capi.OpenFlux._fields_} == offsets
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    assert "/* 40 bytes: offsets 0, 8, 16, 20, 24, 28, 32, 36 */" in header
    rec = np.zeros(2, sfl.OPEN_FLUX_DTYPE)
    rec["inflow"], rec["outflow"], rec["exp2"] = (3 << 31, -5), (1 << 31, 7), (-31, 2)
    assert np.array_equal(sfl.openings_flux_xy(rec), [[3.0, 1.0], [-20.0, 28.0]]) and sfl.openings_flux_xy(rec[0]).shape == (2,)


def test_the_header_states_the_rule_in_its_own_section():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    start, end = header.index("/* --- INFLOW PROFILES AND FLUX"), header.index("/* A batch is used from one thread at a time")
    assert header.index("SFL_API int sfl_openings_download(") < start < end
    section = header[start:end]
    for words in ("the later wins", "map byte is SFL_OPEN_INFLOW", "names the first offending", "solid at the time has no effect", "A new map (sfl_batch_set_openings, sfl_set_openings) drops",
                  "keeps it", "ANCHOR", "produces the bits of no profile", "LIVE OPEN CELLS", "MINUS the pressure gradient of item 6", "what actually enters, not what\n * was imposed",
                  "-v.x on the W rim, +v.x on E, -v.y on S, +v.y on N", "ONE q serves both sums", "trunc(ldexp((double)n, -q))", "positive when fluid enters",
                  "no launch is made", "the same bytes", "argument checks come first", "without openings there is no profile", "leaves the profile as it was"):
        assert words in section, words
    for name in CONTEXT + BATCH:
        assert f"SFL_API int {name}(" in section, name


# ---- the rule's anchors --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(7, 5), (33, 18)])
def test_a_uniform_profile_gives_the_bits_of_no_profile_over_three_steps(oracle, dim_x, dim_y):
    v, c, _ = random_fields(dim_x, dim_y, 21, vamp=30.0)
    solid, open, inflow = channel_walls(dim_x, dim_y), tunnel(dim_x, dim_y), (np.float32(3.5), np.float32(-0.25))
    solid[dim_y // 2, 0] = True   # a solid inflow cell: its record has no effect
    profile = [((0, j), inflow) for j in range(1, dim_y - 1)]
    forces = [(2, 2, 3.0, -2.0), (0, 2, 5.0, 6.0)]   # the second on a profiled cell: no effect
    a, b = (v, None, None, c), (v, None, None, c)
    for _ in range(3):
        a = rule.step(oracle, a[0], a[3], solid, open, inflow, profile, DT, DX, ITERS, OMEGA, forces)
        b = opening_rule.step(oracle, b[0], b[3], solid, open, inflow, DT, DX, ITERS, OMEGA, forces)
        for name, x, y in zip(("velocity", "divergence", "pressure", "colour"), a, b):
            assert_bit_equal(x, y, name)
    # ... and another profile is another flow; of two records on a cell the later wins
    other = rule.step(oracle, v, c, solid, open, inflow, parabola(dim_y, 6.0), DT, DX, ITERS, OMEGA)
    assert not np.array_equal(other[0], opening_rule.step(oracle, v, c, solid, open, inflow, DT, DX, ITERS, OMEGA)[0])
    twice = [((0, 1), (9.0, 9.0))] + parabola(dim_y, 6.0)
    assert_bit_equal(rule.step(oracle, v, c, solid, open, inflow, twice, DT, DX, ITERS, OMEGA)[0], other[0], "the later record wins")
    assert rule.unique(twice) == rule.unique(parabola(dim_y, 6.0)) and [cell for cell, _ in rule.unique(twice[::-1])] == [(0, j) for j in range(1, dim_y - 1)]
    assert rule.check_profile([((0, 1), (1, 1)), ((dim_x - 1, 1), (1, 1))], open) == 1 and rule.check_profile([((1, 1), (1, 1))], open) == 0


def test_the_flux_of_a_known_parabolic_inlet_is_the_integers_computed_by_hand():
    """6 x 6, the west cells of rows 1..4 an inflow with u = 0.75, 1.75, 1.75, 0.75 (a parabola of peak 2 sampled at s = 1/8, 3/8,
    ...: 2 * 4 s (1 - s) = 0.875, 1.875 -- taken as the dyadic 0.75 and 1.75 so that every term is an integer by hand), the east
    cells an outflow with u = 1.25 each.  max |n| = 1.75: floor(log2) = 0, q = -32, every term is n * 2^32."""
    open = tunnel(6, 6)
    v = np.zeros((6, 6, 2), np.float32)
    v[1:5, 0, 0] = [0.75, 1.75, 1.75, 0.75]
    v[1:5, -1, 0] = 1.25
    v[2, 3] = (99.0, -99.0)   # an interior cell: no part of it
    rec = rule.flux(v, open)
    assert (int(rec["exp2"]), float(rec["max_abs_n"])) == (-32, 1.75)
    assert int(rec["inflow"]) == 5 * 2 ** 32 and int(rec["outflow"]) == 5 * 2 ** 32 and int(rec["inflow"]) - int(rec["outflow"]) == 0
    assert (int(rec["inflow_cells"]), int(rec["outflow_cells"]), int(rec["nonfinite"]), int(rec["reserved"])) == (4, 4, 0, 0)
    assert rule.flux_xy(rec) == (5.0, 5.0) == opening_rule.flux(v, open)
    # a solid open cell takes no part; a NaN and an Inf are counted and the rest is summed; a backflow is negative
    solid = np.zeros((6, 6), bool)
    solid[1, 0] = True
    v[2, -1, 0], v[3, -1, 0], v[4, -1, 0] = np.nan, -np.inf, -0.5
    rec = rule.flux(v, open, solid)
    assert (int(rec["inflow_cells"]), int(rec["outflow_cells"]), int(rec["nonfinite"])) == (3, 4, 2)
    assert int(rec["inflow"]) == int(4.25 * 2 ** 32) and int(rec["outflow"]) == int(0.75 * 2 ** 32)
    # denormals are included; all zeros give q = 0
    tiny = np.zeros((6, 6, 2), np.float32)
    tiny[1, 0, 0], tiny[2, 0, 0] = np.float32(3e-45), np.float32(1.4e-45)   # 2 and 1 units of 2^-149
    rec = rule.flux(tiny, open)
    assert int(rec["exp2"]) == -148 - 32 and int(rec["inflow"]) == 3 * 2 ** 31 and rule.flux_xy(rec)[0] == 3 * 2.0 ** -149
    rec = rule.flux(np.zeros((6, 6, 2), np.float32), open)
    assert rec.tobytes()[:24] == bytes(24) and int(rec["inflow_cells"]) == 4
    assert rule.flux(v, np.zeros((6, 6), np.uint8)).tobytes() == bytes(40), "no live open cell: all zeros"


@pytest.mark.parametrize("dim_x,dim_y", [(7, 9), (61, 41)])
def test_inflow_minus_outflow_of_a_uniform_stream_through_a_channel_is_exactly_zero(dim_x, dim_y):
    solid, open = channel_walls(dim_x, dim_y), tunnel(dim_x, dim_y)
    v = np.zeros((dim_y, dim_x, 2), np.float32)
    v[~solid, 0] = np.float32(3.3)   # (not a dyadic number: the terms are truncated alike on both sides)
    rec = rule.flux(v, open, solid)
    assert int(rec["inflow"]) == int(rec["outflow"]) > 0 and int(rec["inflow_cells"]) == int(rec["outflow_cells"]) == dim_y - 2


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    cells, good = (C.c_int * 4)(0, 1, 0, 2), (C.c_float * 4)(1.0, 0.0, 2.0, 0.0)
    nan, inf = (C.c_float * 4)(1.0, 0.0, 2.0, float("nan")), (C.c_float * 4)(float("-inf"), 0.0, 2.0, 0.0)
    rec, n, w = cap.OpenFlux(), C.c_int(5), C.c_int64(5)
    refusals = [
        (lambda: lib.sfl_set_inflow_profile(None, cells, good, -1), "sfl_set_inflow_profile: n must be >= 0 (got -1)"),
        (lambda: lib.sfl_set_inflow_profile(None, None, good, 2), "sfl_set_inflow_profile: cells_ij is NULL with n = 2"),
        (lambda: lib.sfl_set_inflow_profile(None, cells, None, 2), "sfl_set_inflow_profile: vel_xy is NULL with n = 2"),
        (lambda: lib.sfl_set_inflow_profile(None, cells, nan, 2), "sfl_set_inflow_profile: the velocity of a record must be finite (record 1: (2, nan))"),
        (lambda: lib.sfl_set_inflow_profile(None, cells, inf, 2), "sfl_set_inflow_profile: the velocity of a record must be finite (record 0: (-inf, 0))"),
        (lambda: lib.sfl_set_inflow_profile(None, cells, good, 2), "sfl_set_inflow_profile: ctx is NULL"),
        (lambda: lib.sfl_set_inflow_profile(None, None, None, 0), "sfl_set_inflow_profile: ctx is NULL"),
        (lambda: lib.sfl_inflow_profile_info(None, C.byref(n)), "sfl_inflow_profile_info: ctx is NULL"),
        (lambda: lib.sfl_inflow_profile_download(None, cells, good, 2), "sfl_inflow_profile_download: ctx is NULL"),
        (lambda: lib.sfl_openings_flux(None, C.byref(rec)), "sfl_openings_flux: ctx is NULL"),
        (lambda: lib.sfl_batch_set_inflow_profile(None, None, cells, good, -3), "sfl_batch_set_inflow_profile: n must be >= 0 (got -3)"),
        (lambda: lib.sfl_batch_set_inflow_profile(None, None, None, good, 1), "sfl_batch_set_inflow_profile: cells_ij is NULL with n = 1"),
        (lambda: lib.sfl_batch_set_inflow_profile(None, None, cells, None, 1), "sfl_batch_set_inflow_profile: vel_xy is NULL with n = 1"),
        (lambda: lib.sfl_batch_set_inflow_profile(None, None, cells, nan, 2), "sfl_batch_set_inflow_profile: the velocity of a record must be finite (record 1: (2, nan))"),
        (lambda: lib.sfl_batch_set_inflow_profile(None, None, cells, good, 2), "sfl_batch_set_inflow_profile: batch is NULL"),
        (lambda: lib.sfl_batch_inflow_profile_info(None, C.byref(n), C.byref(w)), "sfl_batch_inflow_profile_info: batch is NULL"),
        (lambda: lib.sfl_batch_inflow_profile_download(None, 0, cells, good, 2, C.byref(n)), "sfl_batch_inflow_profile_download: batch is NULL"),
        (lambda: lib.sfl_batch_openings_flux(None, 0, 1, C.byref(rec), 40), "sfl_batch_openings_flux: batch is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert n.value == 5 and w.value == 5


def test_the_python_front_end_checks_the_shapes_before_the_library_sees_the_records(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2

        def __del__(self):
            pass

    class FakeContext(sfl.Solver):
        def __init__(self):
            self._h, self._lib = None, None
            self.dim_x, self.dim_y = 4, 3

        def __del__(self):
            pass

    for fake in (Fake(), FakeContext()):
        with pytest.raises(ValueError, match="cells of shape"):
            fake.set_inflow_profile([0, 1], [[1.0, 0.0]])
        with pytest.raises(ValueError, match="cells of shape"):
            fake.set_inflow_profile([[0.5, 1.0]], [[1.0, 0.0]])
        with pytest.raises(ValueError, match="vel of shape"):
            fake.set_inflow_profile([[0, 1]], [[1.0, 0.0], [2.0, 0.0]])
    with pytest.raises(ValueError, match="members of shape"):
        Fake().set_inflow_profile([[0, 1]], [[1.0, 0.0]], members=[0, 1])


# ---- the host unit and the shared flux header ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "inflow.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(cpp, "inflow_driver")


def test_the_host_side_of_the_profiles_and_the_flux():
    """`make -C tests/cpp -f inflow.mk`: tests/cpp/inflow_driver.cpp, a stand-alone program (a plain build, no sanitizer).  Its
    head comment lists what it checks."""
    r = subprocess.run([driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


def flux_cases():
    """(name, v, solid, open): random fields on the shapes of the GPU tests, and the textures a reduction can go wrong on."""
    from test_openings_gpu import map_of, solid_of
    out = []
    for dim_x, dim_y, m, s in ((3, 3, "four", "none"), (7, 5, "four", "none"), (61, 81, "four", "disc"), (96, 64, "slot", "seeded"), (257, 130, "on_solid", "walls"),
                               (5, 4, "west_east", "none"), (130, 70, "out_only", "seeded"), (61, 81, "in_only", "none"), (7, 5, "empty", "none")):
        v = random_fields(dim_x, dim_y, 77, vamp=40.0)[0]
        out.append((f"random {dim_x}x{dim_y} {m} {s}", v, solid_of(s, dim_x, dim_y), map_of(m, dim_x, dim_y)))
    dim_x, dim_y = 61, 81
    open, none = map_of("four", dim_x, dim_y), np.zeros((dim_y, dim_x), bool)
    v = random_fields(dim_x, dim_y, 78, vamp=40.0)[0].copy()
    v[5, 0, 0], v[7, -1, 0], v[0, 9, 1], v[-1, 11, 1] = np.nan, np.inf, -np.inf, np.nan
    v[9, 0, 1] = np.nan   # the tangential component of a west cell: no part of n
    out.append(("a NaN and an Inf on every side", v, none, open))
    tiny = (random_fields(dim_x, dim_y, 79, vamp=1.0)[0] * np.float32(1e-44)).astype(np.float32)
    assert 0 < np.abs(tiny).max() < np.finfo(np.float32).tiny
    out.append(("denormal normals", tiny, none, open))
    mixed = tiny.copy()
    mixed[40, 0, 0] = np.float32(3.0e38)
    out.append(("a huge normal beside denormals", mixed, none, open))
    out.append(("all-zero velocity", np.zeros((dim_y, dim_x, 2), np.float32), none, open))
    out.append(("negative zeros", np.full((dim_y, dim_x, 2), -0.0, np.float32), none, open))
    rim = open != 0
    out.append(("every open cell solid", v, rim, open))
    one = none.copy()
    one[5, 0] = True   # the NaN's cell is solid: it is not counted
    out.append(("a solid open cell", v, one, open))
    return out


def test_the_shared_flux_term_and_reduction_run_on_the_host_give_the_rules_records(tmp_path):
    """csrc/open_flux.h -- the walk over the rim, the normal, the quantisation and the two passes, as the kernels of
    csrc/inflow.hip include them -- on records dumped to a file: the rule's 40 bytes each."""
    cases = flux_cases()
    src, dst = tmp_path / "cases.bin", tmp_path / "flux.bin"
    with open(src, "wb") as f:
        for _, v, solid, open_map in cases:
            dim_y, dim_x = open_map.shape
            f.write(np.array([dim_x, dim_y], np.int32).tobytes())
            f.write(np.ascontiguousarray(v, np.float32).tobytes())
            f.write(np.ascontiguousarray(solid).astype(np.uint8).tobytes())
            f.write(np.ascontiguousarray(open_map, np.uint8).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} flux records by the shared header" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, rule.FLUX_DTYPE)
    assert len(got) == len(cases)
    for rec, (name, v, solid, open_map) in zip(got, cases):
        want = rule.flux(v, open_map, solid)
        assert rec.tobytes() == want.tobytes(), (name, rec, want)
    by_name = {name: rec for rec, (name, *_) in zip(got, cases)}
    assert int(by_name["a NaN and an Inf on every side"]["nonfinite"]) == 4 and int(by_name["a solid open cell"]["nonfinite"]) == 3
    assert by_name["every open cell solid"].tobytes() == bytes(40) and int(by_name["denormal normals"]["exp2"]) < -149
    assert int(by_name["all-zero velocity"]["exp2"]) == 0 and int(by_name["all-zero velocity"]["inflow_cells"]) > 0
