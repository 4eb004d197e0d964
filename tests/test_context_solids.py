"""Solid cells inside the grid of a whole-domain context, the CPU side (include/sfl.h "SOLIDS OF A CONTEXT"): sfl_set_solids
and its companions as the binding sees them; every refusal that needs no device; the host unit (csrc/context_solids.cpp and
its hooks in the step, the operators, the solves, the statistics, the history, the views and the transports) run through by
tests/cpp/context_solids_driver.cpp over a runtime that lives on the host; and the tile core of the masked solve
(csrc/sor_solid_tile.h) run on the host by the same program, one workgroup's tile after the other, against
tests/solid_rule.py bit for bit -- which checks the halo depth and the shrinking valid region of the temporal blocking
without a GPU.  tests/test_context_solids_gpu.py has the kernels."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solid_rule as rule
import value_cases
from conftest import ROOT, assert_bit_equal, random_fields
from test_solids_gpu import mask_of

CPP = os.path.join(ROOT, "tests", "cpp")
DX, OMEGA = 0.7, 1.9


def tile_shape():
    """TX, TY and D as csrc/sor_solid_tile.h states them."""
    text = open(os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "sor_solid_tile.h")).read()
    return tuple(int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1)) for name in ("kTX", "kTY", "kD"))


TX, TY, D = tile_shape()
# smaller than one tile; exactly one; one cell more each way; three tiles wide and one row short of a tile; 5 x 5 ragged tiles
SHAPES = [(7, 5), (TX, TY), (TX + 1, TY + 1), (2 * TX + 3, TY - 1), (257, 130)]
ITERS = [0, 1, D - 1, D, D + 1, 2 * D + 3]
MASKS = ["empty", "seeded", "plate", "isolated", "all"]


def mask(kind, dim_x, dim_y):
    """The masks of tests/test_solids_gpu.py; the plate lies ACROSS a tile edge where the shape has one."""
    if kind == "plate" and dim_x > TX:
        m = np.zeros((dim_y, dim_x), bool)
        m[dim_y // 2, TX - 3:TX + 4] = True   # a row of seven solid cells over the edge between tile columns 0 and 1
        if dim_y > TY:
            m[TY - 3:TY + 4, dim_x // 3] = True   # ... and a column over the edge between tile rows 0 and 1
        return m
    return mask_of(kind, dim_x, dim_y)


# ---- the binding and the header ------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, sz, pi, pb, pl = C.c_void_p, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(C.c_int64)
    want = {"sfl_set_solids": [vp, pb], "sfl_solids_info": [vp, pi, pl], "sfl_solids_download": [vp, pb, sz]}
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
    assert "SFL_API int sfl_set_solids(sfl_context *ctx, const uint8_t *mask);" in header
    assert "SFL_API int sfl_solids_info(sfl_context *ctx, int *set, int64_t *solid_cells);" in header
    assert "SFL_API int sfl_solids_download(sfl_context *ctx, uint8_t *host, size_t bytes);" in header
    for name in ("set_solids", "solids", "solids_info"):
        assert callable(getattr(sfl.Solver, name, None)), name
    assert lib.sfl_abi_version() == 1


def test_the_header_names_the_honoured_and_the_refused_calls_and_leaves_the_rule_alone():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    start = header.index("--- SOLIDS OF A CONTEXT")
    assert start > header.index("SFL_API int sfl_batch_solids_download"), "the new section comes behind the batches' calls"
    section = header[start:header.index("SFL_API int sfl_set_solids")]
    for words in ("sfl_step, sfl_step_n", "sfl_calculate_divergence", "sfl_poisson_solve ", "sfl_poisson_continue", "sfl_subtract_gradient",
                  "sfl_residual", "sfl_poisson_solve_until", "sfl_flow_stats", "sfl_history_", "items 1 to 7", "0.0f when there is none",
                  "SFL_OPT_SOR_FOLD", "have no effect while solids are set", "No step seams", "nranks != 1", "transport attached",
                  "sfl_comm_attach", "sfl_group_link", "SFL_VIEW_DIVERGENCE", "sfl_advect_velocity and sfl_advect_color called on their own",
                  "tracers", "vorticity", "argument checks come first"):
        assert words in section, words
    assert "(((z + W) + E) + S) + N" not in section, "the arithmetic is stated once, in the section above"
    # the rule's own section: byte for byte the parent commit's where git can show it
    old = header[header.index("--- SOLIDS:"):header.index("SFL_API int sfl_batch_set_solids")]
    r = subprocess.run(["git", "-C", ROOT, "show", "HEAD:include/sfl.h"], capture_output=True, text=True) if shutil.which("git") else None
    if r is not None and r.returncode == 0:
        was = r.stdout
        assert old == was[was.index("--- SOLIDS:"):was.index("SFL_API int sfl_batch_set_solids")]
    assert "z = -0.0f iff present == 4" in old and "sfl_batch_history_start" in old and "sfl_set_solids" not in old


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    """(The `bytes` check of sfl_solids_download needs a context to be wrong about: the host driver below has it.)"""
    lib, cap = sfl.capi.lib(), sfl.capi
    mask12, w, n = (C.c_uint8 * 12)(), C.c_int(5), C.c_int64(5)
    refusals = [
        (lambda: lib.sfl_set_solids(None, mask12), "sfl_set_solids: ctx is NULL"),
        (lambda: lib.sfl_set_solids(None, None), "sfl_set_solids: ctx is NULL"),
        (lambda: lib.sfl_solids_info(None, C.byref(w), C.byref(n)), "sfl_solids_info: ctx is NULL"),
        (lambda: lib.sfl_solids_download(None, mask12, 12), "sfl_solids_download: ctx is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert w.value == 5 and n.value == 5


def test_the_python_front_end_checks_the_mask_before_the_library_sees_it(sfl):
    class Fake(sfl.Solver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y = 4, 3

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        Fake().set_solids(np.zeros((4, 3), bool))
    with pytest.raises(ValueError, match="shape"):
        Fake().set_solids(np.zeros((2, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="bool or uint8"):
        Fake().set_solids(np.zeros((3, 4), np.float32))


# ---- the host unit and the tile core -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def driver():
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    subprocess.run(["make", "-C", CPP, "-f", "context_solids.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    return os.path.join(CPP, "context_solids_driver")


def test_the_host_side_of_a_contexts_solids():
    """`make -C tests/cpp -f context_solids.mk`: tests/cpp/context_solids_driver.cpp, a stand-alone program (a plain build,
    no sanitizer).  Which launcher each honoured call picks with a mask, without one and after a clear, the seams and the
    one-launch step of a small grid included; the launch sequence of a masked step; ceil(iters / D) solve launches with the
    right last k and p / p_alt swapped as often; the admission order: a call's own argument checks, then the state refusals
    with their messages, and nothing launched by a refused call; the `bytes` check of the download; destroy leaves no
    allocation."""
    r = subprocess.run([driver()], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


@pytest.mark.parametrize("dim_x,dim_y", SHAPES, ids=[f"{x}x{y}" for x, y in SHAPES])
def test_the_tile_core_run_on_the_host_solves_by_the_rule(tmp_path, dim_x, dim_y):
    """Every mask at every iteration count of one shape in one run of the driver: d, the mask, the shape, iters, dx and omega
    go in through a file, the solve runs tile by tile with the launch segmentation of the host code, p comes back."""
    d = (random_fields(dim_x, dim_y, 31)[2] * np.float32(7.5)).astype(np.float32)
    cases = [(kind, iters) for kind in MASKS for iters in ITERS]
    src, dst = tmp_path / "cases.bin", tmp_path / "p.bin"
    with open(src, "wb") as f:
        for kind, iters in cases:
            f.write(np.array([dim_x, dim_y, iters], np.int32).tobytes())
            f.write(np.array([DX, OMEGA], np.float32).tobytes())
            f.write(d.tobytes())
            f.write(mask(kind, dim_x, dim_y).astype(np.uint8).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} cases solved tile by tile (TX {TX}, TY {TY}, D {D})" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.float32).reshape(len(cases), dim_y, dim_x)
    for k, (kind, iters) in enumerate(cases):
        assert_bit_equal(got[k], rule.solve(d, mask(kind, dim_x, dim_y), DX, iters, OMEGA), f"{dim_x}x{dim_y} {kind} iters {iters}")


VALUE_SHAPES = [(TX + 1, TY + 1), (257, 130)]
VALUE_TEXTURES = [("quiescent", 1e-38), ("tiny", None)]   # (a quiescent right-hand side of 1e-30 leaves no denormals in 2 D + 3 iterations)


@pytest.mark.parametrize("name,amplitude", VALUE_TEXTURES, ids=[t[0] for t in VALUE_TEXTURES])
@pytest.mark.parametrize("dim_x,dim_y", VALUE_SHAPES, ids=[f"{x}x{y}" for x, y in VALUE_SHAPES])
def test_the_tile_core_on_right_hand_sides_at_the_bottom_of_the_float_range(tmp_path, dim_x, dim_y, name, amplitude):
    """The quiescent and the tiny texture of tests/value_cases.py through the same file and the same program: a pressure
    front that decays through the denormals into cells that are still zero, and a field that is denormal throughout,
    across the tile edges and the halo of the temporal blocking.  Every mask with a fluid cell keeps 100 denormal cells."""
    d = value_cases.texture(name, dim_x, dim_y, amplitude).rhs
    cases = [(kind, iters) for kind in MASKS for iters in (D - 1, 2 * D + 3)]
    src, dst = tmp_path / "cases.bin", tmp_path / "p.bin"
    with open(src, "wb") as f:
        for kind, iters in cases:
            f.write(np.array([dim_x, dim_y, iters], np.int32).tobytes())
            f.write(np.array([DX, OMEGA], np.float32).tobytes())
            f.write(d.tobytes())
            f.write(mask(kind, dim_x, dim_y).astype(np.uint8).tobytes())
    r = subprocess.run([driver(), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(cases)} cases solved tile by tile (TX {TX}, TY {TY}, D {D})" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.float32).reshape(len(cases), dim_y, dim_x)
    for k, (kind, iters) in enumerate(cases):
        want = rule.solve(d, mask(kind, dim_x, dim_y), DX, iters, OMEGA)
        assert kind == "all" or value_cases.denormals(want) >= 100, (kind, iters, value_cases.denormals(want))
        assert_bit_equal(got[k], want, f"{name} {dim_x}x{dim_y} {kind} iters {iters}")


# ---- a guard on the shapes -----------------------------------------------------------------------------------------------
def test_the_shapes_of_both_test_files_straddle_the_tile():
    """The shape and iteration lists are derived from TX, TY and D where they can be; the fixed ones must keep their place
    should the tile change: fails when they no longer straddle it."""
    import test_context_solids_gpu as gpu
    assert 2 <= TX <= 128 and 2 <= TY <= 64 and D >= 2
    for shapes in (SHAPES, gpu.SHAPES):
        assert any(x < TX and y < TY for x, y in shapes), "a shape inside one tile"
        assert (TX + 1, TY + 1) in shapes, "one cell more than a tile, both ways"
        assert any(x > 2 * TX and x % TX and y > 2 * TY and y % TY for x, y in shapes), "several ragged tiles both ways"
    assert (TX, TY) in SHAPES and (2 * TX + 3, TY - 1) in SHAPES
    for iters in (ITERS, gpu.SOLVE_ITERS):
        assert list(iters) == [0, 1, D - 1, D, D + 1, 2 * D + 3]
    assert gpu.ITERS_LONG == 2 * D + 3 and gpu.ITERS % D != 0, "the steps' solves end in a launch that runs fewer than D iterations"
    # the plates cross a tile edge
    for dim_x, dim_y in SHAPES[2:]:
        m = mask("plate", dim_x, dim_y)
        assert m[:, TX - 1].any() and m[:, TX].any(), (dim_x, dim_y)
    m = mask("plate", 257, 130)
    assert m[TY - 1].any() and m[TY].any()
    assert mask_of("plate", 257, 130)[TY - 1:TY + 1, 257 // 3].all(), "the GPU file's plate crosses the edge between tile rows 0 and 1"
