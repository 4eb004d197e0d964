"""Solid cells inside a batch member's grid, the CPU side: the rule of include/sfl.h ("SOLIDS") as tests/solid_rule.py restates
it, held against the reference and the oracle where the two must agree bit for bit (no solid cell: the reference's step; a
solid outer ring: the reference on the inner grid); the rule's own invariants on seeded masks; sfl_batch_set_solids and its
companions as the binding sees them; every refusal that needs no device; and the host unit (csrc/solids.cpp and its hooks in
the step, solve, statistics, history and view calls) run through by tests/cpp/solids_driver.cpp over a runtime that lives on
the host.  tests/test_solids_gpu.py has the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import solid_rule as rule
from conftest import ROOT, assert_bit_equal, random_fields

SHAPES = [(2, 2), (3, 2), (7, 5), (33, 18), (61, 81)]   # (dim_x, dim_y)
DXS = [1.0, 0.7]
ITERS, OMEGA, DT = 7, 1.9, 1 / 30.0


@pytest.fixture(params=["reference", "oracle"])
def cpu(request):
    """The compiled reference (skipped where it was never built) and its C restatement (always)."""
    return request.getfixturevalue(request.param)


def fields(dim_x, dim_y, seed=11):
    v, c, s = random_fields(dim_x, dim_y, seed, vamp=40.0)
    return v, c, s


def framed(a, fill=0):
    """a[dim_y, dim_x, ...] inside a ring of `fill`."""
    pad = [(1, 1), (1, 1)] + [(0, 0)] * (a.ndim - 2)
    return np.ascontiguousarray(np.pad(a, pad, constant_values=fill))


def ring(dim_x, dim_y):
    """The mask of a (dim_x + 2) x (dim_y + 2) grid whose outer ring is solid."""
    m = np.ones((dim_y + 2, dim_x + 2), bool)
    m[1:-1, 1:-1] = False
    return m


def seeded_mask(dim_x, dim_y, seed, share=0.3):
    return np.random.default_rng(seed).random((dim_y, dim_x)) < share


# ---- the two anchors: the rule against the reference and the oracle --------------------------------------------------
@pytest.mark.parametrize("dx", DXS)
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_with_no_solid_cell_the_rules_step_is_the_reference_step(cpu, dim_x, dim_y, dx):
    v, c, _ = fields(dim_x, dim_y)
    got = rule.step(cpu, v, c, np.zeros((dim_y, dim_x), bool), DT, dx, ITERS, OMEGA)
    want = cpu.step(v, c, DT, dx, ITERS, OMEGA)
    for name, a, b in zip(("velocity", "divergence", "pressure", "colour"), got, want):
        assert_bit_equal(a, b, f"{name} {dim_x}x{dim_y} dx {dx}")


@pytest.mark.parametrize("dx", DXS)
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_inside_a_solid_ring_the_three_operators_are_the_references_on_the_inner_grid(cpu, dim_x, dim_y, dx):
    v, _, s = fields(dim_x, dim_y)
    m = ring(dim_x, dim_y)
    inner = (slice(1, -1), slice(1, -1))
    assert_bit_equal(rule.divergence(framed(v), m, dx)[inner], cpu.divergence(v, dx), "divergence")
    assert_bit_equal(rule.solve(framed(s), m, dx, ITERS, OMEGA)[inner], cpu.poisson_solve(s, dx, ITERS, OMEGA), "solve")
    assert_bit_equal(rule.gradient(framed(v), framed(s), m, dx)[inner], cpu.subtract_gradient(v, s, dx), "gradient")
    # (what the ring itself holds: nothing)
    assert not rule.divergence(framed(v), m, dx)[m].any() and not rule.solve(framed(s), m, dx, ITERS, OMEGA)[m].any()


@pytest.mark.parametrize("dx", DXS)
@pytest.mark.parametrize("dim_x,dim_y", SHAPES)
def test_inside_a_solid_ring_a_step_at_dt_0_is_the_references_on_the_inner_grid(cpu, dim_x, dim_y, dx):
    v, c, _ = fields(dim_x, dim_y)
    got = rule.step(cpu, framed(v), framed(c), ring(dim_x, dim_y), 0.0, dx, ITERS, OMEGA)
    want = cpu.step(v, c, 0.0, dx, ITERS, OMEGA)
    for name, a, b in list(zip(("velocity", "divergence", "pressure"), got, want)):
        assert_bit_equal(np.ascontiguousarray(a[1:-1, 1:-1]), b, f"{name} {dim_x}x{dim_y} dx {dx}")


# ---- the rule's own invariants on seeded masks -------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y,seed", [(7, 5, 3), (33, 18, 4), (61, 81, 5)])
def test_invariants_on_seeded_masks(oracle, dim_x, dim_y, seed):
    v, c, _ = fields(dim_x, dim_y, seed)
    solid = seeded_mask(dim_x, dim_y, seed)
    solid[2, 3] = False   # an isolated fluid cell: present == 0 ...
    solid[1, 3] = solid[3, 3] = solid[2, 2] = solid[2, 4] = True
    n = rule.count_present(solid)
    assert (n == 0).any() and (n == 1).any() and solid.any() and not solid.all()
    sj, si = np.argwhere(solid)[len(np.argwhere(solid)) // 2]
    fj, fi = np.argwhere(~solid)[len(np.argwhere(~solid)) // 2]
    forces = [(int(fi), int(fj), 3.0, -2.0)]
    got = rule.step(oracle, v, c, solid, DT, 0.7, ITERS, OMEGA, forces)
    u, d, p, col = got
    # solid cells end with v = 0, p = 0, div = 0 (as bits: +0.0f)
    for name, a in (("velocity", u), ("divergence", d), ("pressure", p)):
        assert not np.ascontiguousarray(a[solid]).view(np.uint32).any(), name
    assert np.isfinite(u).all() and np.isfinite(p).all()
    # a force on a solid cell changes no field; one on a fluid cell does
    again = rule.step(oracle, v, c, solid, DT, 0.7, ITERS, OMEGA, forces + [(int(si), int(sj), 50.0, 60.0)])
    for name, a, b in zip(("velocity", "divergence", "pressure", "colour"), again, got):
        assert_bit_equal(a, b, name)
    without = rule.step(oracle, v, c, solid, DT, 0.7, ITERS, OMEGA)
    assert not np.array_equal(without[0], u)
    # the update norm ignores solid cells, whatever they hold; and is the plain maximum over the fluid ones
    norm = rule.update_norm(p, d, solid, 0.7)
    p2, d2 = p.copy(), d.copy()
    p2[solid], d2[solid] = np.nan, 1e30
    assert rule.update_norm(p2, d2, solid, 0.7).view(np.uint32) == norm.view(np.uint32) and np.isfinite(norm) and norm > 0
    p3 = p.copy()
    p3[fj, fi] = np.nan
    assert np.isnan(rule.update_norm(p3, d, solid, 0.7))
    assert rule.update_norm(p, d, np.ones_like(solid), 0.7).view(np.uint32) == 0


def test_the_code_bytes_of_a_hand_written_mask():
    """4 x 3, row j = 0 first: bit 0 W, 1 E, 2 S (j - 1), 3 N (j + 1) present, bit 4 fluid; a solid cell's byte is 0.  The same
    mask and bytes as tests/cpp/solids_driver.cpp holds the host unit to."""
    solid = np.array([[0, 1, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]], bool)
    want = np.array([[16 | 8, 0, 16 | 2, 16 | 1 | 8],
                     [16 | 2 | 4 | 8, 16 | 1 | 8, 0, 16 | 4],
                     [16 | 2 | 4, 16 | 1 | 2 | 4, 16 | 1, 0]], np.uint8)
    assert np.array_equal(rule.codes(solid), want)
    assert np.array_equal(rule.codes(np.zeros((3, 3), bool)), [[26, 27, 25], [30, 31, 29], [22, 23, 21]])
    assert not rule.codes(np.ones((2, 2), bool)).any()


# ---- the binding --------------------------------------------------------------------------------------------------------
def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pb = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint8)
    want = {"sfl_batch_set_solids": [vp, pb, i], "sfl_batch_solids_info": [vp, pi, pi], "sfl_batch_solids_download": [vp, i, i, pb, sz]}
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, args), name
        assert getattr(lib, name).argtypes == args and getattr(lib, name).restype == C.c_int
        assert re.search(r"SFL_API int %s\(sfl_batch \*b[,)]" % name, header), name
    assert "sfl_batch_set_solids(sfl_batch *b, const uint8_t *mask, int per_member);" in header
    assert "sfl_batch_solids_download(sfl_batch *b, int first, int count, uint8_t *host, size_t bytes);" in header
    for name in ("set_solids", "solids", "solids_info"):
        assert callable(getattr(sfl.BatchSolver, name, None)), name
    assert lib.sfl_abi_version() == 1


def test_the_header_states_the_rule():
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    section = header[header.index("--- SOLIDS:"):header.index("SFL_API int sfl_batch_set_solids")]
    for words in ("PRESENT when it is inside the domain and fluid", "(((z + W) + E) + S) + N", "z = -0.0f iff present == 4",
                  "-0.25f, (float)(-1.0 / 3.0), -0.5f, -1.0f", "k = 0.0f for present == 0", "(i + j) & 1", "own.x for W, -own.x for E, own.y for S, -own.y for",
                  "maximum over FLUID cells", "a member without a fluid cell reports 0.0f", "the vorticity view reads the zero",
                  "sfl_batch_create_large", "sfl_batch_step_n_until", "sfl_batch_history_start", "SFL_VIEW_DIVERGENCE"):
        assert words in section, words


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    mask, w = (C.c_uint8 * 12)(), C.c_int(5)
    refusals = [
        (lambda: lib.sfl_batch_set_solids(None, mask, 2), "sfl_batch_set_solids: per_member must be 0 or 1 (got 2)"),
        (lambda: lib.sfl_batch_set_solids(None, mask, -1), "per_member must be 0 or 1 (got -1)"),
        (lambda: lib.sfl_batch_set_solids(None, mask, 1), "sfl_batch_set_solids: batch is NULL"),
        (lambda: lib.sfl_batch_set_solids(None, None, 0), "sfl_batch_set_solids: batch is NULL"),
        (lambda: lib.sfl_batch_solids_info(None, C.byref(w), C.byref(w)), "sfl_batch_solids_info: batch is NULL"),
        (lambda: lib.sfl_batch_solids_download(None, 0, 1, mask, 12), "sfl_batch_solids_download: batch is NULL")]
    for k, (call, message) in enumerate(refusals):
        assert call() == cap.ERR_INVALID, k
        assert message in lib.sfl_last_error().decode(), (k, message, lib.sfl_last_error())
    assert w.value == 5


def test_the_python_front_end_checks_the_mask_before_the_library_sees_it(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        Fake().set_solids(np.zeros((4, 3), bool))
    with pytest.raises(ValueError, match="shape"):
        Fake().set_solids(np.zeros((3, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="bool or uint8"):
        Fake().set_solids(np.zeros((3, 4), np.float32))


def test_the_host_side_of_the_solids():
    """`make -C tests/cpp -f solids.mk`: tests/cpp/solids_driver.cpp, a stand-alone program (a plain build, no sanitizer).  The
    code bytes the device is handed for a hand-written mask; which launcher each call picks with and without solids and with
    which member stride; clearing restores the old launchers; a timeline replay falls back to a launch per step; the admission
    order: a call's own argument checks, then the state refusals with their messages, and nothing staged or launched by a
    refused call; download and info; destroy with solids set leaves no allocation."""
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "solids.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, "solids_driver")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
