"""CPU suite: the loads (include/sfl.h "LOADS") without a GPU.  The header states the rule and the record, the binding
mirrors it; the argument refusals that need no device, each with its own message; the sanity of the rule's numpy restatement
(tests/load_rule.py), which tests/test_loads_gpu.py holds the samplers to; the host side (csrc/loads.cpp and its hooks in the
step calls) run through by tests/cpp/loads_driver.cpp."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import load_rule as rule
from conftest import ROOT

F = np.float32
FLT_MAX = np.finfo(F).max


def header():
    return open(os.path.join(ROOT, "include", "sfl.h")).read()


# ---- the header, the struct, the binding ----------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = header()
    section = text[text.index("--- LOADS:"):text.index("SFL_API int sfl_batch_set_bodies")]
    for words in ("S is INSIDE THE DOMAIN", "The rim of the grid is not a body and has no faces", "0 = in no body", "SFL_MAX_BODIES",
                  "only where the cell is solid at the time of the sample", "NaN or +-Inf", "0.0f when there is none",
                  "floor(log2(max_abs_p)) - 32", "frexp((double)max_abs_p)'s exponent - 1 - 32", "q = 0 when",
                  "(int64_t)trunc(ldexp((double)p, -q))", "|t| < 2^33", "24 bits", "2^-32 of the largest", "WEST", "EAST", "SOUTH and NORTH",
                  "faces[0] is the frontal area", "2^28 cells", "2^30 faces", "2^63", "never overflow", "fx * 2^exp2", "multiplies by dx",
                  "PRESSURE load only", "no torque", "All zeros mean a body", "bit for bit", "refused WHOLE", "(s + 1) * every",
                  "while no solids are set is zero records"):
        assert words in section, words
    assert "#define SFL_MAX_BODIES 16" in text


def test_the_struct_is_48_bytes_and_the_bindings_match_it(sfl):
    text = header()
    body = re.search(r"struct sfl_body_load \{(.*?)\};", text, re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(\w+)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [("int64_t", "fx"), ("int64_t", "fy"), ("int32_t", "exp2"), ("float", "max_abs_p"), ("uint32_t", "faces[4]"),
                      ("uint32_t", "nonfinite"), ("uint32_t", "reserved")]
    offsets = {"fx": 0, "fy": 8, "exp2": 16, "max_abs_p": 20, "faces": 24, "nonfinite": 40, "reserved": 44}
    for dtype in (sfl.BODY_LOAD_DTYPE, rule.DTYPE):
        assert dtype.itemsize == 48 and {n: dtype.fields[n][1] for n in dtype.names} == offsets
        assert dtype["faces"].shape == (4,) and dtype["fx"] == np.int64 and dtype["exp2"] == np.int32 and dtype["max_abs_p"] == np.float32
    assert sfl.BODY_LOAD_DTYPE == rule.DTYPE
    assert C.sizeof(sfl.capi.BodyLoad) == 48 and {n: getattr(sfl.capi.BodyLoad, n).offset for n, _ in sfl.capi.BodyLoad._fields_} == offsets
    assert sfl.capi.MAX_BODIES == rule.MAX_BODIES == 16


def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pb, pl, p64 = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_uint8), C.POINTER(cap.BodyLoad), C.POINTER(C.c_int64)
    want = {"sfl_batch_set_bodies": [vp, pb, i, i], "sfl_batch_bodies_info": [vp, pi, pi, pi], "sfl_batch_bodies_download": [vp, i, i, pb, sz],
            "sfl_batch_loads": [vp, i, i, pl, sz], "sfl_batch_loads_start": [vp, i, i, i, i], "sfl_batch_loads_stop": [vp],
            "sfl_batch_loads_info": [vp, pi, pi, p64, pi], "sfl_batch_loads_read": [vp, i, i, pl, sz],
            "sfl_set_bodies": [vp, pb, i], "sfl_bodies_info": [vp, pi, pi], "sfl_bodies_download": [vp, pb, sz], "sfl_loads": [vp, pl, sz],
            "sfl_loads_start": [vp, i, i], "sfl_loads_stop": [vp], "sfl_loads_info": [vp, pi, pi, p64, pi], "sfl_loads_read": [vp, i, i, pl, sz]}
    text = header()
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (i, args), name
        assert re.search(r"SFL_API int %s\(" % name, text), name


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    lib = sfl.capi.lib()
    lab, rec, w = (C.c_uint8 * 12)(), (sfl.capi.BodyLoad * 2)(), C.c_int(5)
    refusals = [
        (lambda: lib.sfl_batch_set_bodies(None, lab, 2, 1), "sfl_batch_set_bodies: per_member must be 0 or 1 (got 2)"),
        (lambda: lib.sfl_batch_set_bodies(None, lab, 0, 0), "sfl_batch_set_bodies: bodies must be 1..16 (got 0)"),
        (lambda: lib.sfl_batch_set_bodies(None, lab, 1, 17), "bodies must be 1..16 (got 17)"),
        (lambda: lib.sfl_batch_set_bodies(None, lab, 0, 16), "sfl_batch_set_bodies: batch is NULL"),
        (lambda: lib.sfl_batch_set_bodies(None, None, 0, 99), "sfl_batch_set_bodies: batch is NULL"),
        (lambda: lib.sfl_batch_bodies_info(None, C.byref(w), None, None), "sfl_batch_bodies_info: batch is NULL"),
        (lambda: lib.sfl_batch_bodies_download(None, 0, 1, lab, 12), "sfl_batch_bodies_download: batch is NULL"),
        (lambda: lib.sfl_batch_loads(None, 0, 1, rec, 48), "sfl_batch_loads: batch is NULL"),
        (lambda: lib.sfl_batch_loads_start(None, 0, 0, 1, 1), "sfl_batch_loads_start: every must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_loads_start(None, 1, 0, 1, -3), "sfl_batch_loads_start: capacity must be >= 1 (got -3)"),
        (lambda: lib.sfl_batch_loads_start(None, 1, 0, 0, 1), "sfl_batch_loads_start: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_loads_start(None, 1, 0, 1, 1), "sfl_batch_loads_start: batch is NULL"),
        (lambda: lib.sfl_batch_loads_stop(None), "sfl_batch_loads_stop: batch is NULL"),
        (lambda: lib.sfl_batch_loads_info(None, C.byref(w), None, None, None), "sfl_batch_loads_info: batch is NULL"),
        (lambda: lib.sfl_batch_loads_read(None, 0, -1, rec, 0), "sfl_batch_loads_read: samples [0, 0 + -1): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_batch_loads_read(None, 0, 1, rec, 48), "sfl_batch_loads_read: batch is NULL"),
        (lambda: lib.sfl_set_bodies(None, lab, 0), "sfl_set_bodies: bodies must be 1..16 (got 0)"),
        (lambda: lib.sfl_set_bodies(None, lab, 2), "sfl_set_bodies: ctx is NULL"),
        (lambda: lib.sfl_bodies_info(None, None, None), "sfl_bodies_info: ctx is NULL"),
        (lambda: lib.sfl_bodies_download(None, lab, 12), "sfl_bodies_download: ctx is NULL"),
        (lambda: lib.sfl_loads(None, rec, 48), "sfl_loads: ctx is NULL"),
        (lambda: lib.sfl_loads_start(None, -1, 1), "sfl_loads_start: every must be >= 1 (got -1)"),
        (lambda: lib.sfl_loads_start(None, 1, 0), "sfl_loads_start: capacity must be >= 1 (got 0)"),
        (lambda: lib.sfl_loads_start(None, 1, 1), "sfl_loads_start: ctx is NULL"),
        (lambda: lib.sfl_loads_stop(None), "sfl_loads_stop: ctx is NULL"),
        (lambda: lib.sfl_loads_info(None, None, None, None, None), "sfl_loads_info: ctx is NULL"),
        (lambda: lib.sfl_loads_read(None, -1, 0, rec, 0), "sfl_loads_read: samples [-1, -1 + 0): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_loads_read(None, 0, 0, rec, 0), "sfl_loads_read: ctx is NULL"),
    ]
    for call, message in refusals:
        assert call() == sfl.capi.ERR_INVALID, message
        assert message in lib.sfl_last_error().decode(), (message, lib.sfl_last_error().decode())
    assert w.value == 5


def test_the_python_front_end_checks_the_labels_before_the_library_sees_them(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks come first)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2

        def __del__(self):
            pass

    with pytest.raises(ValueError, match="shape"):
        Fake().set_bodies(np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError, match="shape"):
        Fake().set_bodies(np.zeros((3, 3, 4), np.uint8))
    with pytest.raises(ValueError, match="uint8"):
        Fake().set_bodies(np.zeros((3, 4), bool))


# ---- the rule's own sanity -------------------------------------------------------------------------------------------------
def disc(dim_x, dim_y, cx, cy, r):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return (i - cx) ** 2 + (j - cy) ** 2 <= r * r


def test_a_body_inside_the_grid_under_a_uniform_pressure_feels_nothing():
    for solid in (disc(33, 18, 16, 9, 5), disc(20, 20, 7, 11, 3) | disc(20, 20, 14, 5, 2)):
        for value in (1.0, -3.7e-5, 2.5e30, 1e-42):
            rec = rule.loads(np.full(solid.shape, value, F), solid)[0]
            assert rec["fx"] == 0 and rec["fy"] == 0, (value, rec)
            assert rec["faces"][rule.W] == rec["faces"][rule.E] > 0 and rec["faces"][rule.S] == rec["faces"][rule.N] > 0
            assert rec["max_abs_p"] == abs(F(value)) and rec["nonfinite"] == 0 and rec["reserved"] == 0


def test_the_sign_and_the_scale():
    """One solid cell at (2, 1) of 5 x 3; its west fluid neighbour (1, 1) holds 3.0: the body is pushed in +x by 3 cell widths."""
    solid = np.zeros((3, 5), bool)
    solid[1, 2] = True
    p = np.zeros((3, 5), F)
    p[1, 1] = 3.0
    rec = rule.loads(p, solid)[0]
    assert list(rec["faces"]) == [1, 1, 1, 1] and rec["exp2"] == 1 - 32 and rec["fx"] == 3 << 31 and rec["fy"] == 0
    assert rule.loads_xy(rec).tolist() == [3.0, 0.0]
    p[:] = 0
    p[2, 2] = -0.75   # the north neighbour: a negative pressure pulls the body towards it, +y
    rec = rule.loads(p, solid)[0]
    assert rec["exp2"] == -1 - 32 and rule.loads_xy(rec).tolist() == [0.0, 0.75] and rec["max_abs_p"] == F(0.75)


def test_label_0_removes_a_wall_from_every_body_and_labels_count_only_where_solid():
    solid = disc(40, 24, 20, 12, 4)
    solid[0:2, :] = solid[-2:, :] = True   # channel walls
    labels = np.zeros(solid.shape, np.uint8)
    labels[disc(40, 24, 20, 12, 4)] = 2
    labels[5, 5] = 1   # a label on a fluid cell: nothing
    p = np.random.default_rng(3).standard_normal(solid.shape).astype(F)
    rec = rule.loads(p, solid, labels, 2)
    alone = rule.loads(p, disc(40, 24, 20, 12, 4))[0]
    assert rec[0].tobytes() == bytes(48), "body 1 has no solid cell"
    assert rec[1].tobytes() == alone.tobytes(), "the walls are in no body"
    everything = rule.loads(p, solid)[0]
    assert everything["faces"].sum() == alone["faces"].sum() + 2 * 40


def test_a_face_to_the_rim_is_not_counted():
    solid = np.zeros((6, 7), bool)
    assert rule.loads(np.ones((6, 7), F), solid)[0].tobytes() == bytes(48), "no solid cell: no face, whatever the rim"
    solid[0, :] = True   # a wall ON the rim: its faces look inward only
    rec = rule.loads(np.ones((6, 7), F), solid)[0]
    assert list(rec["faces"]) == [0, 0, 0, 7] and rec["fy"] == -7 << 32 and rec["fx"] == 0
    solid[:] = True
    assert rule.loads(np.ones((6, 7), F), solid)[0].tobytes() == bytes(48), "all solid: no fluid cell, no face"


def test_nonfinite_faces_are_counted_and_left_out():
    solid = np.zeros((5, 5), bool)
    solid[2, 2] = True
    p = np.ones((5, 5), F)
    clean = rule.loads(p, solid)[0]
    p[2, 1], p[3, 2] = np.nan, -np.inf   # the W and the N face
    p[0, 0] = p[2, 2] = np.nan           # a cell that is not wet and the solid cell itself: no effect
    rec = rule.loads(p, solid)[0]
    assert rec["nonfinite"] == 2 and list(rec["faces"]) == list(clean["faces"]) == [1, 1, 1, 1]
    assert rec["max_abs_p"] == 1.0 and rec["exp2"] == -32 and rec["fx"] == -1 << 32 and rec["fy"] == 1 << 32
    p[:] = np.inf
    rec = rule.loads(p, solid)[0]
    assert rec["nonfinite"] == 4 and rec["max_abs_p"] == 0.0 and rec["exp2"] == 0 and rec["fx"] == 0 and rec["fy"] == 0


def test_a_field_of_denormals_only():
    solid = np.zeros((4, 6), bool)
    solid[1:3, 2:4] = True
    tiny = np.array([1], np.uint32).view(F)[0]   # 2^-149
    p = np.full((4, 6), 0, F)
    p[1, 1], p[2, 1], p[1, 4] = 5 * tiny, 2 * tiny, -3 * tiny   # two W faces, one E face
    rec = rule.loads(p, solid)[0]
    assert rec["max_abs_p"] == 5 * tiny and rec["exp2"] == (2 - 149) - 32
    assert rec["fx"] == (5 + 2 + 3) << 30 and rule.loads_xy(rec)[0] == 10 * float(tiny)


def test_every_face_at_flt_max_does_not_overflow():
    """The header's bound: |t| < 2^33 per face and fewer than 2^30 faces.  Columns fluid (+FLT_MAX), solid, fluid (-FLT_MAX),
    repeated: every face adds +t to fx, nothing cancels, and the sum is exactly faces * t -- which at 2^30 faces is below 2^63."""
    dim_x, dim_y = 63, 8
    solid = np.zeros((dim_y, dim_x), bool)
    solid[:, 1::3] = True
    p = np.zeros((dim_y, dim_x), F)
    p[:, 0::3], p[:, 2::3] = FLT_MAX, -FLT_MAX
    rec = rule.loads(p, solid)[0]
    t = (2 ** 24 - 1) << 9
    assert rule.terms([FLT_MAX], 127 - 32) == [t] and t < 2 ** 33 and 2 ** 30 * t < 2 ** 63
    assert rec["exp2"] == 127 - 32 and rec["max_abs_p"] == FLT_MAX and rec["nonfinite"] == 0
    assert list(rec["faces"]) == [21 * dim_y, 21 * dim_y, 0, 0] and rec["fx"] == 2 * 21 * dim_y * t and rec["fy"] == 0


def test_two_bodies_each_get_their_own_exponent():
    solid = np.zeros((8, 12), bool)
    solid[3, 3] = solid[4, 8] = True
    labels = np.zeros((8, 12), np.uint8)
    labels[3, 3], labels[4, 8] = 1, 3
    p = np.zeros((8, 12), F)
    p[3, 2], p[4, 9] = 1e30, 1e-30
    rec = rule.loads(p, solid, labels, 3)
    assert rec[0]["exp2"] == rule.exponent(F(1e30)) and rec[2]["exp2"] == rule.exponent(F(1e-30)) and rec[1].tobytes() == bytes(48)
    assert rule.loads_xy(rec)[0, 0] == float(F(1e30)) and rule.loads_xy(rec)[2, 0] == -float(F(1e-30))


def test_the_terms_formed_on_the_floats_bits_are_the_rules():
    """csrc/loads.hip forms a term without a double: the mantissa shifted by (exponent - 150) - q, towards zero (exp2_of and
    term_of there).  The same integer arithmetic, restated, against trunc(ldexp((double)p, -q)) on seeded bit patterns of
    every kind: any, denormals only, small and large exponents."""
    def exp2_of(max_bits):
        e = max_bits >> 23
        return 0 if max_bits == 0 else (e - 127 if e else (max_bits.bit_length() - 1) - 149) - 32

    def term_of(bits, q):
        e = (bits >> 23) & 0xFF
        mant = (bits & 0x7FFFFF) | (0x800000 if e else 0)
        shift = (e if e else 1) - 150 - q
        mag = mant << shift if shift >= 0 else (mant >> -shift if shift > -24 else 0)
        return -mag if bits >> 31 else mag

    rng = np.random.default_rng(1)
    checked = 0
    for trial in range(4000):
        n, kind = int(rng.integers(1, 6)), trial % 4
        frac, sign = rng.integers(0, 2 ** 23, n, dtype=np.uint64), rng.integers(0, 2, n, dtype=np.uint64) << 31
        expo = [rng.integers(0, 256, n, dtype=np.uint64), np.zeros(n, np.uint64), rng.integers(1, 40, n, dtype=np.uint64),
                rng.integers(100, 255, n, dtype=np.uint64)][kind]
        bits = (sign | (expo << 23) | frac).astype(np.uint32)
        p = bits.view(F)
        finite = np.isfinite(p)
        if not finite.any():
            continue
        largest = int((bits[finite] & np.uint32(0x7FFFFFFF)).max())
        q = exp2_of(largest)
        assert q == rule.exponent(np.array([largest], np.uint32).view(F)[0])
        assert [term_of(int(b), q) for b in bits[finite]] == rule.terms(p[finite], q)
        checked += 1
    assert checked > 3900


# ---- the host side ---------------------------------------------------------------------------------------------------------
def test_the_host_side_of_the_loads():
    """`make -C tests/cpp -f loads.mk`: tests/cpp/loads_driver.cpp, a stand-alone program (a plain build, no sanitizer).  The
    admission order; loads_admit refusing a call whole; steps counted across calls in both branches of run_steps and in
    sfl_step / sfl_step_n with the fused boundaries kept; samples zero-filled without solids; what the samplers are handed;
    set_bodies refused while recording; with the recorder off the launch log of a step call is the one from before
    loads_start; destroy leaves no allocation."""
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "loads.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, "loads_driver")], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
