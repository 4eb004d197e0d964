"""CPU suite: the friction (include/sfl.h "FRICTION") without a GPU.  The header states the rule and the record, the binding
mirrors it; the argument refusals that need no device, each with its own message, in the loads' order; the sanity of the
rule's numpy restatement (tests/friction_rule.py), which tests/test_friction_gpu.py holds the samplers to; the host side
(csrc/friction.cpp, csrc/body_recorder.h and the hooks in the step calls) run through by tests/cpp/friction_driver.cpp, plain
and under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import friction_rule as rule
import load_rule
from conftest import ROOT

F = np.float32
FLT_MAX = np.finfo(F).max
W, E, S, N = rule.W, rule.E, rule.S, rule.N


def header():
    return open(os.path.join(ROOT, "include", "sfl.h")).read()


def section():
    text = header()
    return text[text.index("--- FRICTION:"):text.index("struct sfl_body_friction {")]


# ---- the header, the struct, the binding ----------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = section()
    for words in ('those of "LOADS", word for word', "S is INSIDE THE DOMAIN", "the rim has no faces", "only where the cell is solid at the time of\n * the sample",
                  "faces[4] of a friction record equals faces[4] of the load record", "THE WALL IS AT REST AND LIES AT NODE S",
                  "nu * (tangential velocity of F) / dx", "the term is v.y and goes into fy", "the term is v.x and goes into fx",
                  "no subtraction between sides", "contributes once per face", "TANGENTIAL component is NaN or +-Inf",
                  "the normal component is not looked at", "0.0f when there is none", "floor(log2(max_abs_t)) - 32", "q = 0 when max_abs_t == 0",
                  "ONE q serves both fx and fy", "(int64_t)trunc(ldexp((double)v_t, -q))", "|t| < 2^33", "SOUTH or NORTH", "WEST or EAST",
                  "Fewer than 2^30 faces", "rho * nu * fx * 2^exp2", "NO FACTOR dx", "does not multiply by nu", "the caller supplies nu",
                  "2 nu dv_n/dn", "no torque", "bit for bit", "The pressure plays no part", "refused WHOLE", "(s + 1) * every",
                  "names the friction recorder", "NOT cut", "history,\n * loads, friction", "while the friction recorder is on"):
        assert words in text, words


def test_the_section_stands_behind_the_inflow_profiles_and_leaves_the_others_alone():
    text = header()
    order = [text.index(w) for w in ("--- LOADS:", "--- VISCOSITY:", "--- OPENINGS:", "--- INFLOW PROFILES AND FLUX", "SFL_API int sfl_batch_openings_flux(",
                                     "--- FRICTION:", "SFL_API int sfl_batch_synchronize(")]
    assert order == sorted(order)
    assert text.count("--- FRICTION:") == 1 and text.count("struct sfl_body_friction {") == 1


def test_the_struct_is_48_bytes_with_the_offsets_of_the_load(sfl):
    text = header()
    body = re.search(r"struct sfl_body_friction \{(.*?)\};", text, re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(\w+)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [("int64_t", "fx"), ("int64_t", "fy"), ("int32_t", "exp2"), ("float", "max_abs_t"), ("uint32_t", "faces[4]"),
                      ("uint32_t", "nonfinite"), ("uint32_t", "reserved")]
    offsets = {"fx": 0, "fy": 8, "exp2": 16, "max_abs_t": 20, "faces": 24, "nonfinite": 40, "reserved": 44}
    for dtype in (sfl.BODY_FRICTION_DTYPE, rule.DTYPE):
        assert dtype.itemsize == 48 and {n: dtype.fields[n][1] for n in dtype.names} == offsets
        assert dtype["faces"].shape == (4,) and dtype["fx"] == np.int64 and dtype["exp2"] == np.int32 and dtype["max_abs_t"] == np.float32
    assert sfl.BODY_FRICTION_DTYPE == rule.DTYPE
    assert C.sizeof(sfl.capi.BodyFriction) == 48 and {n: getattr(sfl.capi.BodyFriction, n).offset for n, _ in sfl.capi.BodyFriction._fields_} == offsets
    load = {n: getattr(sfl.capi.BodyLoad, n).offset for n, _ in sfl.capi.BodyLoad._fields_}
    assert {n.replace("max_abs_p", "max_abs_t"): o for n, o in load.items()} == offsets


def test_the_ten_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pf, p64 = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(cap.BodyFriction), C.POINTER(C.c_int64)
    want = {"sfl_batch_friction": [vp, i, i, pf, sz], "sfl_batch_friction_start": [vp, i, i, i, i], "sfl_batch_friction_stop": [vp],
            "sfl_batch_friction_info": [vp, pi, pi, p64, pi], "sfl_batch_friction_read": [vp, i, i, pf, sz],
            "sfl_friction": [vp, pf, sz], "sfl_friction_start": [vp, i, i], "sfl_friction_stop": [vp], "sfl_friction_info": [vp, pi, pi, p64, pi],
            "sfl_friction_read": [vp, i, i, pf, sz]}
    text = header()
    assert len(want) == 10
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (i, args), name
        assert re.search(r"SFL_API int %s\(" % name, text), name
    for cls in (sfl.Solver, sfl.BatchSolver):
        for method in ("friction", "friction_xy", "friction_start", "friction_info", "friction_history", "friction_history_xy", "friction_stop"):
            assert callable(getattr(cls, method)), (cls, method)


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message_in_the_loads_order(sfl):
    lib = sfl.capi.lib()
    rec, lrec, w = (sfl.capi.BodyFriction * 2)(), (sfl.capi.BodyLoad * 2)(), C.c_int(5)
    refusals = [
        (lambda: lib.sfl_batch_friction(None, 0, 1, rec, 48), "sfl_batch_friction: batch is NULL"),
        (lambda: lib.sfl_batch_friction_start(None, 0, 0, 1, 1), "sfl_batch_friction_start: every must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_friction_start(None, 1, 0, 1, -3), "sfl_batch_friction_start: capacity must be >= 1 (got -3)"),
        (lambda: lib.sfl_batch_friction_start(None, 1, 0, 0, 1), "sfl_batch_friction_start: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_friction_start(None, 1, 0, 1, 1), "sfl_batch_friction_start: batch is NULL"),
        (lambda: lib.sfl_batch_friction_stop(None), "sfl_batch_friction_stop: batch is NULL"),
        (lambda: lib.sfl_batch_friction_info(None, C.byref(w), None, None, None), "sfl_batch_friction_info: batch is NULL"),
        (lambda: lib.sfl_batch_friction_read(None, 0, -1, rec, 0), "sfl_batch_friction_read: samples [0, 0 + -1): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_batch_friction_read(None, 0, 1, rec, 48), "sfl_batch_friction_read: batch is NULL"),
        (lambda: lib.sfl_friction(None, rec, 48), "sfl_friction: ctx is NULL"),
        (lambda: lib.sfl_friction_start(None, -1, 1), "sfl_friction_start: every must be >= 1 (got -1)"),
        (lambda: lib.sfl_friction_start(None, 1, 0), "sfl_friction_start: capacity must be >= 1 (got 0)"),
        (lambda: lib.sfl_friction_start(None, 1, 1), "sfl_friction_start: ctx is NULL"),
        (lambda: lib.sfl_friction_stop(None), "sfl_friction_stop: ctx is NULL"),
        (lambda: lib.sfl_friction_info(None, None, None, None, None), "sfl_friction_info: ctx is NULL"),
        (lambda: lib.sfl_friction_read(None, -1, 0, rec, 0), "sfl_friction_read: samples [-1, -1 + 0): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_friction_read(None, 0, 0, rec, 0), "sfl_friction_read: ctx is NULL"),
    ]
    for call, message in refusals:
        assert call() == sfl.capi.ERR_INVALID, message
        assert message in lib.sfl_last_error().decode(), (message, lib.sfl_last_error().decode())
    assert w.value == 5
    # the order is the loads': the same arguments, the same refusal, the call's name exchanged
    pairs = [(lambda: lib.sfl_batch_loads_start(None, 0, 0, 0, 0), lambda: lib.sfl_batch_friction_start(None, 0, 0, 0, 0)),
             (lambda: lib.sfl_batch_loads_start(None, 1, 0, 0, 0), lambda: lib.sfl_batch_friction_start(None, 1, 0, 0, 0)),
             (lambda: lib.sfl_batch_loads_read(None, -1, -1, lrec, 7), lambda: lib.sfl_batch_friction_read(None, -1, -1, rec, 7)),
             (lambda: lib.sfl_loads_start(None, 0, 0), lambda: lib.sfl_friction_start(None, 0, 0)),
             (lambda: lib.sfl_loads(None, lrec, 1), lambda: lib.sfl_friction(None, rec, 1))]
    for loads_call, friction_call in pairs:
        assert loads_call() == friction_call()
        said = lib.sfl_last_error().decode()
        loads_call()
        assert said == lib.sfl_last_error().decode().replace("loads", "friction")


def test_the_python_front_end_checks_nu_before_the_library_sees_it(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the check of nu's shape needs neither)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 5

        def __del__(self):
            pass

    fake = Fake()
    assert fake._friction_nu(0.25, 0, 5).shape == () and fake._friction_nu(np.arange(5.0), 0, 5).shape == (5, 1, 1)
    with pytest.raises(ValueError, match="nu of shape"):
        fake._friction_nu(np.zeros(4), 0, 5)


# ---- the rule's own sanity -------------------------------------------------------------------------------------------------
def disc(dim_x, dim_y, cx, cy, r):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return (i - cx) ** 2 + (j - cy) ** 2 <= r * r


def block(dim_x, dim_y, i0, j0, w, h):
    solid = np.zeros((dim_y, dim_x), bool)
    solid[j0:j0 + h, i0:i0 + w] = True
    return solid


def stream(shape, u, v=0.0):
    out = np.empty(shape + (2,), F)
    out[..., 0], out[..., 1] = u, v
    return out


def test_fluid_at_rest_gives_zero_sums_with_the_faces_counted():
    for solid in (disc(33, 18, 16, 9, 5), disc(20, 20, 7, 11, 3) | disc(20, 20, 14, 5, 2)):
        rec = rule.friction(np.zeros(solid.shape + (2,), F), solid)[0]
        assert rec["fx"] == 0 and rec["fy"] == 0 and rec["exp2"] == 0 and rec["max_abs_t"] == 0 and rec["nonfinite"] == 0 and rec["reserved"] == 0
        assert rec["faces"][W] == rec["faces"][E] > 0 and rec["faces"][S] == rec["faces"][N] > 0


@pytest.mark.parametrize("w,h", [(1, 1), (5, 2), (3, 7)])
@pytest.mark.parametrize("u", [1.0, 0.75, 3.0e-5, 1.5e30])
def test_a_uniform_stream_past_a_block_drags_it_by_two_widths(w, h, u):
    """(U, 0) past a w x h block: the w faces below and the w above each add U to fx; the side faces see v.y = 0."""
    solid = block(20, 16, 6, 4, w, h)
    rec = rule.friction(stream(solid.shape, u), solid)[0]
    assert list(rec["faces"]) == [h, h, w, w] and rec["fy"] == 0 and rec["nonfinite"] == 0 and rec["max_abs_t"] == F(u)
    assert float(rule.friction_xy(rec, 1.0)[0]) == 2 * w * float(F(u)) and rec["fx"] * 2.0 ** int(rec["exp2"]) == 2 * w * float(F(u))
    back = rule.friction(stream(solid.shape, -u), solid)[0]
    assert back["fx"] == -rec["fx"] and back["fy"] == 0 and back["exp2"] == rec["exp2"] and list(back["faces"]) == list(rec["faces"])
    # the transposed grid in the transposed stream (0, U): fx and fy change places, and so do the W, E and the S, N counts
    turned = rule.friction(stream((20, 16), 0.0, u), solid.T)[0]
    assert turned["fy"] == rec["fx"] and turned["fx"] == 0 and turned["exp2"] == rec["exp2"] and list(turned["faces"]) == [w, w, h, h]
    assert rule.friction_xy(rec, 0.5).tolist() == [w * float(F(u)), 0.0], "nu scales the figure; no dx anywhere"


def test_the_faces_are_the_loads_faces_for_seeded_masks_and_labels():
    rng = np.random.default_rng(11)
    for trial in range(40):
        dim_x, dim_y, bodies = int(rng.integers(2, 24)), int(rng.integers(2, 24)), int(rng.integers(1, 17))
        solid = rng.random((dim_y, dim_x)) < rng.choice([0.1, 0.4, 0.8])
        labels = None if trial % 5 == 0 else rng.integers(0, bodies + 1, (dim_y, dim_x)).astype(np.uint8)
        bodies = 1 if labels is None else bodies
        v = rng.standard_normal((dim_y, dim_x, 2)).astype(F)
        p = rng.standard_normal((dim_y, dim_x)).astype(F)
        assert rule.friction(v, solid, labels, bodies)["faces"].tolist() == load_rule.loads(p, solid, labels, bodies)["faces"].tolist()


def test_label_0_removes_a_wall_from_every_body_and_labels_count_only_where_solid():
    solid = disc(40, 24, 20, 12, 4)
    solid[0:2, :] = solid[-2:, :] = True   # channel walls
    labels = np.zeros(solid.shape, np.uint8)
    labels[disc(40, 24, 20, 12, 4)] = 2
    labels[5, 5] = 1   # a label on a fluid cell: nothing
    v = np.random.default_rng(3).standard_normal(solid.shape + (2,)).astype(F)
    rec = rule.friction(v, solid, labels, 2)
    alone = rule.friction(v, disc(40, 24, 20, 12, 4))[0]
    assert rec[0].tobytes() == bytes(48), "body 1 has no solid cell"
    assert rec[1].tobytes() == alone.tobytes(), "the walls are in no body"
    everything = rule.friction(v, solid)[0]
    assert everything["faces"].sum() == alone["faces"].sum() + 2 * 40


def test_a_face_to_the_rim_is_not_counted():
    solid = np.zeros((6, 7), bool)
    assert rule.friction(stream((6, 7), 1.0, 1.0), solid)[0].tobytes() == bytes(48), "no solid cell: no face, whatever the rim"
    solid[0, :] = True   # a wall ON the rim: its faces look inward only
    rec = rule.friction(stream((6, 7), 1.0, 5.0), solid)[0]
    assert list(rec["faces"]) == [0, 0, 0, 7] and rec["fx"] == 7 << 32 and rec["fy"] == 0 and rec["max_abs_t"] == 1.0
    solid[:] = True
    assert rule.friction(stream((6, 7), 1.0, 1.0), solid)[0].tobytes() == bytes(48), "all solid: no fluid cell, no face"


def test_a_nan_in_the_normal_component_changes_nothing_and_one_in_the_tangential_is_counted_and_left_out():
    solid = np.zeros((5, 5), bool)
    solid[2, 2] = True
    v = stream((5, 5), 1.0, -2.0)
    clean = rule.friction(v, solid)[0]
    assert list(clean["faces"]) == [1, 1, 1, 1] and clean["max_abs_t"] == 2.0 and clean["exp2"] == 1 - 32
    assert clean["fx"] == 2 << 31 and clean["fy"] == -(4 << 31)
    v[2, 1, 0] = v[2, 3, 0] = np.nan      # the W and E faces slide along y: x is their NORMAL component
    v[1, 2, 1] = v[3, 2, 1] = -np.inf     # the S and N faces slide along x: y is theirs
    v[0, 0] = v[2, 2] = np.nan            # a cell that is not wet and the solid cell itself
    assert rule.friction(v, solid)[0].tobytes() == clean.tobytes()
    v[2, 1, 1], v[3, 2, 0] = np.nan, np.inf   # the W face's and the N face's TANGENTIAL components
    rec = rule.friction(v, solid)[0]
    assert rec["nonfinite"] == 2 and list(rec["faces"]) == [1, 1, 1, 1]
    assert rec["max_abs_t"] == 2.0 and rec["exp2"] == 1 - 32 and rec["fx"] == 1 << 31 and rec["fy"] == -(2 << 31)
    v[:] = np.inf
    rec = rule.friction(v, solid)[0]
    assert rec["nonfinite"] == 4 and rec["max_abs_t"] == 0.0 and rec["exp2"] == 0 and rec["fx"] == 0 and rec["fy"] == 0


def test_a_field_of_denormals_only():
    solid = block(6, 4, 2, 1, 2, 2)
    tiny = np.array([1], np.uint32).view(F)[0]   # 2^-149
    v = np.zeros((4, 6, 2), F)
    v[1, 1, 1], v[2, 1, 1], v[1, 4, 1] = 5 * tiny, 2 * tiny, -3 * tiny   # two W faces, one E face: along y
    v[0, 2, 0] = 4 * tiny                                                  # one S face: along x
    v[0, 3, 1] = 7 * tiny                                                  # ... whose neighbour's NORMAL component is larger: ignored
    rec = rule.friction(v, solid)[0]
    assert rec["max_abs_t"] == 5 * tiny and rec["exp2"] == (2 - 149) - 32
    assert rec["fy"] == (5 + 2 - 3) << 30 and rec["fx"] == 4 << 30 and rule.friction_xy(rec, 1.0).tolist() == [4 * float(tiny), 4 * float(tiny)]


def test_every_face_at_flt_max_does_not_overflow():
    """The header's bound: |t| < 2^33 per face and fewer than 2^30 faces.  Rows fluid, solid, fluid, repeated, every fluid cell at
    (+FLT_MAX, .): every face adds +t to fx, nothing cancels, and the sum is exactly faces * t -- at 2^30 faces below 2^63."""
    dim_x, dim_y = 8, 63
    solid = np.zeros((dim_y, dim_x), bool)
    solid[1::3, :] = True
    v = stream((dim_y, dim_x), FLT_MAX, -FLT_MAX)
    rec = rule.friction(v, solid)[0]
    t = (2 ** 24 - 1) << 9
    assert load_rule.terms([FLT_MAX], 127 - 32) == [t] and t < 2 ** 33 and 2 ** 30 * t < 2 ** 63
    assert rec["exp2"] == 127 - 32 and rec["max_abs_t"] == FLT_MAX and rec["nonfinite"] == 0
    assert list(rec["faces"]) == [0, 0, 21 * dim_x, 21 * dim_x] and rec["fx"] == 2 * 21 * dim_x * t and rec["fy"] == 0


def test_two_bodies_each_get_their_own_exponent():
    solid = np.zeros((8, 12), bool)
    solid[3, 3] = solid[4, 8] = True
    labels = np.zeros((8, 12), np.uint8)
    labels[3, 3], labels[4, 8] = 1, 3
    v = np.zeros((8, 12, 2), F)
    v[3, 2, 1], v[5, 8, 0] = 1e30, -1e-30   # body 1's W face along y, body 3's N face along x
    rec = rule.friction(v, solid, labels, 3)
    assert rec[0]["exp2"] == load_rule.exponent(F(1e30)) and rec[2]["exp2"] == load_rule.exponent(F(1e-30)) and rec[1].tobytes() == bytes(48)
    xy = rule.friction_xy(rec, 1.0)
    assert xy[0].tolist() == [0.0, float(F(1e30))] and xy[2].tolist() == [-float(F(1e-30)), 0.0]


def test_a_cell_between_two_solid_cells_of_one_body_counts_twice_and_a_corner_cell_feeds_both_sums():
    solid = np.zeros((5, 7), bool)
    solid[2, 2] = solid[2, 4] = True      # fluid (3, 2) lies E of the one and W of the other
    v = np.zeros((5, 7, 2), F)
    v[2, 3] = (9.0, 3.0)
    rec = rule.friction(v, solid)[0]
    assert list(rec["faces"]) == [2, 2, 2, 2] and rec["max_abs_t"] == 3.0 and rule.friction_xy(rec, 1.0).tolist() == [0.0, 6.0]
    labels = np.zeros((5, 7), np.uint8)
    labels[2, 2], labels[2, 4] = 1, 2     # ... of two bodies: once each
    rec = rule.friction(v, solid, labels, 2)
    assert rule.friction_xy(rec, 1.0).tolist() == [[0.0, 3.0], [0.0, 3.0]]
    corner = np.zeros((5, 7), bool)
    corner[2, 2] = corner[1, 3] = True    # fluid (3, 2) lies E of (2, 2) and N of (3, 1): .y into fy, .x into fx, one q
    rec = rule.friction(v, corner)[0]
    assert rec["max_abs_t"] == 9.0 and rec["exp2"] == 3 - 32 and rule.friction_xy(rec, 1.0).tolist() == [9.0, 3.0]


def test_the_pressure_plays_no_part():
    """The rule takes no pressure at all: friction(v, ...) has no such argument, and the loads' record of the same grid moves
    with p while the friction's bytes stay.  tests/test_friction_gpu.py repeats this on the device, where a pressure is held."""
    rng = np.random.default_rng(5)
    solid = disc(24, 20, 11, 9, 4)
    v = rng.standard_normal((20, 24, 2)).astype(F)
    p1, p2 = rng.standard_normal((20, 24)).astype(F), rng.standard_normal((20, 24)).astype(F)
    assert load_rule.loads(p1, solid).tobytes() != load_rule.loads(p2, solid).tobytes()
    assert rule.friction(v, solid).tobytes() == rule.friction(v.copy(), solid).tobytes()
    import inspect
    assert list(inspect.signature(rule.friction).parameters) == ["v", "solid", "labels", "bodies"]


# ---- the host side ---------------------------------------------------------------------------------------------------------
def build_and_run(target, program):
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "friction.mk", "-j4", target], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


def test_the_host_side_of_the_friction():
    """`make -C tests/cpp -f friction.mk`: tests/cpp/friction_driver.cpp, a stand-alone program.  Admission at all five points;
    a refusal leaves the steps and the recorder untouched; zero-filled samples inside a one-launch replay and across the seams,
    neither cut; history, loads, friction in the launch log; no friction recorder: the log of the null pointer; set_bodies
    refused while either recorder is on, each with its message; destroy leaves no allocation."""
    build_and_run("all", "friction_driver")


def test_the_host_side_of_the_friction_under_asan_and_ubsan():
    """The same stand-alone program, every unit compiled with -fsanitize=address,undefined, run directly."""
    build_and_run("san", "friction_driver_san")
