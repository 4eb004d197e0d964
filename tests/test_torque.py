"""CPU suite: the torque (include/sfl.h "TORQUE") without a GPU.  The header states the rule and the record, the binding
mirrors it; the argument refusals that need no device, each with its own message, in the loads' order; the sanity of the
rule's numpy restatement (tests/torque_rule.py), which tests/test_torque_gpu.py holds the samplers to -- the identity with
tests/load_rule.py and tests/friction_rule.py under a move of the pivot, the shift s where faces times arm would overflow and
the boundary where it is still 0; csrc/torque_face.h run face by face on the host against the rule, through a file; the
host side (csrc/torque.cpp, csrc/body_recorder.h and the hooks in the step calls) run through by tests/cpp/torque_driver.cpp,
plain and under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import friction_rule
import load_rule
import torque_rule as rule
from conftest import ROOT

F = np.float32
FLT_MAX = np.finfo(F).max
W, E, S, N = rule.W, rule.E, rule.S, rule.N


def header():
    return open(os.path.join(ROOT, "include", "sfl.h")).read()


def section():
    text = header()
    return text[text.index("--- TORQUE:"):text.index("struct sfl_body_torque {")]


# ---- the header, the struct, the binding ----------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = section()
    for words in ('those of "LOADS", word for word', "S is INSIDE THE DOMAIN", "the rim has no faces", "COUNTER-CLOCKWISE POSITIVE", "ACT AT NODE S",
                  "HALF cell widths", "(pivot2[0] / 2, pivot2[1] / 2)", "SFL_TORQUE_MAX_PIVOT2 = 2^24", "Without pivots every pivot is\n * (0, 0)",
                  "rx2 = 2 * iS - pivot2[0] and ry2 = 2 * jS - pivot2[1], in int32", "non-finite ones included", "max(|rx2|, |ry2|)",
                  "s = max(0, L(faces) + L(max_arm2) - 30)", "q_p + s and q_f + s", "(int64_t)trunc(ldexp((double)p, -exp2_p))", "|t| < 2^(33 - s)",
                  "-ry2 * tp for dir 0, +ry2 * tp for dir 1, +rx2 * tp for dir 2 and -rx2 * tp for dir 3",
                  "+rx2 * tf for dir 0 and 1 (tf from v.y) and -ry2 * tf for dir 2 and 3 (tf from v.x)", "rx * Fy - ry * Fx",
                  "|sum| < 2^(33 - s + L(max_arm2) + L(faces)) <= 2^63", "mp * 2^(exp2_p - 1)", "rho * nu * mf * 2^(exp2_f - 1) * dx",
                  "-(a2 * fy - b2 * fx)", "pivot2 is still\n * filled in", "bit\n * for bit", "refused\n * WHOLE", "names the torque recorder",
                  "(s + 1) * every", "NOT cut", "history, loads, friction, torque", "while the torque recorder is on", "as from sfl_loads"):
        assert words in text, words


def test_the_section_stands_behind_the_averages_and_leaves_the_others_alone():
    text = header()
    order = [text.index(w) for w in ("--- LOADS:", "--- FRICTION:", "--- AVERAGES:", "SFL_API int sfl_batch_mean_download(", "--- TORQUE:",
                                     "SFL_API int sfl_torque_read(", "SFL_API int sfl_batch_synchronize(")]
    assert order == sorted(order)
    assert text.count("--- TORQUE:") == 1 and text.count("struct sfl_body_torque {") == 1 and "#define SFL_TORQUE_MAX_PIVOT2 16777216" in text


OFFSETS = {"mp": 0, "mf": 8, "exp2_p": 16, "exp2_f": 20, "max_abs_p": 24, "max_abs_t": 28, "faces": 32, "max_arm2": 36, "nonfinite_p": 40,
           "nonfinite_t": 44, "pivot2": 48, "reserved": 56}


def test_the_struct_is_64_bytes_with_the_issues_offsets(sfl):
    body = re.search(r"struct sfl_body_torque \{(.*?)\};", header(), re.S).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(\w+)\s+([^;]+);", body) for n in names.split(",")]
    assert fields == [("int64_t", "mp"), ("int64_t", "mf"), ("int32_t", "exp2_p"), ("int32_t", "exp2_f"), ("float", "max_abs_p"), ("float", "max_abs_t"),
                      ("uint32_t", "faces"), ("uint32_t", "max_arm2"), ("uint32_t", "nonfinite_p"), ("uint32_t", "nonfinite_t"), ("int32_t", "pivot2[2]"),
                      ("uint32_t", "reserved[2]")]
    for dtype in (sfl.BODY_TORQUE_DTYPE, rule.DTYPE):
        assert dtype.itemsize == 64 and {n: dtype.fields[n][1] for n in dtype.names} == OFFSETS
        assert dtype["pivot2"].shape == (2,) and dtype["pivot2"].base == np.int32 and dtype["mp"] == np.int64 and dtype["max_abs_t"] == np.float32
    assert sfl.BODY_TORQUE_DTYPE == rule.DTYPE
    assert C.sizeof(sfl.capi.BodyTorque) == 64 and {n: getattr(sfl.capi.BodyTorque, n).offset for n, _ in sfl.capi.BodyTorque._fields_} == OFFSETS


def test_the_fourteen_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, pt, p64, p32 = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(cap.BodyTorque), C.POINTER(C.c_int64), C.POINTER(C.c_int32)
    want = {"sfl_batch_set_body_pivots": [vp, p32, i, i], "sfl_batch_body_pivots_download": [vp, i, i, p32, sz], "sfl_batch_torque": [vp, i, i, pt, sz],
            "sfl_batch_torque_start": [vp, i, i, i, i], "sfl_batch_torque_stop": [vp], "sfl_batch_torque_info": [vp, pi, pi, p64, pi],
            "sfl_batch_torque_read": [vp, i, i, pt, sz], "sfl_set_body_pivots": [vp, p32, i], "sfl_body_pivots_download": [vp, p32, sz],
            "sfl_torque": [vp, pt, sz], "sfl_torque_start": [vp, i, i], "sfl_torque_stop": [vp], "sfl_torque_info": [vp, pi, pi, p64, pi],
            "sfl_torque_read": [vp, i, i, pt, sz]}
    text = header()
    assert len(want) == 14
    for name, args in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (i, args), name
        assert re.search(r"SFL_API int %s\(" % name, text), name
    for cls in (sfl.Solver, sfl.BatchSolver):
        for method in ("set_body_pivots", "body_pivots", "torque", "torque_xy", "torque_start", "torque_info", "torque_history", "torque_stop"):
            assert callable(getattr(cls, method)), (cls, method)


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message_in_the_loads_order(sfl):
    lib = sfl.capi.lib()
    rec, lrec, w, piv = (sfl.capi.BodyTorque * 2)(), (sfl.capi.BodyLoad * 2)(), C.c_int(5), (C.c_int32 * 2)()
    refusals = [
        (lambda: lib.sfl_batch_torque(None, 0, 1, rec, 64), "sfl_batch_torque: batch is NULL"),
        (lambda: lib.sfl_batch_torque_start(None, 0, 0, 1, 1), "sfl_batch_torque_start: every must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_torque_start(None, 1, 0, 1, -3), "sfl_batch_torque_start: capacity must be >= 1 (got -3)"),
        (lambda: lib.sfl_batch_torque_start(None, 1, 0, 0, 1), "sfl_batch_torque_start: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_torque_start(None, 1, 0, 1, 1), "sfl_batch_torque_start: batch is NULL"),
        (lambda: lib.sfl_batch_torque_stop(None), "sfl_batch_torque_stop: batch is NULL"),
        (lambda: lib.sfl_batch_torque_info(None, C.byref(w), None, None, None), "sfl_batch_torque_info: batch is NULL"),
        (lambda: lib.sfl_batch_torque_read(None, 0, -1, rec, 0), "sfl_batch_torque_read: samples [0, 0 + -1): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_batch_torque_read(None, 0, 1, rec, 64), "sfl_batch_torque_read: batch is NULL"),
        (lambda: lib.sfl_torque(None, rec, 64), "sfl_torque: ctx is NULL"),
        (lambda: lib.sfl_torque_start(None, -1, 1), "sfl_torque_start: every must be >= 1 (got -1)"),
        (lambda: lib.sfl_torque_start(None, 1, 0), "sfl_torque_start: capacity must be >= 1 (got 0)"),
        (lambda: lib.sfl_torque_start(None, 1, 1), "sfl_torque_start: ctx is NULL"),
        (lambda: lib.sfl_torque_stop(None), "sfl_torque_stop: ctx is NULL"),
        (lambda: lib.sfl_torque_info(None, None, None, None, None), "sfl_torque_info: ctx is NULL"),
        (lambda: lib.sfl_torque_read(None, -1, 0, rec, 0), "sfl_torque_read: samples [-1, -1 + 0): first_sample and samples must be >= 0"),
        (lambda: lib.sfl_torque_read(None, 0, 0, rec, 0), "sfl_torque_read: ctx is NULL"),
        (lambda: lib.sfl_batch_set_body_pivots(None, piv, 3, 1), "sfl_batch_set_body_pivots: per_member must be 0 or 1 (got 3)"),
        (lambda: lib.sfl_batch_set_body_pivots(None, piv, 1, 1), "sfl_batch_set_body_pivots: batch is NULL"),
        (lambda: lib.sfl_batch_body_pivots_download(None, 0, 1, piv, 8), "sfl_batch_body_pivots_download: batch is NULL"),
        (lambda: lib.sfl_set_body_pivots(None, piv, 1), "sfl_set_body_pivots: ctx is NULL"),
        (lambda: lib.sfl_body_pivots_download(None, piv, 8), "sfl_body_pivots_download: ctx is NULL"),
    ]
    for call, message in refusals:
        assert call() == sfl.capi.ERR_INVALID, message
        assert message in lib.sfl_last_error().decode(), (message, lib.sfl_last_error().decode())
    assert w.value == 5
    # the order is the loads': the same arguments, the same refusal, the call's name exchanged
    pairs = [(lambda: lib.sfl_batch_loads_start(None, 0, 0, 0, 0), lambda: lib.sfl_batch_torque_start(None, 0, 0, 0, 0)),
             (lambda: lib.sfl_batch_loads_start(None, 1, 0, 0, 0), lambda: lib.sfl_batch_torque_start(None, 1, 0, 0, 0)),
             (lambda: lib.sfl_batch_loads_read(None, -1, -1, lrec, 7), lambda: lib.sfl_batch_torque_read(None, -1, -1, rec, 7)),
             (lambda: lib.sfl_loads_start(None, 0, 0), lambda: lib.sfl_torque_start(None, 0, 0)),
             (lambda: lib.sfl_loads(None, lrec, 1), lambda: lib.sfl_torque(None, rec, 1))]
    for loads_call, torque_call in pairs:
        assert loads_call() == torque_call()
        said = lib.sfl_last_error().decode()
        loads_call()
        assert said == lib.sfl_last_error().decode().replace("loads", "torque")


def test_the_python_front_end_takes_pivots_in_multiples_of_half_a_cell(sfl):
    sent = []

    class Fake(sfl.BatchSolver):
        def __init__(self):   # (no library, no device: the checks of the pivots need neither)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 5

        def __del__(self):
            pass

        def bodies_info(self):
            return (2, True, False)

        def _loads_call(self, name):
            def call(h, ptr, *args):
                n = 2 * 2 * (5 if args[0] else 1)
                sent.append((name, np.ctypeslib.as_array(ptr, (n,)).copy().tolist() if ptr else None, args))
                return sfl.capi.OK
            return call

    fake = Fake()
    fake.set_body_pivots([[1.5, -2.0], [0.0, 8388608.0]])
    assert sent[-1] == ("set_body_pivots", [3, -4, 0, 16777216], (0, 2))
    fake.set_body_pivots(np.full((5, 2, 2), 0.5))
    assert sent[-1] == ("set_body_pivots", [1] * 20, (1, 2))
    fake.set_body_pivots(None)
    assert sent[-1] == ("set_body_pivots", None, (0, 1))
    for bad, words in (([[0.25, 0.0], [0.0, 0.0]], "multiple of 0.5"), ([[np.nan, 0.0], [0.0, 0.0]], "multiple of 0.5"), ([[0.0, 0.0]], "shape"),
                       (np.zeros((4, 2, 2)), "shape")):
        with pytest.raises(ValueError, match=words):
            fake.set_body_pivots(bad)
    assert len(sent) == 3


# ---- the rule's own sanity -------------------------------------------------------------------------------------------------
def disc(dim_x, dim_y, cx, cy, r):
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    return (i - cx) ** 2 + (j - cy) ** 2 <= r * r


def block(dim_x, dim_y, i0, j0, w, h):
    solid = np.zeros((dim_y, dim_x), bool)
    solid[j0:j0 + h, i0:i0 + w] = True
    return solid


def test_L_and_s():
    assert [rule.bit_length(x) for x in (0, 1, 2, 3, 4, 255, 256, 2 ** 24, 2 ** 32 - 1)] == [0, 1, 2, 2, 3, 8, 9, 25, 32]
    assert rule.shift(0, 0) == 0 and rule.shift(2 ** 15 - 1, 2 ** 15 - 1) == 0 and rule.shift(2 ** 15, 2 ** 15 - 1) == 1 and rule.shift(2 ** 30 - 1, 2 ** 30 - 1) == 30


def test_one_solid_cell_by_hand():
    """Solid (3, 2) in 7 x 5, pivot at its own node: the four faces act AT THE NODE, so every arm is zero and so are both sums;
    from the pivot (0, 0) the arms are (6, 4) doubled."""
    solid = block(7, 5, 3, 2, 1, 1)
    p = np.zeros((5, 7), F)
    v = np.zeros((5, 7, 2), F)
    p[2, 2], p[2, 4], p[1, 3], p[3, 3] = 1.0, 0.5, 0.25, 0.125           # the fluid cells W, E, S, N of it
    v[2, 2, 1], v[2, 4, 1], v[1, 3, 0], v[3, 3, 0] = 1.0, -0.5, 0.25, 0.125
    own = rule.torque(p, v, solid, None, 1, [[6, 4]])[0]
    assert own["faces"] == 4 and own["max_arm2"] == 0 and own["mp"] == 0 and own["mf"] == 0 and list(own["pivot2"]) == [6, 4]
    assert own["exp2_p"] == -32 and own["exp2_f"] == -32 and own["max_abs_p"] == 1.0 and own["max_abs_t"] == 1.0
    rec = rule.torque(p, v, solid)[0]
    one = 1 << 32
    # rx2 = 6, ry2 = 4 for every face: mp = -4 * 1 + 4 * 0.5 + 6 * 0.25 - 6 * 0.125; mf = 6 * (1 - 0.5) - 4 * (0.25 + 0.125)
    assert rec["max_arm2"] == 6 and rec["mp"] == int((-4 + 2 + 1.5 - 0.75) * one) and rec["mf"] == int((3 - 1.5) * one)
    assert rule.torque_xy(rec).tolist() == [(-4 + 2 + 1.5 - 0.75) / 2, (3 - 1.5) / 2], "the arms are doubled: 2^(exp2 - 1)"
    assert rule.torque_xy(rec, dx=0.5, rho=3.0, nu=0.1).tolist() == [-1.25 / 2 * 0.25, 1.5 / 2 * 0.1 * (3.0 * 0.5)]


def test_a_uniform_pressure_turns_nothing_and_a_shear_turns_a_block_counter_clockwise():
    solid = block(20, 16, 6, 4, 4, 3)
    centre2 = [[2 * 6 + 3, 2 * 4 + 2]]   # (7.5, 5.0): the centre of the nodes 6..9 x 4..6
    p = np.full((16, 20), 3.0, F)
    v = np.zeros((16, 20, 2), F)
    v[3, :, 0], v[7, :, 0] = 1.0, -1.0     # below the block to the right, above it to the left: counter-clockwise
    for piv in (centre2, None, [[-7, 100]]):
        rec = rule.torque(p, v, solid, None, 1, piv)[0]
        assert rec["mp"] == 0, "a closed body in a uniform pressure: no moment about any pivot"
    rec = rule.torque(p, v, solid, None, 1, centre2)[0]
    assert rec["faces"] == 14 and rec["mf"] > 0 and rule.torque_xy(rec)[1] == 2 * 4 * 1.0, "4 faces below and 4 above, arm 1 each"


def test_moving_the_pivot_changes_the_sums_by_the_load_and_the_friction_records():
    rng = np.random.default_rng(12)
    for trial in range(25):
        dim_x, dim_y, bodies = int(rng.integers(3, 24)), int(rng.integers(3, 24)), int(rng.integers(1, 17))
        solid = rng.random((dim_y, dim_x)) < rng.choice([0.1, 0.4, 0.8])
        labels = None if trial % 5 == 0 else rng.integers(0, bodies + 1, (dim_y, dim_x)).astype(np.uint8)
        bodies = 1 if labels is None else bodies
        p = (rng.standard_normal((dim_y, dim_x)) * 10.0 ** rng.integers(-30, 30)).astype(F)
        v = (rng.standard_normal((dim_y, dim_x, 2)) * 10.0 ** rng.integers(-30, 30)).astype(F)
        if trial % 3 == 0:
            p[rng.random(p.shape) < 0.1] = np.nan
            v[rng.random(v.shape) < 0.1] = np.inf
        at = rng.integers(-60, 60, (bodies, 2))
        move = rng.integers(-(1 << 16), 1 << 16, (bodies, 2))
        first, second = rule.torque(p, v, solid, labels, bodies, at), rule.torque(p, v, solid, labels, bodies, at + move)
        loads, friction = load_rule.loads(p, solid, labels, bodies), friction_rule.friction(v, solid, labels, bodies)
        for k in range(bodies):
            a2, b2 = int(move[k, 0]), int(move[k, 1])
            assert first[k]["exp2_p"] == second[k]["exp2_p"] == loads[k]["exp2"] and first[k]["exp2_f"] == friction[k]["exp2"], "s = 0: the terms are the records'"
            assert first[k]["faces"] == loads[k]["faces"].sum() == friction[k]["faces"].sum()
            assert first[k]["nonfinite_p"] == loads[k]["nonfinite"] and first[k]["nonfinite_t"] == friction[k]["nonfinite"]
            assert first[k]["max_abs_p"] == loads[k]["max_abs_p"] and first[k]["max_abs_t"] == friction[k]["max_abs_t"]
            assert int(second[k]["mp"]) - int(first[k]["mp"]) == -(a2 * int(loads[k]["fy"]) - b2 * int(loads[k]["fx"]))
            assert int(second[k]["mf"]) - int(first[k]["mf"]) == -(a2 * int(friction[k]["fy"]) - b2 * int(friction[k]["fx"]))


def checkerboard():
    j, i = np.mgrid[0:9, 0:9]
    return (i + j) % 2 == 1


def test_the_exponents_are_raised_where_faces_times_arm_would_overflow():
    """9 x 9, every other cell solid, pivot2 = (2^24, -2^24), every face at +-FLT_MAX: with s = 0 the sum would need more than 63
    bits; the rule (which asserts the header's bound itself) raises both exponents by s."""
    solid = checkerboard()
    piv = [[1 << 24, -(1 << 24)]]
    p = np.full((9, 9), FLT_MAX, F)
    v = np.full((9, 9, 2), -FLT_MAX, F)
    rec = rule.torque(p, v, solid, None, 1, piv)[0]
    faces, arm = int(rec["faces"]), int(rec["max_arm2"])
    assert faces >= 32 and arm == (1 << 24) + 16 and rule.bit_length(arm) == 25
    s = rule.bit_length(faces) + 25 - 30
    assert s >= 1 and rec["exp2_p"] == 127 - 32 + s and rec["exp2_f"] == 127 - 32 + s
    t = ((2 ** 24 - 1) << 9) >> s
    assert load_rule.terms([FLT_MAX], 127 - 32 + s) == [t] and t < 2 ** (33 - s)
    # the friction sum does not cancel: every face adds a product of the same sign per direction pair
    assert abs(int(rec["mf"])) > 2 ** 33 * 2 ** 24 and abs(int(rec["mf"])) < 2 ** 63 and abs(int(rec["mp"])) < 2 ** 63
    without_s = sum(abs(rule.friction_product(d, rx2, ry2, load_rule.terms([vt], 127 - 32)[0])) for d, rx2, ry2, _, vt in rule.face_list(p, v, solid, None, 1, *piv[0]))
    assert without_s >= abs(int(rec["mf"])) << s > 0, "the unshifted products are 2^s times as large"
    # ... and moderate values lose their low s bits only
    rng = np.random.default_rng(13)
    p, v = rng.standard_normal((9, 9)).astype(F), rng.standard_normal((9, 9, 2)).astype(F)
    rec = rule.torque(p, v, solid, None, 1, piv)[0]
    assert rec["exp2_p"] == load_rule.loads(p, solid)[0]["exp2"] + s and rec["exp2_f"] == friction_rule.friction(v, solid)[0]["exp2"] + s


def test_at_the_boundary_L_faces_plus_L_arm_equal_to_30_s_is_still_zero():
    """A single solid cell has 4 faces, L = 3: the arm's bit length may be 27.  2^26 is beyond the pivots' bound, so the boundary
    is reached with more faces: a 2 x 62 block has 128 faces, L = 8, and an arm of 2^21 .. 2^22 - 1 half cells, L = 22."""
    solid = block(70, 8, 3, 2, 62, 2)
    p = np.random.default_rng(14).standard_normal((8, 70)).astype(F)
    v = np.random.default_rng(15).standard_normal((8, 70, 2)).astype(F)
    rec = rule.torque(p, v, solid, None, 1, [[-(1 << 22) + 200, 0]])[0]
    assert rec["faces"] == 128 and rule.bit_length(rec["faces"]) == 8 and rule.bit_length(rec["max_arm2"]) == 22
    assert rule.shift(rec["faces"], rec["max_arm2"]) == 0 and rec["exp2_p"] == load_rule.loads(p, solid)[0]["exp2"]
    over = rule.torque(p, v, solid, None, 1, [[-(1 << 22), 0]])[0]
    assert rule.bit_length(over["max_arm2"]) == 23 and over["exp2_p"] == rec["exp2_p"] + 1 and over["exp2_f"] == rec["exp2_f"] + 1, "one bit more: s = 1"


def test_a_body_without_a_face_and_nonfinite_faces():
    solid = block(7, 5, 3, 2, 1, 1)
    labels = np.zeros((5, 7), np.uint8)
    labels[2, 3] = 2
    p = np.ones((5, 7), F)
    v = np.ones((5, 7, 2), F)
    rec = rule.torque(p, v, solid, labels, 3, [[1, 2], [3, 4], [5, 6]])
    for k in (0, 2):
        want = np.zeros((), rule.DTYPE)
        want["pivot2"] = [[1, 2], [3, 4], [5, 6]][k]
        assert rec[k].tobytes() == want.tobytes(), "no face: all zeros, the pivot filled in"
    assert rec[1]["faces"] == 4
    p[2, 2] = np.nan          # the W face's pressure
    v[1, 3, 0] = np.inf       # the S face's tangential component
    v[2, 4, 0] = np.nan       # the E face's NORMAL component: not looked at
    cut = rule.torque(p, v, solid, labels, 3, [[1, 2], [3, 4], [5, 6]])[1]
    assert cut["nonfinite_p"] == 1 and cut["nonfinite_t"] == 1 and cut["faces"] == 4 and cut["max_arm2"] == rec[1]["max_arm2"]
    rx2, ry2 = 2 * 3 - 3, 2 * 2 - 4
    assert int(rec[1]["mp"]) - int(cut["mp"]) == rule.pressure_product(W, rx2, ry2, 1 << 32), "the face left mp alone ..."
    assert int(rec[1]["mf"]) - int(cut["mf"]) == rule.friction_product(S, rx2, ry2, 1 << 32), "... and the other left mf alone"


# ---- csrc/torque_face.h on the host, face by face ---------------------------------------------------------------------------
def build(target="all"):
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "torque.mk", "-j4", target], check=True, stdout=subprocess.DEVNULL)
    return cpp


def test_torque_face_h_gives_the_rules_arms_and_products_face_by_face(tmp_path):
    rng = np.random.default_rng(16)
    records, want = [], []
    cases = [(checkerboard(), (1 << 24, -(1 << 24))), (checkerboard(), (-(1 << 24), 1 << 24)), (disc(33, 18, 16, 9, 5), (33, 19)), (block(7, 5, 3, 2, 1, 1), (0, 0)),
             (rng.random((23, 31)) < 0.4, (-77, 1001))]
    for solid, (px2, py2) in cases:
        p = np.zeros(solid.shape, F)
        v = np.zeros(solid.shape + (2,), F)
        faces = rule.face_list(p, v, solid, None, 1, px2, py2)
        arm = max(max(abs(rx2), abs(ry2)) for _, rx2, ry2, _, _ in faces)
        s = rule.shift(len(faces), arm)
        for n, (d, rx2, ry2, _, _) in enumerate(faces):
            # the fluid cell back from the arms; terms as large as the rule allows, of either sign, and small ones
            di, dj = rule.SOLID_OF[d]
            i, j = (rx2 + px2) // 2 - di, (ry2 + py2) // 2 - dj
            big = (1 << (33 - s)) - 1
            tp, tf = (big, -big) if n % 3 == 0 else (int(rng.integers(-big, big + 1)), int(rng.integers(-1000, 1000)))
            records.append([i, j, d, px2, py2, tp, tf, len(faces), arm])
            want.append([rx2, ry2, max(abs(rx2), abs(ry2)), rule.pressure_product(d, rx2, ry2, tp), rule.friction_product(d, rx2, ry2, tf),
                         rule.bit_length(len(faces)), rule.bit_length(arm), s])
    for faces, arm in ((0, 0), (1, 1), (2 ** 15 - 1, 2 ** 15 - 1), (2 ** 15, 2 ** 15 - 1), (2 ** 30 - 1, 2 ** 30 - 1), (2 ** 32 - 1, 2 ** 32 - 1), (128, 2 ** 22 - 1), (128, 2 ** 22)):
        records.append([0, 0, 0, 0, 0, 0, 0, faces, arm])
        want.append([2, 0, 2, 0, 0, rule.bit_length(faces), rule.bit_length(arm), rule.shift(faces, arm)])
    assert all(abs(x) < 2 ** 63 for row in want for x in row) and len({r[2] for r in records}) == 4 and any(w[7] > 0 for w in want)
    src, dst = tmp_path / "faces.bin", tmp_path / "products.bin"
    np.array(records, np.int64).tofile(src)
    r = subprocess.run([os.path.join(build(), "torque_driver"), str(src), str(dst)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and f"{len(records)} faces through torque_face.h" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    got = np.fromfile(dst, np.int64).reshape(len(records), 8)
    assert got.tolist() == want


# ---- the host side ---------------------------------------------------------------------------------------------------------
def build_and_run(target, program):
    r = subprocess.run([os.path.join(build(target), program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


def test_the_host_side_of_the_torque():
    """`make -C tests/cpp -f torque.mk`: tests/cpp/torque_driver.cpp, a stand-alone program.  The pivots' calls; admission at all
    five points; a refusal leaves the steps and the recorder untouched; samples of zeros and the pivots inside a one-launch
    replay and across the seams, neither cut; history, loads, friction, torque in the launch log; no torque recorder: the log
    of the null pointer; set_bodies refused while the recorder is on, with its message; destroy leaves no allocation."""
    build_and_run("all", "torque_driver")


def test_the_host_side_of_the_torque_under_asan_and_ubsan():
    """The same stand-alone program, every unit compiled with -fsanitize=address,undefined, run directly."""
    build_and_run("san", "torque_driver_san")
