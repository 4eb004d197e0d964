"""CPU suite: the averages (include/sfl.h "AVERAGES") without a GPU.  The header states the rule, the binding mirrors it; the
argument refusals that need no device, each with its own message; the rule's numpy restatement (tests/mean_rule.py), which
tests/test_means_gpu.py holds the kernel to, against exact arithmetic; the host side (csrc/means.cpp and the hooks in the step
calls) run through by tests/cpp/means_driver.cpp, plain and under ASan + UBSan."""
import ctypes as C
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mean_rule as rule
from conftest import ROOT

F = np.float32


def header():
    return open(os.path.join(ROOT, "include", "sfl.h")).read()


def section():
    text = header()
    return text[text.index("--- AVERAGES:"):text.index("SFL_API int sfl_batch_mean_download(")]


# ---- the header and the binding -------------------------------------------------------------------------------------------
def test_the_header_states_the_rule():
    text = section()
    for words in ("one PLANE per quantity, one value per cell", "ONE launch on the stream", "the host never waits", "only the planes of the chosen groups exist",
                  "SFL_MEAN_VELOCITY (1)   planes U (0), V (1)", "SFL_MEAN_STRESS   (2)   planes UU (2), VV (3), UV (4)", "SFL_MEAN_PRESSURE (4)   planes P (5), PP (6)",
                  "SFL_MEAN_DYE      (8)   planes R (7), G (8), B (9)", "uint64", "the raw UQ32 value of each channel", "(double)v.x * (double)v.y", "(double)p * (double)p",
                  "STARTS AT +0.0 (0 for the dye planes)", "THE FIELDS HELD", "the projected\n * velocity of the step it follows", "SFL_FIELD_PRESSURE as held",
                  "SOLID CELLS INCLUDED", "ONE IEEE-754 DOUBLE ADDITION PER PLANE AND CELL, in sample order", "exact\n * in a double (48 <= 53 bits)",
                  "needs no word\n * about contraction", "PLAIN IEEE", "NO OTHER CELL'S", "NEVER FLUSHED", "+0.0 + (-0.0) is +0.0", "BIT FOR BIT", "NO TOLERANCE",
                  "cannot\n * wrap below 2^32 samples", "THE MEANS ARE NOT THE LIBRARY'S", "sum / samples", "UU / n - (U / n)^2", "no division on\n * the device",
                  "(s + 1) * every", "IS CUT at the steps whose sample is due", "WITHOUT ITS FUSED STEP BOUNDARIES", "exactly as with a history on",
                  "`every` == 0: nothing is added behind the steps and no\n * hook is set", "tracers, history, loads, friction, averages", "NO CAPACITY",
                  "never refused for the averages", "launches exactly what it launched before", "5.4 GB", "SFL_ERR_NOMEM with nothing set",
                  "a slab and a context with a transport attached get SFL_ERR_STATE", "argument checks come first", "A start while on begins anew from zero",
                  "Drains the stream, frees the planes", "whatever `every` is", "densely packed, whatever the\n * padding on the device",
                  "must lie inside the recorded range"):
        assert words in text, words


def test_the_section_stands_behind_the_friction_and_leaves_the_others_alone():
    text = header()
    order = [text.index(w) for w in ("--- LOADS:", "--- VISCOSITY:", "--- OPENINGS:", "--- INFLOW PROFILES AND FLUX", "--- FRICTION:", "SFL_API int sfl_friction_read(",
                                     "--- AVERAGES:", "SFL_API int sfl_batch_mean_download(", "SFL_API int sfl_batch_synchronize(")]
    assert order == sorted(order)
    assert text.count("--- AVERAGES:") == 1


def test_the_constants_of_the_header_the_binding_and_the_rule_agree(sfl):
    text = header()
    defined = {name: int(num) for name, num in re.findall(r"#define SFL_(MEAN_\w+)\s+(\d+)", text)}
    assert defined == {"MEAN_VELOCITY": 1, "MEAN_STRESS": 2, "MEAN_PRESSURE": 4, "MEAN_DYE": 8, "MEAN_ALL": 15, "MEAN_PLANE_U": 0, "MEAN_PLANE_V": 1,
                       "MEAN_PLANE_UU": 2, "MEAN_PLANE_VV": 3, "MEAN_PLANE_UV": 4, "MEAN_PLANE_P": 5, "MEAN_PLANE_PP": 6, "MEAN_PLANE_R": 7, "MEAN_PLANE_G": 8,
                       "MEAN_PLANE_B": 9, "MEAN_PLANES": 10}
    assert {k: v for k, v in vars(sfl.capi).items() if k.startswith("MEAN_")} == defined
    assert (sfl.MEAN_VELOCITY, sfl.MEAN_STRESS, sfl.MEAN_PRESSURE, sfl.MEAN_DYE, sfl.MEAN_ALL) == (rule.VELOCITY, rule.STRESS, rule.PRESSURE, rule.DYE, rule.ALL)
    assert sfl.MEAN_PLANE_NAMES == rule.NAMES and [defined["MEAN_PLANE_" + n] for n in rule.NAMES] == list(range(10))
    assert [len(rule.planes_of(w)) for w in range(16)] == [0, 2, 3, 5, 2, 4, 5, 7, 3, 5, 6, 8, 5, 7, 8, 10]
    assert [rule.dtype_of(k) for k in range(10)] == [np.float64] * 7 + [np.uint64] * 3


def test_the_ten_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, sz, pi, p64 = C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int64)
    want = {"sfl_mean_start": ([vp, i, i], "sfl_context *ctx, int what, int every"), "sfl_mean_stop": ([vp], "sfl_context *ctx"),
            "sfl_mean_sample": ([vp], "sfl_context *ctx"),
            "sfl_mean_info": ([vp, pi, pi, p64, p64], "sfl_context *ctx, int *what, int *every, int64_t *samples, int64_t *steps"),
            "sfl_mean_download": ([vp, i, vp, sz], "sfl_context *ctx, int plane, void *host, size_t bytes"),
            "sfl_batch_mean_start": ([vp, i, i, i, i], "sfl_batch *b, int what, int every, int first, int count"), "sfl_batch_mean_stop": ([vp], "sfl_batch *b"),
            "sfl_batch_mean_sample": ([vp], "sfl_batch *b"),
            "sfl_batch_mean_info": ([vp, pi, pi, p64, p64], "sfl_batch *b, int *what, int *every, int64_t *samples, int64_t *steps"),
            "sfl_batch_mean_download": ([vp, i, i, i, vp, sz], "sfl_batch *b, int plane, int first_member, int members, void *host, size_t bytes")}
    text = header()
    assert len(want) == 10
    for name, (args, declared) in want.items():
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (i, args), name
        assert f"SFL_API int {name}({declared});" in text, name
    for cls in (sfl.Solver, sfl.BatchSolver):
        for method in ("mean_start", "mean_stop", "mean_sample", "mean_info", "mean_sums", "means", "reynolds_stress"):
            assert callable(getattr(cls, method)), (cls, method)


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message_argument_checks_first(sfl):
    lib = sfl.capi.lib()
    host, w, n = (C.c_double * 4)(), C.c_int(5), C.c_int64(7)
    refusals = [
        (lambda: lib.sfl_batch_mean_start(None, 0, 1, 0, 1), "sfl_batch_mean_start: what must be a mask of SFL_MEAN_* groups, 1..15 (got 0)"),
        (lambda: lib.sfl_batch_mean_start(None, 16, 1, 0, 1), "sfl_batch_mean_start: what must be a mask of SFL_MEAN_* groups, 1..15 (got 16)"),
        (lambda: lib.sfl_batch_mean_start(None, 3, -1, 0, 1), "sfl_batch_mean_start: every must be >= 0 (got -1)"),
        (lambda: lib.sfl_batch_mean_start(None, 3, 0, 0, 0), "sfl_batch_mean_start: count must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_mean_start(None, 3, 0, 0, 1), "sfl_batch_mean_start: batch is NULL"),
        (lambda: lib.sfl_batch_mean_stop(None), "sfl_batch_mean_stop: batch is NULL"),
        (lambda: lib.sfl_batch_mean_sample(None), "sfl_batch_mean_sample: batch is NULL"),
        (lambda: lib.sfl_batch_mean_info(None, C.byref(w), C.byref(w), C.byref(n), C.byref(n)), "sfl_batch_mean_info: batch is NULL"),
        (lambda: lib.sfl_batch_mean_download(None, 10, 0, 1, host, 32), "sfl_batch_mean_download: plane must be one of SFL_MEAN_PLANE_*, 0..9 (got 10)"),
        (lambda: lib.sfl_batch_mean_download(None, -1, 0, 1, host, 32), "sfl_batch_mean_download: plane must be one of SFL_MEAN_PLANE_*, 0..9 (got -1)"),
        (lambda: lib.sfl_batch_mean_download(None, 0, 0, 0, host, 32), "sfl_batch_mean_download: members must be >= 1 (got 0)"),
        (lambda: lib.sfl_batch_mean_download(None, 0, 0, 1, host, 32), "sfl_batch_mean_download: batch is NULL"),
        (lambda: lib.sfl_mean_start(None, 0, 1), "sfl_mean_start: what must be a mask of SFL_MEAN_* groups, 1..15 (got 0)"),
        (lambda: lib.sfl_mean_start(None, 15, -2), "sfl_mean_start: every must be >= 0 (got -2)"),
        (lambda: lib.sfl_mean_start(None, 15, 0), "sfl_mean_start: ctx is NULL"),
        (lambda: lib.sfl_mean_stop(None), "sfl_mean_stop: ctx is NULL"),
        (lambda: lib.sfl_mean_sample(None), "sfl_mean_sample: ctx is NULL"),
        (lambda: lib.sfl_mean_info(None, None, None, None, None), "sfl_mean_info: ctx is NULL"),
        (lambda: lib.sfl_mean_download(None, 10, host, 32), "sfl_mean_download: plane must be one of SFL_MEAN_PLANE_*, 0..9 (got 10)"),
        (lambda: lib.sfl_mean_download(None, 9, host, 32), "sfl_mean_download: ctx is NULL"),
    ]
    for call, message in refusals:
        assert call() == sfl.capi.ERR_INVALID, message
        assert message in lib.sfl_last_error().decode(), (message, lib.sfl_last_error().decode())
    assert w.value == 5 and n.value == 7


def test_the_python_front_end_forms_means_and_central_moments_in_float64(sfl):
    class Fake(sfl.BatchSolver):
        def __init__(self, sums, samples):   # (no library, no device: the arithmetic needs neither)
            self._h, self._lib = None, None
            self.dim_x, self.dim_y, self.batch = 4, 3, 2
            self.sums, self.samples = sums, samples

        def __del__(self):
            pass

        def mean_info(self):
            return 3, 1, self.samples, self.samples

        def mean_sums(self, plane, first=None, count=None):
            return self.sums[plane]

    rng = np.random.default_rng(1)
    fields = [(rng.standard_normal((2, 3, 4, 2)).astype(F), None, None) for _ in range(5)]
    s = rule.sums(3, fields)
    fake = Fake(s, 5)
    m, rs, want = fake.means(), fake.reynolds_stress(), rule.reynolds_stress(s, 5)
    assert sorted(m) == ["U", "UU", "UV", "V", "VV"] and all(a.dtype == np.float64 for a in m.values())
    assert m["UV"].tobytes() == (s[rule.UV] / np.float64(5)).tobytes()
    assert all(rs[k].dtype == np.float64 and rs[k].tobytes() == want[k].tobytes() for k in ("uu", "vv", "uv", "tke"))
    u = np.stack([f[0][..., 0] for f in fields]).astype(np.float64)
    assert np.allclose(rs["uu"], u.var(axis=0), rtol=1e-12, atol=1e-15), "the central moment is the variance over the samples"
    assert all(np.isnan(a).all() for a in Fake(s, 0).means().values()), "no sample yet: NaN, not a division by zero that raises"
    with pytest.raises(ValueError, match="MEAN_VELOCITY . MEAN_STRESS are needed"):
        type("OnlyStress", (Fake,), {"mean_info": lambda self: (2, 1, 5, 5)})(s, 5).reynolds_stress()


# ---- the rule against exact arithmetic --------------------------------------------------------------------------------------
def seeded_floats(n, seed):
    """float32 over the whole finite range: seeded bit patterns (denormals, both zeros and the extremes put in)."""
    rng = np.random.default_rng(seed)
    bits = rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)
    a = bits.view(F)
    a = a[np.isfinite(a)]
    extra = np.array([0.0, -0.0, np.finfo(F).max, -np.finfo(F).max, np.finfo(F).tiny, 1e-45, -1e-45, 1.0, 3.0], F)
    return np.concatenate([extra, a])


def test_the_product_of_two_float32_values_is_exact_in_a_double():
    a, b = seeded_floats(600, 21), seeded_floats(600, 22)
    n = min(len(a), len(b))
    a, b = a[:n], b[:n]
    prod = a.astype(np.float64) * b.astype(np.float64)
    assert np.isfinite(prod).all()
    for x, y, p in zip(a, b, prod):
        assert Fraction(float(x)) * Fraction(float(y)) == Fraction(float(p)), (x, y, p)
    # ... and so a fused multiply-add rounds what multiply-then-add rounds: the exact sum, once
    acc = seeded_floats(600, 23)[:n].astype(np.float64) * 1e10
    for x, y, s, got in list(zip(a, b, acc, acc + prod))[:300]:
        exact = Fraction(float(s)) + Fraction(float(x)) * Fraction(float(y))
        if exact != 0 and abs(exact) < Fraction(np.finfo(np.float64).max):
            lo, hi = np.nextafter(got, -np.inf), np.nextafter(got, np.inf)
            assert abs(Fraction(float(got)) - exact) <= min(abs(Fraction(float(lo)) - exact), abs(Fraction(float(hi)) - exact))
    tiny = np.array([1e-45], F)
    assert float(tiny[0].astype(np.float64)) == 2.0 ** -149 and float(tiny.astype(np.float64)[0] ** 2) == 2.0 ** -298, "a denormal converts exactly"


def test_a_sequence_of_samples_equals_a_per_cell_python_loop():
    rng = np.random.default_rng(31)
    shape, n = (2, 3, 5), 6
    samples = []
    for _ in range(n):
        with np.errstate(all="ignore"):
            v = (rng.standard_normal(shape + (2,)) * 10.0 ** rng.uniform(-44, 18, shape + (2,))).astype(F)
            p = (rng.standard_normal(shape) * 10.0 ** rng.uniform(-44, 18, shape)).astype(F)
        v[0, 0, 0], v[0, 0, 1], p[1, 2, 4] = (-0.0, 0.0), (1e-45, -1e-45), -0.0
        samples.append((v, p, rng.integers(0, 2 ** 32, shape + (3,), dtype=np.uint64).astype(np.uint32)))
    got = rule.sums(rule.ALL, samples)
    assert sorted(got) == list(range(10))
    for cell in np.ndindex(*shape):
        acc = [0.0] * 7 + [0] * 3
        for v, p, dye in samples:
            x, y, q = float(v[cell][0]), float(v[cell][1]), float(p[cell])   # (a Python float is a double)
            for k, t in enumerate((x, y, x * x, y * y, x * y, q, q * q)):
                acc[k] = acc[k] + t
            for ch in range(3):
                acc[7 + ch] += int(dye[cell][ch])
        for k in range(10):
            want = np.array(acc[k], rule.dtype_of(k))
            assert got[k][cell].tobytes() == want.tobytes(), (cell, rule.NAMES[k], got[k][cell], acc[k])
    for what in (1, 2, 4, 8, 6):
        part = rule.sums(what, samples)
        assert sorted(part) == rule.planes_of(what) and all(part[k].tobytes() == got[k].tobytes() for k in part)


def test_special_values_go_the_way_ieee_sends_them_and_stay_in_their_cell():
    v = np.zeros((3, 4, 2), F)
    p = np.zeros((3, 4), F)
    dye = np.full((3, 4, 3), 0xFFFFFFFF, np.uint32)
    v[1, 2], v[0, 0], v[2, 3] = (np.nan, 2.0), (np.inf, -1.0), (-0.0, -0.0)
    p[2, 1] = -np.inf
    s = rule.sums(rule.ALL, [(v, p, dye)] * 3)
    assert np.argwhere(np.isnan(s[rule.U])).tolist() == [[1, 2]] and np.argwhere(np.isnan(s[rule.UV])).tolist() == [[1, 2]]
    assert np.argwhere(~np.isfinite(s[rule.V])).tolist() == [] and s[rule.V][1, 2] == 6.0 and s[rule.VV][1, 2] == 12.0
    assert s[rule.U][0, 0] == np.inf and s[rule.UU][0, 0] == np.inf and s[rule.UV][0, 0] == -np.inf and s[rule.P][2, 1] == -np.inf and s[rule.PP][2, 1] == np.inf
    assert not np.signbit(s[rule.U][2, 3]) and not np.signbit(s[rule.UV][2, 3]), "+0.0 + (-0.0) is +0.0"
    assert (s[rule.R] == 3 * 0xFFFFFFFF).all() and 2 ** 32 * 0xFFFFFFFF < 2 ** 64, "the dye sums cannot wrap below 2^32 samples"
    quiet = rule.sums(rule.ALL, [(np.zeros((3, 4, 2), F), np.zeros((3, 4), F), np.zeros((3, 4, 3), np.uint32))] * 2)
    assert all(a.tobytes() == bytes(a.nbytes) for a in quiet.values()), "a quiescent field gives +0.0 everywhere"


# ---- the sources ------------------------------------------------------------------------------------------------------------
def test_the_new_host_code_is_a_unit_of_its_own_and_the_step_calls_only_hold_pointers():
    csrc = os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc")
    read = lambda name: open(os.path.join(csrc, name)).read()
    assert len(read("batch.cpp").splitlines()) <= 900
    for unit in ("batch.cpp", "slab_step.cpp", "context.cpp"):
        text = read(unit)
        assert "mean_kernels.h" not in text and "launch_mean_sample" not in text and "sfl_mean_" not in text and "sfl_batch_mean_" not in text, unit
    batch, slab = read("batch.cpp"), read("slab_step.cpp")
    assert batch.count("if (b->mean_step) SFL_TRY(b->mean_step(b,") == 2 and "mean_run(b->means," in batch and "b->means.d_planes" in batch
    for text, hooks in ((batch, ("b->history_step(", "b->loads_step(", "b->friction_step(", "b->mean_step(")),
                        (slab, ("ctx->tracers_follow(", "ctx->history_step(", "ctx->loads_step(", "ctx->friction_step(", "ctx->mean_step("))):
        end = text.rindex(hooks[-1])
        at = [text.rindex(h, 0, end) for h in hooks[:-1]] + [end]   # (the last call of each hook in front of the averages')
        assert at == sorted(at) and end - at[0] < 1200, "behind a step: tracers, history, loads, friction, averages"
    assert "!ctx->history_step && !ctx->mean_step" in slab and "c->means.d_planes" in read("context.cpp")
    kernel = read("means.hip")
    code = kernel[kernel.index("#include"):]   # (behind the opening comment, which says so in words)
    assert "atomic" not in code and "__shared__" not in code and "__syncthreads" not in code, "no atomics, no LDS"


# ---- the host side ---------------------------------------------------------------------------------------------------------
def build_and_run(target, program):
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "means.mk", "-j4", target], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(cpp, program)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout


def test_the_host_side_of_the_averages():
    """`make -C tests/cpp -f means.mk`: tests/cpp/means_driver.cpp, a stand-alone program.  The order history, loads, friction,
    averages behind a step; the replay cut at the due steps and not cut with every == 0; sfl_step_n unfused only while the hook
    is set; planes and bytes per mask; a restart zeroing the planes; steps counted across calls; the downloads; stop and
    destroy freeing the planes."""
    build_and_run("all", "means_driver")


def test_the_host_side_of_the_averages_under_asan_and_ubsan():
    """The same stand-alone program, every unit compiled with -fsanitize=address,undefined, run directly."""
    build_and_run("san", "means_driver_san")
