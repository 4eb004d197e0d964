"""Views, the CPU side: sfl_view_* / sfl_batch_view_* / sfl_batch_record_view (include/sfl.h "VIEWS") as the binding sees them
-- symbols, signatures, constants, the layout of struct sfl_view, the Python methods -- every refusal that needs no device
with its own message, the numpy rule of the GPU tests (tests/view_rule.py) checked against the oracle and against known
values, the header's claim about the palette's range checked on the rule, and the host unit (csrc/views.cpp and its hook in
the recorder) run through by tests/cpp/views_driver.cpp over a runtime that lives on the host.  tests/test_views_gpu.py has
the kernels."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import view_rule as rule
from conftest import ROOT, assert_bit_equal, random_fields

CALLS = ["sfl_view_scalar", "sfl_batch_view_scalar", "sfl_view_texels", "sfl_batch_view_texels", "sfl_view_render",
         "sfl_batch_view_render_members", "sfl_batch_record_view"]
M = rule.MAX_COLOUR


def test_the_symbols_are_exported_and_bound_with_the_headers_types(sfl):
    lib, cap = sfl.capi.lib(), sfl.capi
    vp, i, f, sz = C.c_void_p, C.c_int, C.c_float, C.c_size_t
    pf, pu, ph, pv = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_uint16), C.POINTER(cap.View)
    want = {"sfl_view_scalar": [vp, i, f, pf, sz], "sfl_batch_view_scalar": [vp, i, f, i, i, pf, sz],
            "sfl_view_texels": [vp, pv, pu, sz], "sfl_batch_view_texels": [vp, pv, i, i, pu, sz],
            "sfl_view_render": [vp, pv, i, i, ph, sz], "sfl_batch_view_render_members": [vp, pv, i, i, i, i, ph, sz],
            "sfl_batch_record_view": [vp, pv]}
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    for name in CALLS:
        assert hasattr(lib, name), name
        assert cap.SIGNATURES[name] == (C.c_int, want[name]), name
        assert getattr(lib, name).argtypes == want[name] and getattr(lib, name).restype == C.c_int
        handle = "sfl_batch *b" if "batch" in name else "sfl_context *ctx"
        assert re.search(r"SFL_API int %s\(%s," % (name, re.escape(handle)), header), name
    for name in ("view_scalar", "view_texels", "view_render"):
        assert callable(getattr(sfl.Solver, name, None)), name
    for name in ("view_scalar", "view_texels", "view_render_members", "record_view"):
        assert callable(getattr(sfl.BatchSolver, name, None)), name
    assert lib.sfl_abi_version() == 1


def test_the_constants_and_the_struct_are_the_headers(sfl):
    cap = sfl.capi
    header = open(os.path.join(ROOT, "include", "sfl.h")).read()
    defines = {name: int(value.rstrip("u"), 0) for name, value in re.findall(r"#define SFL_(VIEW_\w+)\s+(\w+)", header)}
    assert defines == {"VIEW_SPEED": 0, "VIEW_VORTICITY": 1, "VIEW_PRESSURE": 2, "VIEW_DIVERGENCE": 3, "VIEW_MAX_STOPS": 256,
                       "VIEW_MAX_COLOUR": 0xFC000000}
    assert defines == {k: v for k, v in vars(cap).items() if k.startswith("VIEW_") and isinstance(v, int)}
    assert (rule.SPEED, rule.VORTICITY, rule.PRESSURE, rule.DIVERGENCE, rule.MAX_COLOUR) == (0, 1, 2, 3, cap.VIEW_MAX_COLOUR)
    kernels = open(os.path.join(ROOT, "esp32-fluid-simulation_amd", "csrc", "view_kernels.h")).read()
    assert int(re.search(r"constexpr int kViewMaxStops = (\d+);", kernels).group(1)) == cap.VIEW_MAX_STOPS
    # struct sfl_view: 40 bytes, the offsets the header states
    offsets = {name: getattr(cap.View, name).offset for name, _ in cap.View._fields_}
    assert C.sizeof(cap.View) == 40
    assert offsets == {"what": 0, "dx": 4, "lo": 8, "hi": 12, "stops": 16, "nan_colour": 20, "colours": 32}
    assert "what 0, dx 4, lo 8, hi 12, stops 16, nan_colour 20, colours 32" in header and "40 bytes" in header
    # the built-in palettes respect the cap, and the blue-white-red one is white in the middle
    for pal in (sfl.PALETTE_GREY, sfl.PALETTE_HEAT, sfl.PALETTE_BLUE_WHITE_RED):
        assert pal.dtype == np.uint32 and pal.ndim == 2 and pal.shape[1] == 3 and 2 <= pal.shape[0] <= 256 and pal.max() <= M
    assert sfl.PALETTE_GREY.shape[0] == 256 and tuple(sfl.PALETTE_GREY[0]) == (0, 0, 0) and tuple(sfl.PALETTE_GREY[-1]) == (M, M, M)
    assert tuple(sfl.PALETTE_BLUE_WHITE_RED[1]) == (M, M, M)
    v = sfl.View(cap.VIEW_VORTICITY, -2.0, 2.0, sfl.PALETTE_BLUE_WHITE_RED, dx=0.5, nan_colour=(1, 2, 3)).struct()
    assert (v.what, v.dx, v.lo, v.hi, v.stops, tuple(v.nan_colour)) == (1, 0.5, -2.0, 2.0, 3, (1, 2, 3))
    with pytest.raises(ValueError):
        sfl.View(0, 0.0, 1.0, np.zeros((4, 2), np.uint32))


def _view(cap, what=1, dx=1.0, lo=-1.0, hi=1.0, stops=3, colours="ok", nan=(0, 0, 0)):
    pal = (C.c_uint32 * 768)(*([M, 0, 7] * 256))
    keep = pal if colours == "ok" else colours
    v = cap.View(what, dx, lo, hi, stops, (C.c_uint32 * 3)(*nan), C.cast(keep, C.POINTER(C.c_uint32)) if keep is not None else None)
    v._keep = pal
    return v


def test_bad_arguments_are_refused_without_a_gpu_each_with_its_own_message(sfl):
    """The checks that need no device: a value that is wrong whatever the object first, then the NULL object."""
    lib, cap = sfl.capi.lib(), sfl.capi
    buf = (C.c_uint32 * 16)()
    fbuf, hbuf = C.cast(buf, C.POINTER(C.c_float)), C.cast(buf, C.POINTER(C.c_uint16))
    over = (C.c_uint32 * 768)(*([0] * 4 + [M + 1] + [0] * 763))
    inf, nan = float("inf"), float("nan")
    bad_views = [   # (view, what its message says)
        (_view(cap, what=4), "unknown view 4"), (_view(cap, what=-1), "unknown view -1"),
        (_view(cap, stops=1), "stops must be 2..256 (got 1)"), (_view(cap, stops=257), "stops must be 2..256 (got 257)"),
        (_view(cap, colours=None), "colours is NULL"),
        (_view(cap, lo=1.0, hi=1.0), "hi - lo must be finite and > 0"), (_view(cap, lo=1.0, hi=0.5), "hi - lo must be finite and > 0"),
        (_view(cap, lo=-3e38, hi=3e38), "hi - lo must be finite and > 0"), (_view(cap, lo=nan), "hi - lo must be finite and > 0"),
        (_view(cap, hi=inf), "hi - lo must be finite and > 0"),
        (_view(cap, dx=0.0), "dx must be finite and > 0"), (_view(cap, dx=-1.0), "dx must be finite and > 0"),
        (_view(cap, dx=inf), "dx must be finite and > 0"), (_view(cap, dx=nan), "dx must be finite and > 0"),
        (_view(cap, nan=(0, M + 1, 0)), "nan_colour channel 1 is 0xFC000001"),
        (_view(cap, colours=over), "stop 1 channel 1 is 0xFC000001"),
        (_view(cap, colours=(C.c_uint32 * 768)(*([0] * 767 + [0xFFFFFFFF])), stops=256), "stop 255 channel 2 is 0xFFFFFFFF"),
    ]
    with_view = {
        "sfl_view_texels": lambda v: lib.sfl_view_texels(None, v, buf, 64),
        "sfl_batch_view_texels": lambda v: lib.sfl_batch_view_texels(None, v, 0, 1, buf, 64),
        "sfl_view_render": lambda v: lib.sfl_view_render(None, v, 4, 1, hbuf, 64),
        "sfl_batch_view_render_members": lambda v: lib.sfl_batch_view_render_members(None, v, 0, 1, 4, 1, hbuf, 64),
        "sfl_batch_record_view": lambda v: lib.sfl_batch_record_view(None, v),
    }
    for name, call in with_view.items():
        for k, (view, message) in enumerate(bad_views):
            assert call(C.byref(view)) == cap.ERR_INVALID, (name, k)
            said = lib.sfl_last_error().decode()
            assert message in said and said.startswith(name + ":"), (name, k, said)
        good = _view(cap)
        assert call(C.byref(good)) == cap.ERR_INVALID   # the NULL object
        assert lib.sfl_last_error().decode() == name + (": batch is NULL" if "batch" in name else ": ctx is NULL")
    for name in ("sfl_view_texels", "sfl_batch_view_texels", "sfl_view_render", "sfl_batch_view_render_members"):
        assert with_view[name](None) == cap.ERR_INVALID and lib.sfl_last_error().decode() == name + ": view is NULL"
    assert lib.sfl_batch_record_view(None, None) == cap.ERR_INVALID   # (a NULL view is the dye: the NULL batch is what is wrong)
    assert lib.sfl_last_error().decode() == "sfl_batch_record_view: batch is NULL"
    good = _view(cap)
    for scaling in (0, 65, -1):
        for name, call in (("sfl_view_render", lambda: lib.sfl_view_render(None, C.byref(good), scaling, 1, hbuf, 64)),
                           ("sfl_batch_view_render_members", lambda: lib.sfl_batch_view_render_members(None, C.byref(good), 0, 1, scaling, 1, hbuf, 64))):
            assert call() == cap.ERR_INVALID
            assert lib.sfl_last_error().decode() == f"{name}: scaling must be 1..64 (got {scaling})"
    scalars = {"sfl_view_scalar": lambda what, dx: lib.sfl_view_scalar(None, what, dx, fbuf, 64),
               "sfl_batch_view_scalar": lambda what, dx: lib.sfl_batch_view_scalar(None, what, dx, 0, 1, fbuf, 64)}
    for name, call in scalars.items():
        for what, dx, message in ((4, 1.0, "unknown view 4"), (-1, 1.0, "unknown view -1"), (0, 0.0, "dx must be finite and > 0"),
                                  (3, nan, "dx must be finite and > 0"), (3, inf, "dx must be finite and > 0"), (1, -2.0, "dx must be finite and > 0"),
                                  (1, 1.0, "batch is NULL" if "batch" in name else "ctx is NULL")):
            assert call(what, dx) == cap.ERR_INVALID, (name, what, dx)
            said = lib.sfl_last_error().decode()
            assert message in said and said.startswith(name + ":"), (name, what, dx, said)
    assert not any(buf), "no refused call wrote anything"


# ---- the rule of the GPU tests, checked ------------------------------------------------------------------------------
@pytest.mark.parametrize("dim_x,dim_y", [(2, 2), (3, 2), (5, 4), (33, 17), (61, 81)])
@pytest.mark.parametrize("dx", [1.0, 0.37])
def test_the_rules_divergence_is_the_oracles_bit_for_bit(oracle, dim_x, dim_y, dx):
    v, _, _ = random_fields(dim_x, dim_y, 5 * dim_x + dim_y)
    assert_bit_equal(rule.divergence(v, dx), oracle.divergence(v, dx), f"{dim_x} x {dim_y}, dx {dx}")
    v[0, 0] = (-0.0, 0.0)   # the signs of zero at a corner, where the sum starts from 0.0f
    v[-1, -1] = (0.0, -0.0)
    assert_bit_equal(rule.divergence(v, dx), oracle.divergence(v, dx), f"{dim_x} x {dim_y}, dx {dx}, signed zeros")


def test_the_rules_vorticity_and_speed_have_their_known_values():
    """A rigid rotation v = omega x r on integer coordinates: every difference is exact, the interior vorticity is 2 omega
    (and 2 omega / dx^... scaled by 1 / (2 dx) for another spacing); on a wall the ghost is minus the node's own component."""
    dim_x, dim_y, omega = 9, 7, 0.5
    j, i = np.mgrid[0:dim_y, 0:dim_x].astype(np.float32)
    v = np.stack([-omega * (j - 3), omega * (i - 4)], -1).astype(np.float32)
    w = rule.vorticity(v, 1.0)
    assert np.all(w[1:-1, 1:-1] == np.float32(1.0))
    assert np.all(rule.vorticity(v, 0.25)[1:-1, 1:-1] == np.float32(4.0))
    # the west wall, away from the corners: E = vy(1, j), W = -vy(0, j); N - S as in the interior
    want = ((v[1:-1, 1, 1] - (-v[1:-1, 0, 1])) - (v[2:, 0, 0] - v[:-2, 0, 0])) * np.float32(0.5)
    assert_bit_equal(w[1:-1, 0], want.astype(np.float32), "the west wall")
    # a corner: both missing neighbours are ghosts
    want = ((v[0, 1, 1] - (-v[0, 0, 1])) - (v[1, 0, 0] - (-v[0, 0, 0]))) * np.float32(0.5)
    assert w[0, 0] == np.float32(want)
    assert rule.speed(np.array([[[3.0, 4.0], [0.0, -0.0]]], np.float32)).tolist() == [[5.0, 0.0]]
    tiny = np.array([[[1e-42, 1e-42]]], np.float32)   # denormal inputs: the squares vanish, not the rule
    assert rule.speed(tiny)[0, 0] == 0.0 and rule.speed(np.array([[[2.0 ** -70, 0.0]]], np.float32))[0, 0] == np.float32(2.0 ** -70)
    assert rule.scalar(rule.PRESSURE, v, w, 1.0) is not w and np.array_equal(rule.scalar(rule.PRESSURE, v, w), w)


@pytest.mark.parametrize("scaling", [1, 3, 4, 64])
def test_the_rules_draw_chain_is_the_oracles(oracle, scaling):
    _, c, _ = random_fields(5, 4, 77, cmax=0xFF000000)
    for byteswap in (True, False):
        assert_bit_equal(rule.render(c, scaling, byteswap), oracle.render_rgb565(c, scaling, byteswap), f"scaling {scaling}, swap {byteswap}")


def test_the_rules_texels_clamp_and_mark_nans():
    pal = np.array([[0, 0, M], [M, M, M], [M, 0, 0]], np.uint32)
    s = np.array([-np.inf, -1.5, -1.0, -0.5, 0.0, 0.5, 1.0, 7.0, np.inf, np.nan], np.float32)
    t = rule.texels(s, -1.0, 1.0, pal, (5, 6, 7))
    assert t[:3].tolist() == [[0, 0, M]] * 3 and t[6:9].tolist() == [[M, 0, 0]] * 3 and t[4].tolist() == [M, M, M]
    assert t[3].tolist() == [M // 2, M // 2, M] and t[5].tolist() == [M, M // 2, M // 2] and t[9].tolist() == [5, 6, 7]
    # a range so small that r is inf: at s == lo, t = 0 * inf is a NaN although s is none
    assert rule.texels(np.float32([0.0, 1.0]), 0.0, 1e-45, pal, (5, 6, 7)).tolist() == [[5, 6, 7], [M, 0, 0]]


# ---- the header's claim about the palette's range ----------------------------------------------------------------------
def _adversarial_palettes():
    rng = np.random.default_rng(2024)
    pals = [np.array([[0, M, 0], [M, 0, M]], np.uint32),                       # a 2-stop table, 0 <-> M neighbours both ways
            np.array([[M, M, M], [M, M, M], [0, 0, 0], [0, 0, 0]], np.uint32),    # equal stops
            np.array([[0, M, 1], [M, 0, M - 1], [0, M, 127], [M, 1, M - 129], [1, M, 255]], np.uint32),   # small values next to M
            rng.integers(0, M + 1, (256, 3), dtype=np.uint32), rng.integers(0, M + 1, (7, 3), dtype=np.uint32),
            rng.choice(np.array([0, 1, 127, 128, 129, 255, 256, M - 256, M - 255, M - 129, M - 128, M - 1, M], np.uint32), (64, 3))]
    alternating = np.zeros((256, 3), np.uint32)
    alternating[::2, 0] = alternating[1::2, 1] = M
    alternating[:, 2] = rng.integers(0, 300, 256)
    return pals + [alternating]


def _sweep(stops):
    """t in [0, 1]: a grid, and the floats next to every n / (stops - 1) as x = t * (stops - 1) sees them."""
    knots = (np.arange(stops, dtype=np.float64) / (stops - 1)).astype(np.float32)
    near = np.concatenate([np.nextafter(knots, np.float32(-1)), knots, np.nextafter(knots, np.float32(2))])
    return np.clip(np.concatenate([np.linspace(0, 1, 997, dtype=np.float32), near]), 0, 1).astype(np.float32)


@pytest.mark.parametrize("k", range(7))
def test_every_float_handed_to_a_narrowing_stays_where_narrowing_is_defined(k):
    """include/sfl.h: with every stop <= 0xFC000000, every intermediate of the palette's lerp and of the draw's walks stays
    inside (-0.5, 2^32).  Checked on the rule: the lerp over a sweep of t, then the draw chains at scaling 1, 3 and 64 over
    the texels it gives, laid out so that the sweep's neighbours and the palette's extremes are neighbours in both axes."""
    pal = _adversarial_palettes()[k]
    t = _sweep(pal.shape[0])
    val, nan = rule.lerp_floats(t, 0.0, 1.0, pal)
    assert not nan.any()
    assert val.min() > -0.5 and val.max() < 2.0 ** 32, (val.min(), val.max())
    tex = rule.narrow(val)
    rng = np.random.default_rng(k)
    extremes = np.array([[0, 0, 0], [M, M, M], [0, M, 0], [M, 0, M]], np.uint32)
    pool = np.concatenate([tex, extremes[rng.integers(0, 4, len(tex) // 4)]])
    for scaling, side in ((1, 30), (3, 30), (64, 12)):   # (the shortest sweep has 1003 texels)
        grid = pool[rng.permutation(len(pool))[:side * side]].reshape(side, side, 3)
        grid[::3, ::2] = extremes[rng.integers(0, 4, grid[::3, ::2].shape[:2])]   # extremes beside anything
        x = rule.draw_floats(grid, scaling)
        assert x.min() > -0.5 and x.max() < 2.0 ** 32, (scaling, x.min(), x.max())
        ordered = tex[:side * side].reshape(side, side, 3)   # ... and the sweep's own order: neighbours in t are neighbours
        x = rule.draw_floats(ordered, scaling)
        assert x.min() > -0.5 and x.max() < 2.0 ** 32, (scaling, x.min(), x.max())


# ---- the host unit -------------------------------------------------------------------------------------------------------
def test_the_host_side_of_the_views():
    """`make -C tests/cpp -f views.mk`: tests/cpp/views_driver.cpp, a stand-alone program under AddressSanitizer + UBSan:
    the pointers and strides the launchers are handed for first > 0, the staged palette's bytes, record_view before
    record_start, its reset by record_start and record_stop, frames by the dye unless a view is set, every refusal with its
    message, and destroy with a staged view leaves no allocation."""
    if not (shutil.which(os.environ.get("CXX", "g++")) and shutil.which("make")):
        pytest.skip("no C++ compiler or make on this box")
    cpp = os.path.join(ROOT, "tests", "cpp")
    subprocess.run(["make", "-C", cpp, "-f", "views.mk", "-j4"], check=True, stdout=subprocess.DEVNULL)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([os.path.join(cpp, "views_driver")], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    assert "0 failed checks, 0 allocations left" in r.stdout
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr and "LeakSanitizer" not in r.stderr, r.stderr[-4000:]
