"""Fields at the bottom of the float range, for every kernel: three seeded textures, the yardstick's answers on them and the
guards that keep a test on them from going vacuous.  tests/test_values.py asserts the guards and pins the yardsticks on these
inputs; tests/test_values_gpu.py holds the kernels to them, bit for bit.

The textures (each a seeded function of the shape; velocity float32[dim_y, dim_x, 2], node (i, j) at [j, i]):

  quiescent  the sketch's own start (ino:199, 264-269) scaled down: a zero velocity, two force records in step 0 -- one at
             the centre, one at cell (1, 1) -- of O(10) times an amplitude A, and touch_dipoles times A as a right-hand
             side.  Six iterations on a small grid put the pressure front into the denormals.  A is 1e-30 or 1e-36 where a
             diffusion spreads the records first, lower in plain and in masked steps (`amplitudes`).  From 61 x 81 up
             only: a smaller grid holds no denormals.
  tiny       dense noise: 40 * 2^-130 times uniform(-1, 1) for the velocity, 2^-130 times a standard normal for the
             right-hand side.  The one texture that has denormals on 2 x 2 and 7 x 9.
  zeros      every velocity component +0.0f or -0.0f with probability 1/2, one force record of normal size; the right-hand
             side is +-0 with one unit spike.
  dense      uniform * 40 and a standard normal: the healthy neighbour of the others in a batch, nothing more.

A flush of denormal inputs or outputs, a multiplication by a 0 / 1 weight where the rule says "absent" (which loses the sign
of a zero), a comparison u <= tol made on a flushed norm and a dropped 0 + x all leave the yardstick's bits on these inputs
and on no dense one.  Not part of the product."""
import functools
from collections import namedtuple

import numpy as np

import solid_rule
import viscosity_rule
from test_batch_params import update_norm
from test_batch_until import sor_iteration, zero_mean
from test_gpu_parity import touch_dipoles
from test_solids_gpu import mask_of

F = np.float32
TINY = np.finfo(np.float32).tiny
# the parameters of the guards: a step of 1 / 30 on a spacing at which no product with dx is exact (tests/dx_cases.py DX_A)
DT, DX, ITERS, OMEGA, NU, SWEEPS, STEPS = 1 / 30.0, 0.37, 6, 1.9, 0.05, 3, 3
AMPLITUDES = (1e-30, 1e-36)


def amplitudes(viscous=False, masked=False):
    """The two amplitudes of the quiescent members.  The sketch's pair puts 100 denormal cells into each of v, d and p only
    where a diffusion spreads the two records first; a plain step needs a start six decades lower for that, and a mask --
    the disc swallows the record at the centre -- two more (measured on the rules: tests/test_values.py prints the counts)."""
    return AMPLITUDES if viscous else (1e-38, 3e-39) if masked else (1e-36, 1e-37)


SCALE = F(2.0 ** -130)
SEED = 7002          # (chosen among 40: the 7 x 9 tiny members keep 12 denormal cells in v, d and p after three steps)
SKETCH = 61 * 81          # cells: the quiescent texture is used from here up, and the guards ask for 100 cells from here up

Texture = namedtuple("Texture", "v forces rhs dye")      # forces: ((i, j, fx, fy), ...), the records of step 0


# ---- the helpers ---------------------------------------------------------------------------------------------------------
def denormals(a):
    """The cells that are nonzero and below finfo.tiny."""
    a = np.abs(np.asarray(a, F))
    return int(np.count_nonzero((a != 0) & (a < TINY)))


def flushed(a):
    """Denormals replaced by zeros of their sign."""
    a = np.asarray(a, F)
    mag = np.abs(a)
    return np.where((mag != 0) & (mag < TINY), np.copysign(F(0), a), a).astype(F)


def negative_zeros(a):
    """The cells that hold -0.0f."""
    return int(np.count_nonzero(np.ascontiguousarray(a, F).view(np.uint32) == np.uint32(0x80000000)))


def positive_zeros(a):
    return int(np.count_nonzero(np.ascontiguousarray(a, F).view(np.uint32) == np.uint32(0)))


def numpy_keeps_denormals():
    """numpy itself must not be flushing: a denormal product, sum and comparison as the yardsticks form them."""
    h = np.array([2.0 ** -130, -2.0 ** -140], F)
    return bool((h * F(0.5) != 0).all() and (h + h != 0).all() and denormals(h * F(0.25)) == 2 and not (np.abs(h) <= F(0)).any())


# ---- the textures --------------------------------------------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def _scale_of(name, amplitude):
    """The size of a force component of the texture, over O(10): the tiny texture's record is of the size of its noise."""
    return F(amplitude) if name == "quiescent" else F(0.4) * SCALE if name == "tiny" else F(1)


@functools.lru_cache(maxsize=None)
def texture(name, dim_x, dim_y, amplitude=None):
    """-> Texture(v, forces, rhs, dye); shared, never written.  The dye lies over [0, 0xFF000000)."""
    assert (name == "quiescent") == (amplitude is not None), (name, amplitude)
    rng = np.random.default_rng(SEED + 131 * dim_x + dim_y + {"quiescent": 0, "tiny": 1, "zeros": 2, "dense": 3}[name])
    dye = rng.integers(0, 0xFF000000, (dim_y, dim_x, 3), dtype=np.uint32)
    cx, cy, s = dim_x // 2, dim_y // 2, _scale_of(name, amplitude)
    centre = (cx, cy, float(F(35.0) * s), float(F(-20.0) * s))
    if name == "quiescent":
        v = np.zeros((dim_y, dim_x, 2), F)
        forces = (centre, (1, 1, float(F(-12.0) * s), float(F(9.0) * s)))
        if dim_x >= 5 and dim_y >= 5:
            rhs = (touch_dipoles(dim_x, dim_y, 20.0, [(0.5, 0.5), (1.5 / dim_x, 1.5 / dim_y)]) * s).astype(F)
        else:   # no room for a dipole: one source and one sink (only the pin of the oracle goes this far down)
            rhs = np.zeros((dim_y, dim_x), F)
            rhs[0, 0], rhs[-1, -1] = F(10) * s, F(-10) * s
    elif name == "tiny":
        v = (rng.uniform(-1, 1, (dim_y, dim_x, 2)).astype(F) * (F(40) * SCALE)).astype(F)
        rhs = (rng.standard_normal((dim_y, dim_x)).astype(F) * SCALE).astype(F)
        forces = (centre,)
    elif name == "zeros":
        v = np.where(rng.random((dim_y, dim_x, 2)) < 0.5, F(0.0), F(-0.0)).astype(F)
        rhs = np.where(rng.random((dim_y, dim_x)) < 0.5, F(0.0), F(-0.0)).astype(F)
        rhs[cy, cx] = 1.0
        forces = (centre,)
    else:
        assert name == "dense", name
        v = (rng.uniform(-1, 1, (dim_y, dim_x, 2)) * 40).astype(F)
        rhs = rng.standard_normal((dim_y, dim_x)).astype(F)
        forces = (centre,)
    return Texture(*_frozen(v), forces, *_frozen(rhs, dye))


def later_record(name, dim_x, dim_y, amplitude=None):
    """One more record, for step 1: with it a batch's step_n(3) replays its timeline in one launch."""
    s = _scale_of(name, amplitude)
    return (dim_x // 3, (2 * dim_y) // 3, float(F(-18.0) * s), float(F(27.0) * s))


# ---- a case: one texture stepped three times by the rules -------------------------------------------------------------------
_Case = namedtuple("Case", "name amplitude dim_x dim_y dt dx iters omega nu sweeps mask later")


def Case(name, amplitude, dim_x, dim_y, dt=DT, dx=DX, iters=ITERS, omega=OMEGA, nu=0.0, sweeps=0, mask=None, later=False):
    """mask: a kind of tests/test_solids_gpu.py mask_of, or None for a plain grid.  nu == 0: no viscosity."""
    return _Case(name, amplitude, dim_x, dim_y, float(dt), float(dx), int(iters), float(omega), float(nu), int(sweeps), mask, bool(later))


def solid_of(case):
    return None if case.mask is None else mask_of(case.mask, case.dim_x, case.dim_y)


def forces_of(case, step):
    """The (i, j, fx, fy) records of one step."""
    if step == 0:
        return texture(case.name, case.dim_x, case.dim_y, case.amplitude).forces
    return (later_record(case.name, case.dim_x, case.dim_y, case.amplitude),) if (step == 1 and case.later) else ()


@functools.lru_cache(maxsize=None)
def rule_steps(case, flush=False):
    """The (v, div, p, colour) every one of the three steps leaves, by tests/viscosity_rule.py (with nu == 0 and no mask the
    oracle's own step; with a mask tests/solid_rule.py).  flush: the velocity a step starts from is passed through `flushed`
    -- what a kernel that flushes its inputs computes.  Shared, never written."""
    from oracle import loader
    cpu = loader.port()
    t = texture(case.name, case.dim_x, case.dim_y, case.amplitude)
    state, out = (t.v, None, None, t.dye), []
    for k in range(STEPS):
        v = flushed(state[0]) if flush else state[0]
        state = viscosity_rule.step(cpu, v, state[3], F(case.dt), F(case.dx), case.iters, F(case.omega), case.nu, case.sweeps,
                                    solid_of(case), forces_of(case, k))
        out.append(_frozen(*(np.ascontiguousarray(a) for a in state)))
    return tuple(out)


def guard(case):
    """What the case must hold to be a test of its value class; raises AssertionError otherwise.  Evaluated on the yardstick
    alone, so it holds wherever the case is used.  Returns the figures."""
    steps = rule_steps(case)
    cells, big = case.dim_x * case.dim_y, case.dim_x * case.dim_y >= SKETCH
    if case.name in ("quiescent", "tiny"):
        assert case.name == "tiny" or big, f"{case}: the quiescent texture holds no denormals below 61 x 81"
        got = tuple(denormals(a) for a in steps[-1][:3])
        need = 100 if big else 5 if cells >= 63 else 1
        assert min(got) >= need, f"{case}: denormal cells in (v, d, p) {got}, need {need} in each"
        return got
    if case.name == "zeros":
        v, d, p = steps[0][:3]
        got = (negative_zeros(d), negative_zeros(p))
        if big and case.nu == 0:   # (a diffusion leaves no negative zero: its own guard, tests/test_values.py)
            assert min(got) >= 1, f"{case}: -0.0f cells in (d, p) of the first step {got}"
        return got
    return ()


def expected(case):
    """The guard, then the steps: what a GPU test compares with."""
    guard(case)
    return rule_steps(case)


# ---- the members of a batch ------------------------------------------------------------------------------------------------
def member_textures(dim_x, dim_y, viscous=False, masked=False):
    """(name, amplitude) of every member of a batch of this shape: the quiescent ones only where they hold denormals."""
    quiet = [("quiescent", a) for a in amplitudes(viscous, masked)] if dim_x * dim_y >= SKETCH else []
    return quiet + [("tiny", None), ("zeros", None), ("dense", None)]


# per member, cycled: dt, dx in {1.0, 0.37}, iters and omega of its own
EACH = dict(dt=(1 / 30.0, 1 / 60.0, 1 / 20.0, 1 / 30.0, 1 / 45.0), dx=(0.37, 1.0, 0.37, 1.0, 0.37), iters=(6, 9, 7, 6, 8),
            omega=(1.9, 1.96, 1.5, 1.9, 1.7))
NUS = (0.05, 0.3, 0.05, 0.0, 0.04)          # one member without viscosity
MASKS = {"quiescent": "disc", "tiny": "seeded", "zeros": "disc", "dense": "seeded"}   # (a seeded mask stops a quiescent front)


def batch_cases(dim_x, dim_y, each=False, later=False, solids=False, viscous=False):
    """The members of one batch call as cases."""
    out = []
    for m, (name, amplitude) in enumerate(member_textures(dim_x, dim_y, viscous, solids)):
        prm = {k: v[m % 5] for k, v in EACH.items()} if each else {}
        out.append(Case(name, amplitude, dim_x, dim_y, later=later, mask=MASKS[name] if solids else None,
                        nu=NUS[m % 5] if viscous else 0.0, sweeps=SWEEPS if viscous else 0, **prm))
    return out


SMALL_SHAPES = [(61, 81), (96, 64), (7, 9)]          # 96 x 64: the 6144 cells a small member may have
LARGE_SHAPES = [(96, 96), (128, 128)]
RULED_SHAPES = [(61, 81), (7, 9)]                    # the batches with solids and viscosity
RULED_VARIANTS = {"solids": dict(solids=True), "viscous": dict(viscous=True), "both": dict(solids=True, viscous=True)}
SMALL_CALLS = {"step_n": dict(), "replay": dict(later=True), "each": dict(each=True), "each-replay": dict(each=True, later=True)}
LARGE_CALLS = {"step_n": dict(), "each": dict(each=True)}


def context_textures(dim_x, dim_y, viscous=False, masked=False):
    return member_textures(dim_x, dim_y, viscous, masked)[:-1]      # every texture; the dense one needs no context of its own


def context_cases():
    """what -> the cases of the contexts' steps: plain at the sizes of every step path, masked, viscous."""
    tx, ty, d = _solid_tile()
    out = {}
    for dim_x, dim_y in ((61, 81), (130, 70), (160, 128), (300, 141)):
        out[f"plain-{dim_x}x{dim_y}"] = [Case(n, a, dim_x, dim_y) for n, a in context_textures(dim_x, dim_y)]
    for dim_x, dim_y in ((130, 70), (tx + 1, ty + 1)):
        for iters in (ITERS, 2 * d + 3):
            out[f"masked-{dim_x}x{dim_y}-i{iters}"] = [Case(n, a, dim_x, dim_y, iters=iters, mask="disc") for n, a in context_textures(dim_x, dim_y, masked=True)]
    for mask in (None, "disc"):
        out[f"viscous-130x70-{mask}"] = [Case(n, a, 130, 70, nu=NU, sweeps=SWEEPS, mask=mask) for n, a in context_textures(130, 70, True, mask is not None)]
    return out


def _solid_tile():
    from test_context_solids import D, TX, TY
    return TX, TY, D


def all_cases():
    """Every case tests/test_values_gpu.py steps, once: what tests/test_values.py asserts the guards of."""
    cases = []
    for shape in SMALL_SHAPES:
        for kw in SMALL_CALLS.values():
            cases += batch_cases(*shape, **kw)
    for shape in LARGE_SHAPES:
        for kw in LARGE_CALLS.values():
            cases += batch_cases(*shape, **kw)
    for shape in RULED_SHAPES:
        for kw in RULED_VARIANTS.values():
            cases += batch_cases(*shape, **kw)
    for group in context_cases().values():
        cases += group
    return list(dict.fromkeys(cases))


# ---- the stopping rule with denormal tolerances ----------------------------------------------------------------------------
Until = namedtuple("Until", "dim_x dim_y exp tol omega every cap mask")


def until_rhs(u):
    """A zero-mean standard normal times 2^exp; dx is 1."""
    return (zero_mean(u.dim_x, u.dim_y, 500 + u.dim_x) * F(2.0 ** u.exp)).astype(F)


def until(d, dx, cap, omega, tol, every, solid=None, flush=False):
    """-> (k, the pressure of k iterations from zero, u_k): the stopping rule of include/sfl.h, sfl_member_stop, as
    tests/test_batch_until.py `rule` states it (pinned to it by tests/test_values.py), with a mask by tests/solid_rule.py.
    flush: the norm is passed through `flushed` in front of the comparison -- what a kernel that flushes it decides."""
    norm = (lambda p: F(update_norm(p, d, dx))) if solid is None else (lambda p: F(solid_rule.update_norm(p, d, solid, dx)))
    iterate = (lambda p: sor_iteration(p, d, dx, omega)) if solid is None else (lambda p: solid_rule.iterate(p, d, solid, dx, 1, omega))
    tol, p, k = F(tol), np.zeros_like(d), 0
    while k < cap:
        if k % every == 0:
            u = norm(p)
            seen = flushed(u)[()] if flush else u
            if tol >= 0 and (seen <= tol or np.isnan(seen)):
                return k, p, u
        p = iterate(p)
        k += 1
    return k, p, norm(p)


@functools.lru_cache(maxsize=None)
def until_answer(u, flush=False):
    d = until_rhs(u)
    solid = None if u.mask is None else mask_of(u.mask, u.dim_x, u.dim_y)
    k, p, norm = until(d, 1.0, u.cap, u.omega, u.tol, u.every, solid, flush)
    return (k, *_frozen(p), norm)


def until_class(u):
    k = until_answer(u)[0]
    return "zero" if k == 0 else "early" if k < u.cap else "cap"


# (the k of the rule and of its flushed variant are measured by tests/test_values.py; the caps lie just above the flushed k,
# so that a member that runs to its cap stays short)
UNTIL_SMALL = [Until(7, 9, -110, 1e-40, 1.5, 3, 100, None), Until(7, 9, -120, 1e-42, 1.7, 4, 100, None),
               Until(7, 9, -120, 0.0, 1.7, 1, 100, None)]
UNTIL_SKETCH = [Until(61, 81, -120, 1e-42, 1.7, 4, 272, None), Until(61, 81, -120, 0.0, 1.5, 1, 340, None)]
UNTIL_LARGE = [Until(96, 96, -122, 1e-42, 1.7, 4, 136, None), Until(96, 96, -122, 0.0, 1.5, 1, 120, None)]
UNTIL_GENERAL = [Until(130, 70, -122, 1e-42, 1.7, 4, 112, None), Until(130, 70, -122, 0.0, 1.5, 1, 90, None)]
UNTIL_MASKED = [u._replace(mask="disc") for u in UNTIL_GENERAL]
UNTIL_CLASSES = {"early": UNTIL_SMALL[:2], "cap": UNTIL_SMALL[2:] + UNTIL_SKETCH + UNTIL_LARGE + UNTIL_GENERAL + UNTIL_MASKED}


def until_guard(u):
    """The rule and its flushed variant stop at different k, the flushed one early."""
    k, kf = until_answer(u)[0], until_answer(u, True)[0]
    assert 0 < kf < u.cap and kf != k, f"{u}: the rule stops at {k}, on a flushed norm at {kf}"
    return k, kf


# ---- steps whose solve stops at a denormal tolerance ------------------------------------------------------------------------
UNTIL_STEPS = 2
# per member, cycled: (tol, every); the cap is the member's iters
STOPS = ((1e-42, 4), (0.0, 1), (1e-40, 3), (1e-42, 4), (1e-3, 4))
UNTIL_STEP_SHAPES = [(61, 81, False), (96, 96, True)]          # (dim_x, dim_y, a batch of large members)


def until_step_members(dim_x, dim_y):
    """[(case, tol, every)]: the textures as members of a step_n_until call, the case's iters the cap of its solves."""
    out = []
    for m, (name, amplitude) in enumerate(member_textures(dim_x, dim_y)):
        out.append((Case(name, amplitude, dim_x, dim_y, dx=(DX, 1.0)[m % 2], iters=24, omega=(1.7, 1.5)[m % 2]), *STOPS[m % 5]))
    return out


@functools.lru_cache(maxsize=None)
def until_steps(case, tol, every, flush=False):
    """UNTIL_STEPS steps by the rule: a step's divergence from a step of no iterations, k from `until` on it, the state from
    a step of k iterations.  -> ([k of every step], [u_k of every step], the last state)."""
    from oracle import loader
    cpu = loader.port()
    t = texture(case.name, case.dim_x, case.dim_y, case.amplitude)
    state, ks, us = (t.v, None, None, t.dye), [], []
    for n in range(UNTIL_STEPS):
        step = lambda iters: viscosity_rule.step(cpu, state[0], state[3], F(case.dt), F(case.dx), iters, F(case.omega), forces=forces_of(case, n))
        k, _, u = until(step(0)[1], case.dx, case.iters, case.omega, tol, every, flush=flush)
        state = step(k)
        ks.append(k)
        us.append(u)
    return ks, us, _frozen(*(np.ascontiguousarray(a) for a in state))


def until_step_guard(case, tol, every):
    """A tiny or quiescent member's divergence lies in the denormals, and a flushed norm stops one of its solves elsewhere."""
    ks, _, state = until_steps(case, tol, every)
    if case.name in ("quiescent", "tiny"):
        kf = until_steps(case, tol, every, True)[0]
        assert denormals(state[1]) >= 100 and kf != ks, f"{case}: stops at {ks}, on a flushed norm at {kf}; {denormals(state[1])} denormal cells in d"
    return ks


# ---- the inputs of the operators called one by one, and of the diffusion on its own ------------------------------------------
@functools.lru_cache(maxsize=None)
def held_velocities(name, amplitude, dim_x, dim_y):
    """Two velocities of a texture: its start with the records of step 0 written in, and what three plain steps leave (on
    the quiescent texture the one that holds denormals).  Shared, never written."""
    t = texture(name, dim_x, dim_y, amplitude)
    start = np.array(t.v)
    for i, j, fx, fy in t.forces:
        start[j, i] = (fx, fy)
    return _frozen(start, np.array(rule_steps(Case(name, amplitude, dim_x, dim_y))[-1][0]))


@functools.lru_cache(maxsize=None)
def operator_answers(name, amplitude, dim_x, dim_y, mask=None):
    """[(v, d, p, v - grad p)] for both held velocities: calculate_divergence, poisson_solve and subtract_gradient one by one
    at DX, ITERS and OMEGA, by the oracle or, with a mask, by tests/solid_rule.py.  Guarded: a tiny or quiescent texture
    holds 100 denormal cells in the d and in the p of one of them."""
    from oracle import loader
    cpu = loader.port()
    solid = None if mask is None else mask_of(mask, dim_x, dim_y)
    out = []
    for v in held_velocities(name, amplitude, dim_x, dim_y):
        if solid is None:
            d = cpu.divergence(v, F(DX))
            p = cpu.poisson_solve(d, F(DX), ITERS, F(OMEGA))
            w = cpu.subtract_gradient(v, p, F(DX))
        else:
            d = solid_rule.divergence(v, solid, DX)
            p = solid_rule.solve(d, solid, DX, ITERS, OMEGA)
            w = np.ascontiguousarray(solid_rule.gradient(v, p, solid, DX))
        out.append(_frozen(v, d, p, w))
    if name in ("quiescent", "tiny"):
        got = [(denormals(d), denormals(p)) for _, d, p, _ in out]
        assert max(min(g) for g in got) >= 100, f"{name} {amplitude} {dim_x}x{dim_y} {mask}: denormal cells in (d, p) {got}"
    if name == "zeros":
        got = [(negative_zeros(d), negative_zeros(p)) for _, d, p, _ in out]
        assert min(got[0]) >= 1, f"zeros {dim_x}x{dim_y} {mask}: -0.0f cells in (d, p) {got}"
    return out


@functools.lru_cache(maxsize=None)
def diffusion_answer(name, amplitude, dim_x, dim_y, sweeps, mask=None):
    """(v, the rule's diffusion of it) at NU, DT and DX: the second held velocity, whose denormals the diffusion spreads."""
    solid = None if mask is None else mask_of(mask, dim_x, dim_y)
    v = held_velocities(name, amplitude, dim_x, dim_y)[1 if name != "zeros" else 0]
    want = viscosity_rule.diffuse(v, NU, DT, DX, sweeps, solid)
    if name in ("quiescent", "tiny"):
        assert denormals(want) >= 100, f"{name} {amplitude} {dim_x}x{dim_y} {mask}: {denormals(want)} denormal components after the diffusion"
    return v, want


# ---- tracers that follow the three steps ----------------------------------------------------------------------------------------
TRACERS = 64


@functools.lru_cache(maxsize=None)
def tracer_answer(case):
    """(the start, the positions after the three steps, the samples of velocity, pressure and divergence there) by
    tests/tracer_rule.py: every step advances the tracers by its dt on its projected velocity.  Guarded: on a tiny or
    quiescent case a sample is a denormal -- a tracer reads the bottom of the range."""
    import tracer_rule
    from test_tracers_gpu import starts
    start = starts(case.dim_x, case.dim_y, TRACERS)
    xy = start
    for state in expected(case):
        xy = tracer_rule.advance(state[0], xy, F(case.dt))
    v, d, p, _ = expected(case)[-1]
    samples = tuple(tracer_rule.sample(a, xy[:, 0], xy[:, 1], False) for a in (v, p, d))
    if case.name in ("quiescent", "tiny"):
        got = [denormals(s[~np.isnan(s)]) for s in samples]
        assert min(got) >= 1, f"{case}: denormal samples of (v, p, d) {got}"
    return start, xy, samples
