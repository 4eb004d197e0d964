"""Model-based call sequences on live handles (contexts, groups of slabs, batches): the model, the vocabulary, a seeded
generator and the runner.  tests/test_sequences.py checks all of it without a GPU, tests/test_sequences_gpu.py runs the
sequences on the library.

An op is a pair (kind, {argument: literal}): it can be applied to a model and to a handle and printed as a Python literal.
A model holds whole-domain numpy fields and says what every field must hold after each op; every operation is composed
from the oracle's operators and from the yardsticks the suite already has (tracer_rule, view_rule, update_norm, rule,
sor_iteration, the numpy distance and envelope).  A handle is anything with ``apply(op)``, ``snapshot()`` and ``close()``:
the library behind a Solver or a BatchSolver, or, for the CPU tests, another model.  Results of queries and snapshots are
dicts of numpy arrays, compared bit for bit.

A step is: advect the velocity, write the step's records, divergence, solve, subtract the gradient, advect the dye with the
projected velocity, advance a following tracer set (include/sfl.h: sfl_step, the timeline rule, TRACERS).

Solids and histories are subjects of their own (Subject(solids=True)): while a model holds a mask its step and its operators
follow items 1 to 7 of "SOLIDS" through tests/solid_rule.py, and while it holds a history it appends one record per sample.  A
call include/sfl.h refuses in the state the model is in changes nothing and returns {"refused": ERR_STATE}; the library's
wrappers turn an SflError into the same dict, and the runner compares the state behind a refused op like any other.  The
generator follows the same state from the op list alone (Gate) so that only the refusals it planted happen.

Viscosity and loads are two more subjects (Subject(viscous=True)) on top of the solids' deck: a step with a viscosity in force is
the step above with tests/viscosity_rule.py's diffuse between the forces and the divergence (item 3a of "VISCOSITY", the mask
where one is held), diffuse_velocity is that function alone, a load is tests/load_rule.py's loads of the model's pressure, mask
and labels, compared as the raw bytes of its records, and the loads recorder counts as a history does and appends zero records
while no mask is held.  The refusals the two features add -- set_bodies while the recorder is on, a batch's step_n_until while a
viscosity is set, a step call that a full loads recorder has no room for, loads_history without a recorder -- are in the models
and in the Gate, from the header.

Four more subjects walk what came after.  Subject(records=True), on top of the viscous deck: the friction and the torque recorder
count as the loads recorder does, each for itself, and sample tests/friction_rule.py and tests/torque_rule.py behind the loads
(zero records without a mask, the torque's but for pivot2); the pivots follow the number of bodies; the averages add
tests/mean_rule.py's terms behind the torque's sample, count only while every >= 1, have no capacity and never refuse a step call;
float64 planes are compared as their uint64 bit patterns.  Subject(opens=True), on top of the solids' deck: while a map is set a
step is tests/inflow_rule.py's (item 2a behind the forces, items 4 to 6 of tests/opening_rule.py), the operators of a context
follow items 4, 5, 5 and 6 and never impose the inflow, and the whole-domain queries use the openings' divergence and update
norm; the flux is compared as the raw bytes of its record.  A refusal carries its code: SFL_ERR_STATE, or SFL_ERR_INVALID for a
profile record off the inflow cells, pivots of another number of bodies and a plane outside `what` (csrc/means.cpp download():
"plane %d belongs to group %u, which is not in the mask")."""
import ctypes

import numpy as np

import friction_rule
import inflow_rule
import load_rule
import mean_rule
import opening_rule
import solid_rule
import torque_rule
import tracer_rule
import view_rule
import viscosity_rule
from conftest import assert_bit_equal, random_fields
from dx_cases import DX_A, DX_C, widened
from test_batch_params import gs_target, update_norm
from test_batch_until import rule, sor_iteration
from test_ensemble_gpu import envelope_yardstick
from test_ensemble_gpu import yardstick as distance_yardstick
from test_solids_gpu import mask_of

FV, FC, FD, FP = 0, 1, 2, 3
FIELDS = {FV: "velocity", FC: "colour", FD: "divergence", FP: "pressure"}
TEXTURES = ("noise", "still", "fast", "landing", "whole-cell")
# (dx: 1.0 keeps the kernels compiled for dx = 1 in the walk; at 0.37 and 3.0 no product with the spacing is exact)
DTS, DXS, OMEGAS, MAX_ITERS = (1 / 30.0, 0.1, 0.25), (0.5, 1.0, widened(DX_A), widened(DX_C)), (1.0, 1.5, 1.96), 12
TOLS, EVERYS = (-1.0, 0.01, 0.5, 1e30), (1, 3, 4)
MAX_COLOUR = 0xFC000000
PALETTE = [[0, 0, MAX_COLOUR], [MAX_COLOUR, MAX_COLOUR, MAX_COLOUR], [MAX_COLOUR, 0, 0]]
NAN_COLOUR = (0, MAX_COLOUR, 0)
VIEW_RANGE = {0: (0.0, 200.0), 1: (-100.0, 100.0), 2: (-50.0, 50.0), 3: (-50.0, 50.0)}   # lo, hi of every view
CAPACITY = 128      # trail slots and recorder frames: more than the steps of one sequence (30 ops of at most 4 steps)
FIXED_HALO, SAFE_REACH = 32, 24.0   # slabs: the fixed advection halo the generator sets, and the longest back-trace (rows) it keeps under it

OPTION_VALUES = {"OPT_ADVECT_KERNEL": (0, 1, 2), "OPT_FUSE_DIVERGENCE": (0, 1), "OPT_FUSE_PROJECTION": (0, 1), "OPT_STEP_SEAMS": (0, 1),
                 "OPT_SMALL_GRID": (0, 1), "OPT_SOR_KERNEL": (0, 1, 2), "OPT_SOR_FUSE": (0, 2, 16)}
SLAB_OPTION_VALUES = dict(OPTION_VALUES, OPT_ADVECT_HALO=(0, FIXED_HALO), OPT_SOR_HALO=(0, 16, 32))

CONTEXT_WRITERS = ("upload", "advect_velocity", "advect_color", "calculate_divergence", "poisson_solve", "poisson_continue",
                   "poisson_solve_until", "subtract_gradient", "step", "step_n", "queue_forces", "queue_drags", "forget_forces",
                   "set_tracers", "advance_tracers", "trail_start", "trail_stop", "set_option")
CONTEXT_QUERIES = ("download", "residual", "flow_stats", "view_scalar", "view_texels", "render_rgb565", "sample_tracers", "tracers",
                   "trail", "forces_pending", "last_solve_info", "distance")
SLAB_WRITERS = ("upload", "advect_velocity", "advect_color", "calculate_divergence", "poisson_solve", "subtract_gradient", "step",
                "step_n", "queue_forces", "queue_drags", "forget_forces", "set_option")
SLAB_QUERIES = ("download", "forces_pending", "last_solve_info")
BATCH_WRITERS = ("upload", "step_n", "step_n_each", "step_n_until", "poisson_solve", "poisson_solve_each", "poisson_solve_until",
                 "queue_forces", "forget_forces", "record_start", "record_view", "record_stop", "set_tracers", "envelope")
BATCH_QUERIES = ("download", "flow_stats", "distance", "envelope_field", "residual", "iterations", "render_members",
                 "view_render_members", "frames", "forces_pending", "tracers")
# the solids' and the histories' calls: tuples of their own, dealt only to the subjects made with solids=True (a kind added
# to the tuples above would reshuffle every sequence the other subjects have)
SOLID_WRITERS = ("set_solids", "clear_solids", "history_start", "history_stop")
SOLID_QUERIES = ("solids", "history")
# the viscosity's and the loads' calls, dealt only to the subjects made with viscous=True (on top of the solids' deck)
VISCOUS_WRITERS = ("set_viscosity", "clear_viscosity", "diffuse_velocity", "set_bodies", "clear_bodies", "loads_start", "loads_stop")
VISCOUS_QUERIES = ("viscosity", "bodies", "loads", "loads_history")
BATCH_VISCOUS_WRITERS = tuple(k for k in VISCOUS_WRITERS if k != "diffuse_velocity")      # (a batch has no operator of its own)
# the friction's, the torque's and the averages' calls, dealt only to the subjects made with record=True (on top of the viscous deck)
RECORD_WRITERS = ("friction_start", "friction_stop", "torque_start", "torque_stop", "set_body_pivots", "mean_start", "mean_stop", "mean_sample")
RECORD_QUERIES = ("friction", "friction_history", "torque", "torque_history", "body_pivots", "mean_info", "mean_sums")
# the openings', the profiles' and the flux's calls, dealt only to the subjects made with opens=True (on top of the solids' deck;
# set_viscosity and clear_viscosity are there to plant the refusals: openings and a viscosity refuse each other)
OPEN_WRITERS = ("set_openings", "clear_openings", "set_inflow", "set_inflow_profile", "set_viscosity", "clear_viscosity")
OPEN_QUERIES = ("openings", "inflow_profile", "openings_flux")
QUERIES = set(CONTEXT_QUERIES) | set(BATCH_QUERIES) | set(SOLID_QUERIES) | set(VISCOUS_QUERIES) | set(RECORD_QUERIES) | set(OPEN_QUERIES)
NUS, CONTEXT_SWEEPS, BATCH_SWEEPS = (0.0, 0.05, 0.3, 2.5), (0, 1, 3, 8, 9, 17), (0, 1, 3, 10)
D_DIFFUSE = 8                                           # sweeps of one launch of a context's diffusion (kD of csrc/diffuse_tile.h)
LABEL_KINDS = {"all one": 1, "halves": 2, "with zeros": 3, "sixteen": 16}     # kind -> bodies
LOAD_BYTES = load_rule.DTYPE.itemsize                   # struct sfl_body_load
# (36 ops a sequence: the deck of the solids' subjects leaves out three calls that touch neither a field nor a launch's path)
SOLID_LEFT_OUT = ("queue_drags", "trail_stop", "last_solve_info")
MASK_KINDS = ("one", "disc", "plate", "channel", "isolated", "all", "seeded", "empty")     # mask_of of tests/test_solids_gpu.py
MIXED_KINDS = tuple(k for k in MASK_KINDS if k not in ("all", "empty"))                     # at least one solid and one fluid cell
ERR_STATE, VIEW_DIVERGENCE, D_SOLID = -5, 3, 8      # SFL_ERR_STATE; SFL_VIEW_DIVERGENCE; iterations of one launch of the masked solve
ERR_INVALID = -1                                    # SFL_ERR_INVALID: a profile record off the inflow cells, pivots of another `bodies`, a plane outside `what`
REFUSED = {"refused": np.int32(ERR_STATE)}


def refusal(code):
    """What a refused call returns: refuses() of a model says True (SFL_ERR_STATE) or the code itself."""
    return {"refused": np.int32(ERR_STATE if code is True else code)}


# struct sfl_history_record (HISTORY_DTYPE of the package): field -> dtype
HISTORY_FIELDS = {"max_abs_vx": np.float32, "max_abs_vy": np.float32, "max_abs_div": np.float32, "what": np.uint32, "dye_sum": np.uint64,
                  "update_norm": np.float32, "iterations": np.int32, "step": np.int64, "dt": np.float32, "dx": np.float32}


def solid_mask(kind, dim_x, dim_y, seed, member=None):
    """The mask a set_solids op sets; per member: member k takes the k-th kind behind `kind` and its own seed."""
    if member is not None:
        kind, seed = MASK_KINDS[(MASK_KINDS.index(kind) + member) % len(MASK_KINDS)], seed + member
    return mask_of(kind, dim_x, dim_y, seed)


def body_labels(kind, dim_x, dim_y, seed, member=None):
    """The labels a set_bodies op sets over the WHOLE grid, fluid cells included: None ("all one": every solid cell is body 1),
    two bodies split at the middle column, a seeded third of the cells in no body, or 1 + (i + j) % 16.  Per member: member k
    shifts the pattern by k cells and takes its own seed."""
    if kind == "all one":
        return None
    k = member or 0
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    if kind == "halves":
        lab = np.where(i + k < dim_x // 2, 1, 2)
    elif kind == "sixteen":
        lab = 1 + (i + j + k) % 16
    else:
        lab = np.where(np.random.default_rng([seed, k, 5]).random((dim_y, dim_x)) < 1 / 3.0, 0, 1 + (i + 2 * j + k) % 3)
    return lab.astype(np.uint8)


def load_bytes(records):
    """sfl_body_load records as their raw bytes, uint8[..., 48]: what the loads are compared as."""
    records = np.ascontiguousarray(records)
    return records.view(np.uint8).reshape(records.shape + (LOAD_BYTES,))


def raw_bytes(records):
    """Records of any of the structs (48, 64 or 40 bytes each) as their raw bytes, uint8[..., itemsize]."""
    records = np.asarray(records)
    return np.ascontiguousarray(records).reshape(-1).view(np.uint8).reshape(records.shape + (records.dtype.itemsize,))


PIVOT_KINDS = ("centre", "seeded")
MEAN_WHATS = (1, 2, 4, 8, 3, 6, 9, 12, 7, 15)          # masks of one group, of several and of all four
OPEN_KINDS = ("channel", "inflow only", "outflow only", "every rim cell", "seeded", "single inflow", "none")
LIVE_OPEN_KINDS = ("channel", "every rim cell", "seeded")       # an inflow and an outflow cell, whatever the seed
INFLOWS = ((12.5, 0.0), (-3.0, 2.5), (0.0, 0.0), (40.0, -7.25))   # the uniform inflow velocities the generator draws from
FLUX_BYTES = inflow_rule.FLUX_DTYPE.itemsize            # struct sfl_open_flux


def body_pivots_of(kind, bodies, dim_x, dim_y, seed, member=None):
    """The pivots a set_body_pivots op sets, int32[bodies, 2] in HALF cells, none of them (0, 0): the centre of the grid (a half
    cell where the side is even) or seeded ones, inside the grid and outside it, odd and negative.  Per member: its own."""
    k = member or 0
    if kind == "centre":
        return np.tile(np.array([dim_x - 1 + 2 * k, dim_y - 1], np.int32), (bodies, 1))
    p = np.random.default_rng([seed, k, 9]).integers(-2 * dim_x, 4 * dim_x, (bodies, 2))
    p[(p == 0).all(axis=1)] = (1, -3)
    return p.astype(np.int32)


def open_map(kind, dim_x, dim_y, seed, member=None):
    """The map a set_openings op sets, uint8[dim_y, dim_x] of 0, INFLOW and OUTFLOW, nonzero only on rim cells that are no corners:
    a channel (the W rim in, the E rim out), inflow only (the incompatible Neumann problem), outflow only (the E and the N rim),
    every non-corner rim cell open with the bytes alternating, a seeded third of the rim cells each way, one inflow cell in the
    middle of the W rim, and no opening at all (the solids' bits).  Per member: member k takes the k-th kind behind `kind` and
    its own seed."""
    if member is not None:
        kind, seed = OPEN_KINDS[(OPEN_KINDS.index(kind) + member) % len(OPEN_KINDS)], seed + member
    m = np.zeros((dim_y, dim_x), np.uint8)
    j, i = np.mgrid[0:dim_y, 0:dim_x]
    rim = ((i == 0).astype(int) + (i == dim_x - 1) + (j == 0) + (j == dim_y - 1)) == 1
    if kind == "channel":
        m[rim & (i == 0)], m[rim & (i == dim_x - 1)] = opening_rule.INFLOW, opening_rule.OUTFLOW
    elif kind == "inflow only":
        m[rim & (i == 0)] = opening_rule.INFLOW
    elif kind == "outflow only":
        m[rim & ((i == dim_x - 1) | (j == dim_y - 1))] = opening_rule.OUTFLOW
    elif kind == "every rim cell":
        m[rim] = (1 + (i + j + seed) % 2)[rim]
    elif kind == "seeded":
        m[rim] = np.random.default_rng([seed, 17]).integers(0, 3, int(rim.sum()))
        m[dim_y // 2, 0], m[dim_y // 2, dim_x - 1] = opening_rule.INFLOW, opening_rule.OUTFLOW      # (never without a cell of each kind)
    elif kind == "single inflow":
        m[dim_y // 2, 0] = opening_rule.INFLOW
    else:
        assert kind == "none"
    assert opening_rule.check_map(m) is None
    return m


def live_cells(open, mask):
    """(live inflow cells, live outflow cells) of one grid: an opening counts only where the cell is fluid."""
    fluid = np.ones(open.shape, bool) if mask is None else ~mask
    return int(((open == opening_rule.INFLOW) & fluid).sum()), int(((open == opening_rule.OUTFLOW) & fluid).sum())


def profile_arrays(profile):
    """The records held as inflow_profile returns them: cells int32[n, 2] (i, j) and vel float32[n, 2], in cell-index order."""
    rows = inflow_rule.unique(profile or [])
    return (np.array([c for c, _ in rows], np.int32).reshape(-1, 2), np.array([uv for _, uv in rows], np.float32).reshape(-1, 2))


def launches_of(nu, sweeps):
    """The launches of a context's diffusion: none where it is skipped, else ceil(sweeps / 8)."""
    return 0 if np.float32(nu) == 0 or sweeps == 0 else -(-sweeps // D_DIFFUSE)


def mixed(mask):
    return mask is not None and bool(mask.any()) and not bool(mask.all())


def masked_rule(d, solid, dx, cap, omega, tol, every):
    """`rule` of tests/test_batch_until.py with the solids' iterations and their update norm: (k, p of k iterations, u_k)."""
    tol, p, k = np.float32(tol), np.zeros_like(d), 0
    while k < cap:
        if k % every == 0:
            u = np.float32(solid_rule.update_norm(p, d, solid, dx))
            if tol >= 0 and (u <= tol or np.isnan(u)):
                return k, p, u
        p = solid_rule.iterate(p, d, solid, dx, 1, omega)
        k += 1
    return k, p, np.float32(solid_rule.update_norm(p, d, solid, dx))


def open_rule_until(d, solid, open, dx, cap, omega, tol, every):
    """masked_rule with the openings' iterations and their update norm (the k of item 5 of "OPENINGS")."""
    tol, p, k = np.float32(tol), np.zeros_like(d), 0
    while k < cap:
        if k % every == 0:
            u = np.float32(opening_rule.update_norm(p, d, solid, open, dx))
            if tol >= 0 and (u <= tol or np.isnan(u)):
                return k, p, u
        p = opening_rule.iterate(p, d, solid, open, dx, 1, omega)
        k += 1
    return k, p, np.float32(opening_rule.update_norm(p, d, solid, open, dx))


def samples_due(hist, n):
    """How many samples n more steps complete, and how many are free (include/sfl.h "COUNTING")."""
    return (hist["steps"] + n) // hist["every"] - hist["steps"] // hist["every"], hist["capacity"] - len(hist["records"])


def history_result(hist, shape):
    recs = hist["records"]
    out = {name: (np.stack([r[name] for r in recs]) if recs else np.zeros((0,) + shape + ((3,) if name == "dye_sum" else ()), dtype))
           for name, dtype in HISTORY_FIELDS.items()}
    out["info"] = np.array([len(recs), hist["capacity"], hist["steps"]], np.int64)
    return out


def texture(kind, field, dim_x, dim_y, seed):
    """The field an upload op writes: all of it behaviour the reference defines.  Dye covers [0, 0xFF000000) whatever the kind."""
    rng = np.random.default_rng([seed, field, TEXTURES.index(kind)])
    shape = (dim_y, dim_x) + {FV: (2,), FC: (3,), FD: (), FP: ()}[field]
    if field == FC:
        return rng.integers(0, 0xFF000000, shape, dtype=np.uint32)
    if kind == "noise":
        v, _, s = random_fields(dim_x, dim_y, seed)
        return v if field == FV else s
    if kind == "still":
        return np.zeros(shape, np.float32)
    if kind == "fast":
        return (rng.uniform(-1, 1, shape) * 1500.0).astype(np.float32)
    if kind == "landing":       # with dt = 0.25 every back-trace source is an exact quarter-lattice point
        return rng.integers(-32, 33, shape).astype(np.float32)
    return (4 * rng.integers(-8, 9, shape)).astype(np.float32)      # whole-cell: displacements of whole cells at dt = 0.25


def as_result(**arrays):
    return {k: np.asarray(a) for k, a in arrays.items()}


def compare(got, want, what):
    assert sorted(got) == sorted(want), (what, sorted(got), sorted(want))
    for name in want:
        g, w = np.asarray(got[name]), np.asarray(want[name])
        if w.dtype in (np.float32, np.uint32):
            assert_bit_equal(np.ascontiguousarray(g, w.dtype), np.ascontiguousarray(w), f"{what}: {name}")
        elif w.dtype == np.float64:          # as the uint64 bit patterns: a NaN equals itself, +0.0 is not -0.0; no cast on either side
            assert g.dtype == np.float64 and g.shape == w.shape, f"{what}: {name}: got {g.dtype}{g.shape}, want float64{w.shape}"
            gb, wb = np.ascontiguousarray(g).view(np.uint64), np.ascontiguousarray(w).view(np.uint64)
            bad = np.argwhere(gb != wb)
            assert not len(bad), (f"{what}: {name}: {len(bad)} of {gb.size} doubles differ bitwise; first at {tuple(bad[0])}: got {g[tuple(bad[0])]!r} "
                                  f"(0x{int(gb[tuple(bad[0])]):016x}) want {w[tuple(bad[0])]!r} (0x{int(wb[tuple(bad[0])]):016x})")
        else:
            assert g.shape == w.shape and np.array_equal(g, w.astype(g.dtype)), f"{what}: {name}: got {g!r}, want {w!r}"


def view_texels(what, v, p, dx):
    lo, hi = VIEW_RANGE[what]
    return view_rule.view_texels(what, v, p, dx, np.float32(lo), np.float32(hi), PALETTE, NAN_COLOUR)


def stats_record(oracle, v, c, dx):
    with np.errstate(all="ignore"):
        return as_result(max_abs_vx=np.max(np.abs(v[..., 0])), max_abs_vy=np.max(np.abs(v[..., 1])),
                         max_abs_div=np.max(np.abs(oracle.divergence(v, dx))), dye_sum=c.astype(np.uint64).sum(axis=(0, 1)))


def distance_record(a, b):
    """numpy's distance of (v, c, p) fields a from b, as the arrays of a sfl_field_distance record."""
    w = distance_yardstick(a, b)
    return as_result(max_abs_dvx=np.float32(w["max_abs_dvx"]), max_abs_dvy=np.float32(w["max_abs_dvy"]), max_abs_dp=np.float32(w["max_abs_dp"]),
                     velocity_cells_differ=np.uint32(w["velocity_cells_differ"]), dye_cells_differ=np.uint32(w["dye_cells_differ"]),
                     pressure_cells_differ=np.uint32(w["pressure_cells_differ"]), max_abs_ddye=np.array(w["max_abs_ddye"], np.uint32),
                     sum_abs_ddye=np.array(w["sum_abs_ddye"], np.uint64))


# ---- the model of a context (a group of slabs holds the same whole-domain fields) ------------------------------------
class ContextModel:
    def __init__(self, oracle, dim_x, dim_y):
        self.o, self.dim_x, self.dim_y = oracle, dim_x, dim_y
        self.v = np.zeros((dim_y, dim_x, 2), np.float32)
        self.c = np.zeros((dim_y, dim_x, 3), np.uint32)
        self.d = np.zeros((dim_y, dim_x), np.float32)
        self.p = np.zeros((dim_y, dim_x), np.float32)
        self.timeline = {}                       # step -> [((i, j), (vx, vy)), ...] in queue order
        self.xy, self.follow, self.trail = None, False, None   # trail: [every, advances, [slots]]
        self.reach = 0.0                         # the longest back-trace along j (rows) of the advections of the last op
        self.peer = None                         # (a model used as a handle: the model it is compared with)
        self.mask = None                         # the solids: None or bool[dim_y, dim_x]
        self.hist = None                         # the history: {"every", "capacity", "steps", "records"}
        self.viscous = False                     # (the viscosity's and the loads' queries are among those of queries())
        self.visc = None                         # the viscosity: None or (nu, sweeps) with nu > 0 and sweeps > 0
        self.labels, self.bodies = None, 1       # the bodies: None (every solid cell is body 1) or uint8[dim_y, dim_x]
        self.loads = None                        # the loads recorder: {"every", "capacity", "steps", "records"}
        self.records = False                     # (the friction's, the torque's and the averages' queries are among those of queries())
        self.pivots = None                       # the pivots: None (every pivot (0, 0)) or int32[bodies, 2] in half cells
        self.friction = self.torque = None       # the friction and the torque recorder, each as the loads recorder
        self.means = None                        # the averages: {"what", "every", "steps", "samples", "sums": {plane: [1, dim_y, dim_x]}}
        self.opens = False                       # (the openings' queries are among those of queries())
        self.open = None                         # the openings: None or uint8[dim_y, dim_x]
        self.inflow = (0.0, 0.0)                 # the uniform inflow velocity
        self.profile = None                      # the inflow profile: None or [((i, j), (u, v))] as given, the later record wins

    # -- plumbing
    def apply(self, op):
        kind, args = op
        self.reach = 0.0
        code = self.refuses(kind, args)
        if code:                                 # refused whole: nothing changes
            return refusal(code)
        return getattr(self, ("q_" if kind in QUERIES else "do_") + kind)(**args)

    def refuses(self, kind, a):
        """Whether include/sfl.h refuses the call in the state the model is in: False, True for SFL_ERR_STATE, or the code
        itself where it is another (ERR_INVALID: the records of a profile against the map, pivots of another `bodies`, a plane
        outside `what`; the library checks those behind the state)."""
        if (self.mask is not None or self.open is not None) and kind in ("view_scalar", "view_texels") and a["what"] == VIEW_DIVERGENCE:
            return True
        if kind in ("set_bodies", "clear_bodies") and not (self.loads is None and self.friction is None and self.torque is None):
            return True
        if kind in ("loads_history", "friction_history", "torque_history") and getattr(self, kind[:-len("_history")]) is None:
            return True
        for recorder in (self.hist, self.loads, self.friction, self.torque):       # (the averages have no capacity: they never refuse)
            if recorder is not None and kind in ("step", "step_n"):
                due, free = samples_due(recorder, a.get("n", 1))
                if due > free:
                    return True
        if kind == "set_body_pivots" and a["pivot_kind"] is not None and a["bodies"] != self.bodies:
            return ERR_INVALID
        if kind in ("mean_sample", "mean_sums") and self.means is None:
            return True
        if kind == "mean_sums" and not self.means["what"] & mean_rule.GROUP_OF[a["plane"]]:
            return ERR_INVALID                   # csrc/means.cpp download(): "plane %d belongs to group %u, which is not in the mask"
        # "OPENINGS OF A CONTEXT": openings and a viscosity refuse each other; without openings no inflow and no profile
        if kind == "set_openings" and self.visc is not None:
            return True
        if kind == "set_viscosity" and self.open is not None and not (np.float32(a["nu"]) == 0 or a["sweeps"] == 0):
            return True
        if kind == "set_inflow" and self.open is None:
            return True
        if kind == "set_inflow_profile" and a["cells"]:
            if self.open is None:
                return True
            if inflow_rule.check_profile(list(zip(map(tuple, a["cells"]), a["vels"])), self.open) is not None:
                return ERR_INVALID
        return False

    def close(self):
        pass

    def fields(self):
        return {"velocity": self.v, "colour": self.c, "divergence": self.d, "pressure": self.p}

    def snapshot(self):
        out = as_result(**self.fields())
        if self.xy is not None:
            out["tracers"] = self.xy
        return out

    def finite(self):
        return all(np.isfinite(a).all() for a in (self.v, self.d, self.p)) and (self.xy is None or bool(np.isfinite(self.xy).all()))

    def _advect(self, field, dt, no_slip):
        with np.errstate(all="ignore"):
            self.reach = max(self.reach, float(np.max(np.abs(self.v[..., 1]))) * dt)
        adv = self.o.advect_vec2f if field.dtype == np.float32 else self.o.advect_vec3uq32
        return adv(field, self.v, dt, no_slip)

    def _advance(self, dt):
        self.xy = tracer_rule.advance(self.v, self.xy, dt)
        if self.trail is not None:
            self.trail[1] += 1
            if self.trail[1] % self.trail[0] == 0:
                self.trail[2].append(self.xy.copy())

    def step_once(self, dt, dx, iters, omega, until=None):
        """One step; with until = (tol, every) the solve stops by the rule.  Returns (iterations, update norm or None)."""
        records = self.timeline.pop(0, [])
        self.timeline = {s - 1: r for s, r in self.timeline.items()}
        va = self._advect(self.v, dt, True)
        for (i, j), u in records:
            if 0 <= i < self.dim_x and 0 <= j < self.dim_y:
                va[j, i] = u
        k, u = iters, None
        if self.open is not None:                # item 2a of "OPENINGS" and of "INFLOW PROFILES": behind the forces, on the fluid inflow cells
            inflow_rule.impose(va, self.mask, self.open, self.inflow, self.profile or [])
        if self.mask is not None:                # items 3 to 6 of "SOLIDS"; the records above stand between items 1 and 3
            va[self.mask] = 0.0
        va = self._diffuse(va, dt, dx)           # item 3a of "VISCOSITY": between the forces (the solids zeroed) and the divergence
        if self.open is not None:                # items 4 to 6 of "OPENINGS", with and without a mask (no viscosity and no _until under a map)
            self.d = opening_rule.divergence(va, self.mask, self.open, dx)
            self.p = opening_rule.solve(self.d, self.mask, self.open, dx, k, omega)
            self.v = np.ascontiguousarray(opening_rule.gradient(va, self.p, self.mask, self.open, dx))
        elif self.mask is not None:
            self.d = solid_rule.divergence(va, self.mask, dx)
            if until is not None:
                k, _, u = masked_rule(self.d, self.mask, dx, iters, omega, until[0], until[1])
            self.p = solid_rule.solve(self.d, self.mask, dx, k, omega)
            self.v = np.ascontiguousarray(solid_rule.gradient(va, self.p, self.mask, dx))
        else:
            self.d = self.o.divergence(va, dx)
            if until is not None:
                k, _, u = rule(self.d, dx, iters, omega, until[0], until[1])
            self.p = self.o.poisson_solve(self.d, dx, k, omega)
            self.v = self.o.subtract_gradient(va, self.p, dx)
        self.c = self._advect(self.c, dt, False)
        if self.follow and self.xy is not None:
            self._advance(dt)
        return k, u

    def _diffuse(self, va, dt, dx):
        if self.visc is None:
            return va
        return np.ascontiguousarray(viscosity_rule.diffuse(va, self.visc[0], dt, dx, self.visc[1], self.mask))

    def load_records(self):
        """The `bodies` records of "LOADS" from the pressure, the mask and the labels held; zeros while no mask is."""
        if self.mask is None:
            return np.zeros(self.bodies, load_rule.DTYPE)
        return load_rule.loads(self.p, self.mask, self.labels, self.bodies)

    # -- writers
    def do_upload(self, field, texture_kind, seed):
        a = texture(texture_kind, field, self.dim_x, self.dim_y, seed)
        if field == FV: self.v = a
        elif field == FC: self.c = a
        elif field == FD: self.d = a
        else: self.p = a

    def do_advect_velocity(self, dt, no_slip):
        self.v = self._advect(self.v, dt, no_slip)

    def do_advect_color(self, dt, no_slip):
        self.c = self._advect(self.c, dt, no_slip)

    # The operators of a context under a map follow items 4, 5, 5 and 6 of "OPENINGS" and never impose the inflow.
    def do_calculate_divergence(self, dx):
        if self.open is not None:
            self.d = opening_rule.divergence(self.v, self.mask, self.open, dx)
        elif self.mask is not None:              # 0 in solid cells; the velocity is not touched
            self.d = solid_rule.divergence(self.v, self.mask, dx)
        else:
            self.d = self.o.divergence(self.v, dx)

    def do_poisson_solve(self, dx, iters, omega):
        if self.open is not None:
            self.p = opening_rule.solve(self.d, self.mask, self.open, dx, iters, omega)
        elif self.mask is not None:              # from p = 0
            self.p = solid_rule.solve(self.d, self.mask, dx, iters, omega)
        else:
            self.p = self.o.poisson_solve(self.d, dx, iters, omega)

    def do_poisson_continue(self, dx, iters, omega):
        if self.open is not None:
            self.p = opening_rule.iterate(self.p, self.d, self.mask, self.open, dx, iters, omega)
            return
        if self.mask is not None:                # solid cells keep what they hold
            self.p = solid_rule.iterate(self.p, self.d, self.mask, dx, iters, omega)
            return
        for _ in range(iters):
            self.p = sor_iteration(self.p, self.d, dx, omega)

    def do_poisson_solve_until(self, dx, iters, omega, tol, every):
        if self.open is not None:
            k, _, u = open_rule_until(self.d, self.mask, self.open, dx, iters, omega, tol, every)
            self.p = opening_rule.solve(self.d, self.mask, self.open, dx, k, omega)
        elif self.mask is not None:
            k, _, u = masked_rule(self.d, self.mask, dx, iters, omega, tol, every)
            self.p = solid_rule.solve(self.d, self.mask, dx, k, omega)
        else:
            k, _, u = rule(self.d, dx, iters, omega, tol, every)
            self.p = self.o.poisson_solve(self.d, dx, k, omega)
        return as_result(iterations=np.int32(k), norm=np.float32(u))

    def do_subtract_gradient(self, dx):
        if self.open is not None:
            self.v = np.ascontiguousarray(opening_rule.gradient(self.v, self.p, self.mask, self.open, dx))
        elif self.mask is not None:              # (0, 0) in solid cells
            self.v = np.ascontiguousarray(solid_rule.gradient(self.v, self.p, self.mask, dx))
        else:
            self.v = self.o.subtract_gradient(self.v, self.p, dx)

    def history_record(self, step, dt, dx, iterations):
        """One sfl_history_record of the fields as they stand: what flow_stats and residual return, and the step's words."""
        out = dict(self.q_flow_stats(dx), what=np.uint32(3), update_norm=self.q_residual(dx)["norm"], iterations=np.int32(iterations),
                   step=np.int64(step), dt=np.float32(dt), dx=np.float32(dx))
        return {name: np.asarray(out[name], dtype) for name, dtype in HISTORY_FIELDS.items()}

    def _counted_step(self, dt, dx, iters, omega):
        k, _ = self.step_once(dt, dx, iters, omega)
        if self.hist is not None:
            self.hist["steps"] += 1
            if self.hist["steps"] % self.hist["every"] == 0:
                self.hist["records"].append(self.history_record(self.hist["steps"], dt, dx, k))
        if self.loads is not None:
            self.loads["steps"] += 1
            if self.loads["steps"] % self.loads["every"] == 0:
                self.loads["records"].append(self.load_records()[None])
        # behind a step the order is history, loads, friction, torque, averages; every recorder counts for itself
        for recorder, records_of in ((self.friction, self.friction_records), (self.torque, self.torque_records)):
            if recorder is not None:
                recorder["steps"] += 1
                if recorder["steps"] % recorder["every"] == 0:
                    recorder["records"].append(records_of()[None])
        self.mean_step()

    def friction_records(self):
        """The `bodies` records of "FRICTION" from the velocity, the mask and the labels held; zeros while no mask is."""
        if self.mask is None:
            return np.zeros(self.bodies, friction_rule.DTYPE)
        return friction_rule.friction(self.v, self.mask, self.labels, self.bodies)

    def torque_records(self):
        """The `bodies` records of "TORQUE" about the pivots held; zeros but for pivot2 while no mask is."""
        if self.mask is None:
            out = np.zeros(self.bodies, torque_rule.DTYPE)
            if self.pivots is not None:
                out["pivot2"] = self.pivots
            return out
        return torque_rule.torque(self.p, self.v, self.mask, self.labels, self.bodies, self.pivots)

    def mean_step(self):
        """"AVERAGES": with every >= 1 steps count across calls and a sample is due behind step (s + 1) * every; with every == 0
        no hook is set and nothing counts."""
        m = self.means
        if m is not None and m["every"] >= 1:
            m["steps"] += 1
            if m["steps"] % m["every"] == 0:
                self.mean_add()

    def mean_add(self):
        m = self.means
        mean_rule.add(m["sums"], m["what"], self.v[None], self.p[None], self.c[None])
        m["samples"] += 1

    def do_step(self, dt, dx, iters, omega):
        self._counted_step(dt, dx, iters, omega)

    def do_step_n(self, n, dt, dx, iters, omega):
        for _ in range(n):
            self._counted_step(dt, dx, iters, omega)

    # Setting or clearing a mask touches no field (include/sfl.h sfl_set_solids).
    def do_set_solids(self, mask_kind, seed):
        self.mask = solid_mask(mask_kind, self.dim_x, self.dim_y, seed)

    def do_clear_solids(self):
        self.mask = None

    def do_history_start(self, every, capacity):
        self.hist = {"every": every, "capacity": capacity, "steps": 0, "records": []}

    def do_history_stop(self):
        self.hist = None

    # "VISCOSITY": nu == 0 or sweeps == 0 clears it; sfl_diffuse_velocity is item 3a alone (nothing zeroed, no other field touched)
    def do_set_viscosity(self, nu, sweeps):
        self.visc = None if np.float32(nu) == 0 or sweeps == 0 else (nu, sweeps)

    def do_clear_viscosity(self):
        self.visc = None

    def do_diffuse_velocity(self, nu, dt, dx, sweeps):
        self.v = np.ascontiguousarray(viscosity_rule.diffuse(self.v, nu, dt, dx, sweeps, self.mask))

    # "LOADS": labels and masks are independent of each other; a restart of the recorder starts afresh
    def do_set_bodies(self, label_kind, bodies, seed):
        before = self.bodies
        self.labels = body_labels(label_kind, self.dim_x, self.dim_y, seed)
        self.bodies = 1 if self.labels is None else bodies
        if self.bodies != before:                # "TORQUE": the pivots are per body; the same number keeps them
            self.pivots = None

    def do_clear_bodies(self):
        self.do_set_bodies("all one", 1, 0)

    def do_loads_start(self, every, capacity):
        self.loads = {"every": every, "capacity": capacity, "steps": 0, "records": []}

    def do_loads_stop(self):
        self.loads = None

    # "FRICTION", "TORQUE": recorders of their own beside the loads'; a restart starts afresh.  A set_bodies that changes the
    # number of bodies puts every pivot back to (0, 0) (do_set_bodies below goes through _bodies_changed).
    def do_friction_start(self, every, capacity):
        self.friction = {"every": every, "capacity": capacity, "steps": 0, "records": []}

    def do_friction_stop(self):
        self.friction = None

    def do_torque_start(self, every, capacity):
        self.torque = {"every": every, "capacity": capacity, "steps": 0, "records": []}

    def do_torque_stop(self):
        self.torque = None

    def do_set_body_pivots(self, pivot_kind, bodies, seed):
        self.pivots = None if pivot_kind is None else body_pivots_of(pivot_kind, bodies, self.dim_x, self.dim_y, seed)

    # "AVERAGES": a start while on begins anew from zero; a sample adds the fields held, every cell as it is
    def do_mean_start(self, what, every):
        self.means = {"what": what, "every": every, "steps": 0, "samples": 0, "sums": mean_rule.start(what, (1, self.dim_y, self.dim_x))}

    def do_mean_stop(self):
        self.means = None

    def do_mean_sample(self):
        self.mean_add()

    # "OPENINGS OF A CONTEXT", "INFLOW PROFILES AND FLUX": no field is touched; a new map drops the profile, a new uniform inflow
    # keeps it, a cleared map takes the profile with it; a record on a solid inflow cell is kept (step_once looks at the mask held)
    def do_set_openings(self, open_kind, seed, inflow):
        self.open, self.inflow, self.profile = open_map(open_kind, self.dim_x, self.dim_y, seed), tuple(inflow), None

    def do_clear_openings(self):
        self.open, self.inflow, self.profile = None, (0.0, 0.0), None

    def do_set_inflow(self, inflow):
        self.inflow = tuple(inflow)

    def do_set_inflow_profile(self, cells, vels):
        self.profile = [(tuple(c), tuple(u)) for c, u in zip(cells, vels)] or None

    # The timeline rule of include/sfl.h: "A step call of n steps consumes the records of steps [0, n).  Later records move down
    # by n.  This applies to sfl_step (n = 1), sfl_step_n, ..." and "Solves, uploads, setup and render calls neither consume nor
    # shift": step_once is the only place that touches it; the stand-alone operators leave it alone.
    def do_queue_forces(self, step, cells, vels):
        self.timeline.setdefault(step, []).extend((tuple(cell), tuple(np.float32(x) for x in u)) for cell, u in zip(cells, vels))

    def do_queue_drags(self, step, drags):     # cell = index(coords.y, coords.x), velocity = (velocity.y, velocity.x)
        self.do_queue_forces(step, [(cy, cx) for cx, cy, _, _ in drags], [(vy, vx) for _, _, vx, vy in drags])

    def do_forget_forces(self):
        self.timeline = {}

    def do_set_tracers(self, xy, follow):
        self.xy, self.follow, self.trail = np.array(xy, np.float32), bool(follow), None

    def do_advance_tracers(self, dt):
        self._advance(dt)

    def do_trail_start(self, every):
        self.trail = [every, 0, []]

    def do_trail_stop(self):
        self.trail = None

    def do_set_option(self, name, value):      # an option never changes a result
        pass

    # -- queries
    def q_download(self, field):
        return as_result(field=self.fields()[FIELDS[field]])

    def q_residual(self, dx):
        if self.open is not None:                # the whole-domain queries use the openings' update norm and divergence while a map is set
            return as_result(norm=np.float32(opening_rule.update_norm(self.p, self.d, self.mask, self.open, dx)))
        if self.mask is not None:                # over the fluid cells; 0.0f without one
            return as_result(norm=np.float32(solid_rule.update_norm(self.p, self.d, self.mask, dx)))
        return as_result(norm=np.float32(update_norm(self.p, self.d, dx)))

    def q_flow_stats(self, dx):
        out = stats_record(self.o, self.v, self.c, dx)
        if self.open is not None:
            with np.errstate(all="ignore"):
                out["max_abs_div"] = np.asarray(np.max(np.abs(opening_rule.divergence(self.v, self.mask, self.open, dx))))
        elif self.mask is not None:
            with np.errstate(all="ignore"):
                out["max_abs_div"] = np.asarray(np.max(np.abs(solid_rule.divergence(self.v, self.mask, dx))))
        return out

    def q_solids(self):
        on = self.mask is not None
        return as_result(mask=self.mask if on else np.zeros((self.dim_y, self.dim_x), bool), set=on, solid_cells=int(self.mask.sum()) if on else 0)

    def q_history(self):
        return history_result(self.hist, ())

    def q_viscosity(self):
        nu, sweeps = (0.0, 0) if self.visc is None else self.visc
        return as_result(nu=np.float32(nu), sweeps=sweeps)

    def q_bodies(self):
        labels = np.ones((self.dim_y, self.dim_x), np.uint8) if self.labels is None else self.labels
        return as_result(labels=labels, bodies=self.bodies, labelled=self.labels is not None)

    def q_loads(self):
        return as_result(records=load_bytes(self.load_records()[None]))

    def q_loads_history(self):
        recs = self.loads["records"]
        stacked = np.stack(recs) if recs else np.zeros((0, 1, self.bodies), load_rule.DTYPE)
        return as_result(records=load_bytes(stacked), info=np.array([len(recs), self.loads["capacity"], self.loads["steps"], self.bodies], np.int64))

    def _recorded(self, recorder, dtype):
        recs = recorder["records"]
        stacked = np.stack(recs) if recs else np.zeros((0, 1, self.bodies), dtype)
        return as_result(records=raw_bytes(stacked), info=np.array([len(recs), recorder["capacity"], recorder["steps"], self.bodies], np.int64))

    def q_friction(self):
        return as_result(records=raw_bytes(self.friction_records()[None]))

    def q_friction_history(self):
        return self._recorded(self.friction, friction_rule.DTYPE)

    def q_torque(self):
        return as_result(records=raw_bytes(self.torque_records()[None]))

    def q_torque_history(self):
        return self._recorded(self.torque, torque_rule.DTYPE)

    def q_body_pivots(self):
        return as_result(pivot2=np.zeros((self.bodies, 2), np.int32) if self.pivots is None else self.pivots)

    def q_mean_info(self):
        m = self.means
        return as_result(info=np.array([0, 0, 0, 0] if m is None else [m["what"], m["every"], m["samples"], m["steps"]], np.int64))

    def q_mean_sums(self, plane):
        return as_result(plane=self.means["sums"][plane].copy())

    def q_openings(self):
        on = self.open is not None
        live = live_cells(self.open, self.mask) if on else (0, 0)
        return as_result(map=self.open if on else np.zeros((self.dim_y, self.dim_x), np.uint8), inflow=np.array(self.inflow, np.float32), set=on,
                         live=np.array(live, np.int64))

    def q_inflow_profile(self):
        cells, vel = profile_arrays(self.profile)
        return as_result(cells=cells, vel=vel)

    def q_openings_flux(self):
        if self.open is None:
            return as_result(record=np.zeros(FLUX_BYTES, np.uint8))
        return as_result(record=raw_bytes(inflow_rule.flux(self.v, self.open, self.mask)))

    def q_view_scalar(self, what, dx):
        return as_result(scalar=view_rule.scalar(what, self.v, self.p, dx))

    def q_view_texels(self, what, dx):
        return as_result(texels=view_texels(what, self.v, self.p, dx))

    def q_render_rgb565(self, scaling, byteswap):
        return as_result(image=view_rule.render(self.c, scaling, byteswap))

    def q_sample_tracers(self, field, no_slip):
        return as_result(samples=tracer_rule.sample(self.fields()[FIELDS[field]], self.xy[:, 0], self.xy[:, 1], no_slip))

    def q_tracers(self):
        return as_result(xy=self.xy)

    def q_trail(self):
        slots = self.trail[2]
        return as_result(slots=np.stack(slots) if slots else np.zeros((0,) + self.xy.shape, np.float32))

    def q_forces_pending(self):
        return as_result(records=sum(len(r) for r in self.timeline.values()), last_step=max(self.timeline, default=-1))

    def q_last_solve_info(self):               # launches and fuse depth are the kernels' business: the call must only leave the state alone
        return {}

    def q_distance(self):                      # (as a handle: against the model it is compared with; as the model: no distance)
        mine = (self.v, self.c, self.p)
        other = mine if self.peer is None else (self.peer.v, self.peer.c, self.peer.p)
        return distance_record(mine, other)

    def queries(self, rng, whole_domain=True):
        """One op of every query that is valid now, arguments drawn from rng."""
        dx = float(rng.choice(DXS))
        out = [("download", {"field": int(rng.integers(4))}), ("forces_pending", {}), ("last_solve_info", {})]
        if not whole_domain:
            return out
        out += [("residual", {"dx": dx}), ("flow_stats", {"dx": dx}), ("view_scalar", {"what": int(rng.integers(4)), "dx": dx}),
                ("view_texels", {"what": int(rng.integers(4)), "dx": dx}), ("render_rgb565", {"scaling": int(rng.integers(1, 4)), "byteswap": bool(rng.integers(2))}),
                ("distance", {})]
        if self.xy is not None:
            out += [("sample_tracers", {"field": int(rng.integers(4)), "no_slip": bool(rng.integers(2))}), ("tracers", {})]
            if self.trail is not None:
                out.append(("trail", {}))
        if self.mask is not None:                # (the divergence view stays among them: refused, and nothing may move)
            out.append(("solids", {}))
        if self.hist is not None:
            out.append(("history", {}))
        if self.viscous:
            out += [("viscosity", {}), ("bodies", {}), ("loads", {})]
            if self.loads is not None:
                out.append(("loads_history", {}))
        if self.records:
            out += [("friction", {}), ("torque", {}), ("body_pivots", {}), ("mean_info", {})]
            if self.friction is not None:
                out.append(("friction_history", {}))
            if self.torque is not None:
                out.append(("torque_history", {}))
            if self.means is not None:
                planes = mean_rule.planes_of(self.means["what"])
                out.append(("mean_sums", {"plane": int(planes[int(rng.integers(len(planes)))])}))
        if self.opens:
            out += [("openings", {}), ("inflow_profile", {}), ("openings_flux", {})]
        return out


class SlabsModel(ContextModel):
    def queries(self, rng, whole_domain=False):
        return super().queries(rng, False)


# ---- the model of a batch --------------------------------------------------------------------------------------------
class BatchModel:
    def __init__(self, oracle, dim_x, dim_y, batch):
        self.o, self.dim_x, self.dim_y, self.batch = oracle, dim_x, dim_y, batch
        self.m = [ContextModel(oracle, dim_x, dim_y) for _ in range(batch)]
        self.norms = self.iters = None           # the reports: float32[B] / int32[B, 2], None while stale
        self.rec = None                          # the recorder: {"every", "first", "count", "scaling", "byteswap", "steps", "view", "frames"}
        self.env = None                          # the envelope's four fields
        self.peer = None
        self.per_member = False                  # the solids: every member's model holds its mask (one shared, or its own)
        self.hist = None                         # the history: {"every", "first", "count", "capacity", "steps", "records"}
        self.viscous = False                     # (the viscosity's and the loads' queries are among those of queries())
        self.visc = None                         # the viscosity: {"nu": [one per member], "sweeps", "per_member"}; the members hold (nu, sweeps)
        self.bodies, self.labels_per_member = 1, False     # the bodies: every member's model holds its labels (or None)
        self.loads = None                        # the loads recorder: {"every", "first", "count", "capacity", "steps", "records"}
        self.records = False                     # (the friction's, the torque's and the averages' queries are among those of queries())
        self.pivots_per_member = False           # the pivots: every member's model holds its own (or None)
        self.friction = self.torque = None       # the friction and the torque recorder, each as the loads recorder
        self.means = None                        # the averages: {"what", "every", "first", "count", "steps", "samples", "sums": {plane: [count, dim_y, dim_x]}}
        self.opens = False                       # (the openings' queries are among those of queries())
        self.open_per_member = self.inflow_per_member = False      # the openings: every member's model holds its map and its inflow
        self.profile_set = False                 # the profile: every member's model holds its records

    def apply(self, op):
        kind, args = op
        code = self.refuses(kind, args)
        if code:                                 # refused whole: nothing changes
            return refusal(code)
        return getattr(self, ("q_" if kind in QUERIES else "do_") + kind)(**args)

    def openings_set(self):
        return self.m[0].open is not None

    def solids_set(self):
        return self.m[0].mask is not None

    def refuses(self, kind, a):
        """Whether include/sfl.h refuses the call with SFL_ERR_STATE in the state the model is in ("SOLIDS", "HISTORIES")."""
        if self.solids_set():
            if kind in ("step_n_until", "poisson_solve_until", "history_start"):
                return True
            if kind in ("record_view", "view_render_members") and a["what"] == VIEW_DIVERGENCE:
                return True
        if kind == "set_solids" and (self.hist is not None or (self.rec is not None and self.rec["view"] == VIEW_DIVERGENCE)):
            return True
        if kind == "step_n_until" and self.visc is not None:      # "VISCOSITY": refused while one is set, whatever its nu
            return True
        if kind in ("set_bodies", "clear_bodies") and not (self.loads is None and self.friction is None and self.torque is None):
            return True
        if kind in ("loads_history", "friction_history", "torque_history") and getattr(self, kind[:-len("_history")]) is None:
            return True
        # "OPENINGS": what a batch refuses while a map is set, and what refuses the map
        if self.openings_set():
            if kind in ("step_n_until", "poisson_solve_until", "history_start", "set_viscosity"):
                return True
            if kind in ("record_view", "view_render_members") and a["what"] == VIEW_DIVERGENCE:
                return True
        if kind == "set_openings" and (self.hist is not None or (self.rec is not None and self.rec["view"] == VIEW_DIVERGENCE) or self.visc is not None):
            return True
        for recorder in (self.hist, self.loads, self.friction, self.torque):       # (the averages have no capacity: they never refuse)
            if recorder is not None and kind in ("step_n", "step_n_each", "step_n_until"):
                due, free = samples_due(recorder, a["n"])
                if due > free:
                    return True
        if kind == "set_body_pivots" and a["pivot_kind"] is not None and a["bodies"] != self.bodies:
            return ERR_INVALID
        if kind in ("mean_sample", "mean_sums") and self.means is None:
            return True
        if kind == "mean_sums":
            if not self.means["what"] & mean_rule.GROUP_OF[a["plane"]]:
                return ERR_INVALID               # csrc/means.cpp download(): a plane outside `what`, then a range outside the recorded one
            if a["first"] < self.means["first"] or a["first"] + a["count"] > self.means["first"] + self.means["count"]:
                return ERR_INVALID
        if kind == "set_inflow" and not self.openings_set():
            return True
        if kind == "set_inflow_profile" and a["cells"]:
            if not self.openings_set():
                return True
            for k, (cell, u) in enumerate(zip(a["cells"], a["vels"])):      # INFLOW in the map of every member the record applies to
                for m in (self.m if a["members"] is None else [self.m[a["members"][k]]]):
                    if inflow_rule.check_profile([(tuple(cell), u)], m.open) is not None:
                        return ERR_INVALID
        return False

    def close(self):
        pass

    def _stack(self, name):
        return np.stack([m.fields()[name] for m in self.m])

    def snapshot(self):
        out = as_result(**{name: self._stack(name) for name in FIELDS.values()})
        if self.m[0].xy is not None:
            out["tracers"] = np.stack([m.xy for m in self.m])
        return out

    def finite(self):
        return all(m.finite() for m in self.m)

    def _each(self, value):
        return list(value) if isinstance(value, (list, tuple)) else [value] * self.batch

    def _frame(self):
        r = self.rec
        r["steps"] += 1
        if r["steps"] % r["every"]:
            return
        imgs = []
        for m in self.m[r["first"]:r["first"] + r["count"]]:
            dye = m.c if r["view"] is None else view_texels(r["view"], m.v, m.p, 1.0)
            imgs.append(view_rule.render(dye, r["scaling"], r["byteswap"]))
        r["frames"].append(np.stack(imgs))

    def _steps(self, n, dt, dx, iters, omega, stops=None):
        dt, dx, iters, omega = (self._each(x) for x in (dt, dx, iters, omega))
        last, total = np.zeros(self.batch, np.int32), np.zeros(self.batch, np.int32)
        for _ in range(n):
            for k, m in enumerate(self.m):
                last[k], _ = m.step_once(dt[k], dx[k], iters[k], omega[k], None if stops is None else stops[k])
                total[k] += last[k]
            if self.rec is not None:
                self._frame()
            if self.hist is not None:
                h = self.hist
                h["steps"] += 1
                if h["steps"] % h["every"] == 0:
                    members = range(h["first"], h["first"] + h["count"])
                    recs = [self.m[k].history_record(h["steps"], dt[k], dx[k], last[k]) for k in members]
                    h["records"].append({name: np.stack([r[name] for r in recs]) for name in HISTORY_FIELDS})
            if self.loads is not None:
                l = self.loads
                l["steps"] += 1
                if l["steps"] % l["every"] == 0:
                    l["records"].append(self._load_records(l["first"], l["count"]))
            for r, records_of in ((self.friction, self._friction_records), (self.torque, self._torque_records)):
                if r is not None:            # behind a step the order is history, loads, friction, torque, averages
                    r["steps"] += 1
                    if r["steps"] % r["every"] == 0:
                        r["records"].append(records_of(r["first"], r["count"]))
            self.mean_step()
        return dx, np.stack([last, total], axis=1)

    def _load_records(self, first, count):
        return np.stack([m.load_records() for m in self.m[first:first + count]])

    def _friction_records(self, first, count):
        return np.stack([m.friction_records() for m in self.m[first:first + count]])

    def _torque_records(self, first, count):
        return np.stack([m.torque_records() for m in self.m[first:first + count]])

    def mean_step(self):
        m = self.means
        if m is not None and m["every"] >= 1:
            m["steps"] += 1
            if m["steps"] % m["every"] == 0:
                self.mean_add()

    def mean_add(self):
        m = self.means
        mine = self.m[m["first"]:m["first"] + m["count"]]
        mean_rule.add(m["sums"], m["what"], np.stack([x.v for x in mine]), np.stack([x.p for x in mine]), np.stack([x.c for x in mine]))
        m["samples"] += 1

    def _norms(self, dx):                        # (a member with a mask: over its fluid cells)
        self.norms = np.array([m.q_residual(dx[k])["norm"] for k, m in enumerate(self.m)], np.float32)

    # -- writers
    def do_upload(self, field, texture_kind, seed):
        for k, m in enumerate(self.m):
            m.do_upload(field, texture_kind, seed + k)
        if field in (FD, FP):
            self.norms = self.iters = None

    def do_step_n(self, n, dt, dx, iters, omega):
        self._steps(n, dt, dx, iters, omega)
        self.norms = self.iters = None

    def do_step_n_each(self, n, dt, dx, iters, omega):
        dx, _ = self._steps(n, dt, dx, iters, omega)
        self._norms(dx)
        self.iters = None

    def do_step_n_until(self, n, dt, dx, iters, omega, tol, every):
        dx, self.iters = self._steps(n, dt, dx, iters, omega, list(zip(self._each(tol), self._each(every))))
        self._norms(dx)

    def do_poisson_solve(self, dx, iters, omega):
        for m in self.m:
            m.do_poisson_solve(dx, iters, omega)
        self.norms = self.iters = None

    def do_poisson_solve_each(self, dx, iters, omega):
        for k, m in enumerate(self.m):
            m.do_poisson_solve(dx[k], iters[k], omega[k])
        self._norms(dx)
        self.iters = None

    def do_poisson_solve_until(self, dx, iters, omega, tol, every):
        ks = [int(m.do_poisson_solve_until(dx[k], iters[k], omega[k], tol[k], every[k])["iterations"]) for k, m in enumerate(self.m)]
        self._norms(dx)
        self.iters = np.array([[k, k] for k in ks], np.int32)

    def do_queue_forces(self, step, members, cells, vels):
        for m, cell, u in zip(members, cells, vels):
            self.m[m].do_queue_forces(step, [cell], [u])

    def do_forget_forces(self):
        for m in self.m:
            m.do_forget_forces()

    def do_record_start(self, every, first, count, scaling, byteswap):
        self.rec = {"every": every, "first": first, "count": count, "scaling": scaling, "byteswap": byteswap, "steps": 0, "view": None, "frames": []}

    def do_record_view(self, what):
        self.rec["view"] = what

    def do_record_stop(self):
        self.rec = None

    def do_set_tracers(self, xy, follow):
        for m, a in zip(self.m, xy):
            m.do_set_tracers(a, follow)

    def do_envelope(self, first, count):
        self.env = envelope_yardstick(self._stack("colour")[first:first + count])

    def do_set_solids(self, mask_kind, seed, per_member):
        self.per_member = bool(per_member)
        for k, m in enumerate(self.m):
            m.mask = solid_mask(mask_kind, self.dim_x, self.dim_y, seed, k if per_member else None)

    def do_clear_solids(self):
        self.per_member = False
        for m in self.m:
            m.mask = None

    def do_history_start(self, every, capacity, first, count):
        self.hist = {"every": every, "first": first, "count": count, "capacity": capacity, "steps": 0, "records": []}

    def do_history_stop(self):
        self.hist = None

    # "VISCOSITY": one nu for all members or one each; a member with nu == 0 skips the item; set is set, whatever the numbers
    def do_set_viscosity(self, nu, sweeps, per_member):
        self.visc = {"nu": list(nu) if per_member else [nu] * self.batch, "sweeps": sweeps, "per_member": bool(per_member)}
        for m, x in zip(self.m, self.visc["nu"]):
            m.visc = (x, sweeps)

    def do_clear_viscosity(self):
        self.visc = None
        for m in self.m:
            m.visc = None

    def do_set_bodies(self, label_kind, bodies, seed, per_member):
        before = self.bodies
        for k, m in enumerate(self.m):
            m.labels = body_labels(label_kind, self.dim_x, self.dim_y, seed, k if per_member else None)
            m.bodies = 1 if m.labels is None else bodies
        self.bodies, self.labels_per_member = self.m[0].bodies, bool(per_member) and self.m[0].labels is not None
        if self.bodies != before:                # "TORQUE": another number of bodies puts every pivot back to (0, 0)
            self.pivots_per_member = False
            for m in self.m:
                m.pivots = None

    def do_friction_start(self, every, capacity, first, count):
        self.friction = {"every": every, "first": first, "count": count, "capacity": capacity, "steps": 0, "records": []}

    def do_friction_stop(self):
        self.friction = None

    def do_torque_start(self, every, capacity, first, count):
        self.torque = {"every": every, "first": first, "count": count, "capacity": capacity, "steps": 0, "records": []}

    def do_torque_stop(self):
        self.torque = None

    def do_set_body_pivots(self, pivot_kind, bodies, seed, per_member):
        self.pivots_per_member = bool(per_member) and pivot_kind is not None
        for k, m in enumerate(self.m):
            m.pivots = None if pivot_kind is None else body_pivots_of(pivot_kind, bodies, self.dim_x, self.dim_y, seed, k if per_member else None)

    def do_mean_start(self, what, every, first, count):
        self.means = {"what": what, "every": every, "first": first, "count": count, "steps": 0, "samples": 0,
                      "sums": mean_rule.start(what, (count, self.dim_y, self.dim_x))}

    def do_mean_stop(self):
        self.means = None

    def do_mean_sample(self):
        self.mean_add()

    # "OPENINGS": the map and the inflow shared or per member; the profile with `members` None (every record to every member) or per record
    def do_set_openings(self, open_kind, seed, per_member, inflow, inflow_per_member):
        self.open_per_member, self.inflow_per_member, self.profile_set = bool(per_member), bool(inflow_per_member), False
        for k, m in enumerate(self.m):
            m.open = open_map(open_kind, self.dim_x, self.dim_y, seed, k if per_member else None)
            m.inflow, m.profile = tuple(inflow[k] if inflow_per_member else inflow), None

    def do_clear_openings(self):
        self.open_per_member = self.inflow_per_member = self.profile_set = False
        for m in self.m:
            m.do_clear_openings()

    def do_set_inflow(self, inflow, per_member):
        self.inflow_per_member = bool(per_member)
        for k, m in enumerate(self.m):
            m.inflow = tuple(inflow[k] if per_member else inflow)

    def do_set_inflow_profile(self, members, cells, vels):
        self.profile_set = bool(cells)
        for k, m in enumerate(self.m):
            rows = [(tuple(c), tuple(u)) for at, (c, u) in enumerate(zip(cells, vels)) if members is None or members[at] == k]
            m.profile = rows or None

    def do_clear_bodies(self):
        self.do_set_bodies("all one", 1, 0, False)

    def do_loads_start(self, every, capacity, first, count):
        self.loads = {"every": every, "first": first, "count": count, "capacity": capacity, "steps": 0, "records": []}

    def do_loads_stop(self):
        self.loads = None

    # -- queries
    def q_viscosity(self):
        on = self.visc is not None
        return as_result(nu=np.array(self.visc["nu"] if on else [0.0] * self.batch, np.float32), sweeps=self.visc["sweeps"] if on else 0,
                         set=on, per_member=on and self.visc["per_member"])

    def q_bodies(self):
        return as_result(labels=np.stack([m.q_bodies()["labels"] for m in self.m]), bodies=self.bodies, labelled=self.m[0].labels is not None,
                         per_member=self.labels_per_member)

    def q_loads(self, first, count):
        return as_result(records=load_bytes(self._load_records(first, count)))

    def q_loads_history(self):
        l = self.loads
        stacked = np.stack(l["records"]) if l["records"] else np.zeros((0, l["count"], self.bodies), load_rule.DTYPE)
        return as_result(records=load_bytes(stacked), info=np.array([len(l["records"]), l["capacity"], l["steps"], self.bodies], np.int64))

    def _recorded(self, r, dtype):
        stacked = np.stack(r["records"]) if r["records"] else np.zeros((0, r["count"], self.bodies), dtype)
        return as_result(records=raw_bytes(stacked), info=np.array([len(r["records"]), r["capacity"], r["steps"], self.bodies], np.int64))

    def q_friction(self, first, count):
        return as_result(records=raw_bytes(self._friction_records(first, count)))

    def q_friction_history(self):
        return self._recorded(self.friction, friction_rule.DTYPE)

    def q_torque(self, first, count):
        return as_result(records=raw_bytes(self._torque_records(first, count)))

    def q_torque_history(self):
        return self._recorded(self.torque, torque_rule.DTYPE)

    def q_body_pivots(self):
        return as_result(pivot2=np.stack([m.q_body_pivots()["pivot2"] for m in self.m]))

    def q_mean_info(self):
        m = self.means
        return as_result(info=np.array([0, 0, 0, 0] if m is None else [m["what"], m["every"], m["samples"], m["steps"]], np.int64))

    def q_mean_sums(self, plane, first, count):
        at = first - self.means["first"]
        return as_result(plane=self.means["sums"][plane][at:at + count].copy())

    def q_openings(self):
        live = np.sum([live_cells(m.open, m.mask) for m in self.m], axis=0) if self.openings_set() else (0, 0)
        return as_result(map=np.stack([m.q_openings()["map"] for m in self.m]), inflow=np.array([m.inflow for m in self.m], np.float32), set=self.openings_set(),
                         per_member=self.open_per_member, inflow_per_member=self.inflow_per_member, live=np.array(live, np.int64))

    def q_inflow_profile(self, member):
        cells, vel = profile_arrays(self.m[member].profile)
        held = sum(len(profile_arrays(m.profile)[0]) for m in self.m)
        return as_result(cells=cells, vel=vel, set=self.profile_set, held=held)

    def q_openings_flux(self, first, count):
        return as_result(records=np.stack([m.q_openings_flux()["record"] for m in self.m[first:first + count]]))

    def q_download(self, field):
        return as_result(field=self._stack(FIELDS[field]))

    def q_flow_stats(self, dx):
        recs = [m.q_flow_stats(dx) for m in self.m]
        return {k: np.stack([r[k] for r in recs]) for k in recs[0]}

    def q_distance(self, ref_member):
        ref = self if self.peer is None else self.peer
        r = ref.m[ref_member]
        recs = [distance_record((m.v, m.c, m.p), (r.v, r.c, r.p)) for m in self.m]
        return {k: np.stack([x[k] for x in recs]) for k in recs[0]}

    def q_envelope_field(self, which):
        return as_result(field=self.env[which])

    def q_residual(self):
        return as_result(norms=self.norms)

    def q_iterations(self):
        return as_result(iterations=self.iters)

    def q_render_members(self, scaling, byteswap):
        return as_result(images=np.stack([view_rule.render(m.c, scaling, byteswap) for m in self.m]))

    def q_view_render_members(self, what, scaling):
        return as_result(images=np.stack([view_rule.render(view_texels(what, m.v, m.p, 1.0), scaling, True) for m in self.m]))

    def q_frames(self):
        r = self.rec
        shape = (r["count"], r["scaling"] * (self.dim_x - 1), r["scaling"] * (self.dim_y - 1))
        return as_result(frames=np.stack(r["frames"]) if r["frames"] else np.zeros((0,) + shape, np.uint16))

    def q_forces_pending(self):
        steps = [s for m in self.m for s in m.timeline]
        return as_result(records=sum(len(r) for m in self.m for r in m.timeline.values()), last_step=max(steps, default=-1))

    def q_tracers(self):
        return as_result(xy=np.stack([m.xy for m in self.m]))

    def q_solids(self):
        return as_result(mask=np.stack([m.q_solids()["mask"] for m in self.m]), set=self.solids_set(), per_member=self.per_member)

    def q_history(self):
        return history_result(self.hist, (self.hist["count"],))

    def queries(self, rng):
        out = [("download", {"field": int(rng.integers(4))}), ("flow_stats", {"dx": float(rng.choice(DXS))}),
               ("distance", {"ref_member": int(rng.integers(self.batch))}), ("forces_pending", {}),
               ("render_members", {"scaling": int(rng.integers(1, 3)), "byteswap": bool(rng.integers(2))}),
               ("view_render_members", {"what": int(rng.integers(4)), "scaling": int(rng.integers(1, 3))})]
        if self.env is not None: out.append(("envelope_field", {"which": int(rng.integers(4))}))
        if self.norms is not None: out.append(("residual", {}))
        if self.iters is not None: out.append(("iterations", {}))
        if self.rec is not None: out.append(("frames", {}))
        if self.m[0].xy is not None: out.append(("tracers", {}))
        if self.solids_set(): out.append(("solids", {}))
        if self.hist is not None: out.append(("history", {}))
        if self.viscous:
            first = int(rng.integers(self.batch))
            out += [("viscosity", {}), ("bodies", {}), ("loads", {"first": first, "count": int(rng.integers(1, self.batch - first + 1))})]
            if self.loads is not None: out.append(("loads_history", {}))
        if self.records:
            first = int(rng.integers(self.batch))
            some = {"first": first, "count": int(rng.integers(1, self.batch - first + 1))}
            out += [("friction", dict(some)), ("torque", dict(some)), ("body_pivots", {}), ("mean_info", {})]
            if self.friction is not None: out.append(("friction_history", {}))
            if self.torque is not None: out.append(("torque_history", {}))
            if self.means is not None:
                planes = mean_rule.planes_of(self.means["what"])
                out.append(("mean_sums", {"plane": int(planes[int(rng.integers(len(planes)))]), "first": self.means["first"], "count": self.means["count"]}))
        if self.opens:
            first = int(rng.integers(self.batch))
            out += [("openings", {}), ("inflow_profile", {"member": int(rng.integers(self.batch))}),
                    ("openings_flux", {"first": first, "count": int(rng.integers(1, self.batch - first + 1))})]
        return out


# ---- the library behind the same interface ---------------------------------------------------------------------------
def _record(rec, names):
    return {k: np.asarray(rec[k]) for k in names}


STATS_NAMES = ("max_abs_vx", "max_abs_vy", "max_abs_div", "dye_sum")
DIST_NAMES = ("max_abs_dvx", "max_abs_dvy", "max_abs_dp", "velocity_cells_differ", "dye_cells_differ", "pressure_cells_differ",
              "max_abs_ddye", "sum_abs_ddye")


class LibraryContext:
    """A whole-domain Solver, or a linked group of `nranks` slabs on one device: operators go to slab 0 (collective over the
    group), field I/O to every slab's own rows."""

    def __init__(self, sfl, dim_x, dim_y, nranks=1, options=()):
        self.sfl, self.dim_x, self.dim_y, self.peer, self.twin = sfl, dim_x, dim_y, None, None
        self.slabs = [sfl.Solver(dim_x, dim_y, 0, r, nranks) for r in range(nranks)]
        if nranks > 1:
            sfl.Solver.link_group(self.slabs)
        self.s = self.slabs[0]
        for name, value in options:
            self.g_set_option(name, value)

    def close(self):
        for s in self.slabs + ([self.twin] if self.twin else []):
            s.close()

    def apply(self, op):
        kind, args = op
        try:
            return getattr(self, "g_" + kind)(**args)
        except self.sfl.capi.SflError as e:      # a refusal is a result like any other: the runner compares the state behind it
            return as_result(refused=np.int32(e.code))

    def _cat(self, field):
        return np.concatenate([s.download(field) for s in self.slabs], axis=0)

    def snapshot(self):
        out = as_result(**{name: self._cat(f) for f, name in FIELDS.items()})
        if len(self.slabs) == 1 and self.s.tracer_count():
            out["tracers"] = self.s.tracers()
        return out

    def _view(self, what, dx):
        lo, hi = VIEW_RANGE[what]
        return self.sfl.View(what, lo, hi, PALETTE, dx=dx, nan_colour=NAN_COLOUR)

    def g_upload(self, field, texture_kind, seed):
        a = texture(texture_kind, field, self.dim_x, self.dim_y, seed)
        for s in self.slabs:
            s.upload(field, a[s.row_begin:s.row_end])

    def g_advect_velocity(self, dt, no_slip): self.s.advect_velocity(dt, no_slip)
    def g_advect_color(self, dt, no_slip): self.s.advect_color(dt, no_slip)
    def g_calculate_divergence(self, dx): self.s.calculate_divergence(dx)
    def g_poisson_solve(self, dx, iters, omega): self.s.poisson_solve(dx, iters, omega)
    def g_poisson_continue(self, dx, iters, omega): self.s.poisson_continue(dx, iters, omega)
    def g_subtract_gradient(self, dx): self.s.subtract_gradient(dx)
    def g_step(self, dt, dx, iters, omega): self.s.step(dt, dx, iters, omega)
    def g_step_n(self, n, dt, dx, iters, omega): self.s.step_n(n, dt, dx, iters, omega)
    def g_forget_forces(self): self.s.forget_forces()
    def g_set_tracers(self, xy, follow): self.s.set_tracers(np.array(xy, np.float32), follow)
    def g_advance_tracers(self, dt): self.s.advance_tracers(dt)
    def g_trail_start(self, every): self.s.trail_start(every, CAPACITY)
    def g_trail_stop(self): self.s.trail_stop()
    def g_set_option(self, name, value): self.s.set_option(getattr(self.sfl.capi, name), value)
    def g_set_solids(self, mask_kind, seed): self.s.set_solids(solid_mask(mask_kind, self.dim_x, self.dim_y, seed))
    def g_clear_solids(self): self.s.set_solids(None)
    def g_history_start(self, every, capacity): self.s.history_start(every, capacity)
    def g_history_stop(self): self.s.history_stop()
    def g_set_viscosity(self, nu, sweeps): self.s.set_viscosity(nu, sweeps)
    def g_clear_viscosity(self): self.s.set_viscosity(0.0, 0)
    def g_diffuse_velocity(self, nu, dt, dx, sweeps): self.s.diffuse_velocity(nu, dt, dx, sweeps)
    def g_clear_bodies(self): self.s.set_bodies(None)
    def g_loads_start(self, every, capacity): self.s.loads_start(every, capacity)
    def g_loads_stop(self): self.s.loads_stop()

    def g_set_bodies(self, label_kind, bodies, seed):
        self.s.set_bodies(body_labels(label_kind, self.dim_x, self.dim_y, seed), bodies)

    def g_friction_start(self, every, capacity): self.s.friction_start(every, capacity)
    def g_friction_stop(self): self.s.friction_stop()
    def g_torque_start(self, every, capacity): self.s.torque_start(every, capacity)
    def g_torque_stop(self): self.s.torque_stop()
    def g_mean_start(self, what, every): self.s.mean_start(what, every)
    def g_mean_stop(self): self.s.mean_stop()
    def g_mean_sample(self): self.s.mean_sample()
    def g_clear_openings(self): self.s.set_openings(None)
    def g_set_inflow(self, inflow): self.s.set_inflow(inflow)
    def g_set_inflow_profile(self, cells, vels): self.s.set_inflow_profile(cells, vels)

    def g_set_body_pivots(self, pivot_kind, bodies, seed):
        """(straight to the C call: the package's method takes `bodies` from the handle, and the op may name another)"""
        if pivot_kind is None:
            return self.s.set_body_pivots(None)
        p2 = np.ascontiguousarray(body_pivots_of(pivot_kind, bodies, self.dim_x, self.dim_y, seed), np.int32)
        self.sfl.capi.check(self.s._lib.sfl_set_body_pivots(self.s._h, p2.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), bodies))

    def g_set_openings(self, open_kind, seed, inflow):
        self.s.set_openings(open_map(open_kind, self.dim_x, self.dim_y, seed), inflow)

    def g_friction(self): return as_result(records=raw_bytes(self.s.friction()))
    def g_torque(self): return as_result(records=raw_bytes(self.s.torque()))
    def g_body_pivots(self): return as_result(pivot2=np.round(self.s.body_pivots() * 2).astype(np.int32))
    def g_mean_info(self): return as_result(info=np.array(self.s.mean_info(), np.int64))
    def g_mean_sums(self, plane): return as_result(plane=self.s.mean_sums(plane))
    def g_openings_flux(self): return as_result(record=raw_bytes(self.s.openings_flux()))

    def g_friction_history(self):
        return as_result(records=raw_bytes(self.s.friction_history()), info=np.array(self.s.friction_info(), np.int64))

    def g_torque_history(self):
        return as_result(records=raw_bytes(self.s.torque_history()), info=np.array(self.s.torque_info(), np.int64))

    def g_openings(self):
        (on, live_in, live_out), (held, inflow) = self.s.openings_info(), self.s.openings()
        return as_result(map=held, inflow=inflow, set=on, live=np.array([live_in, live_out], np.int64))

    def g_inflow_profile(self):
        cells, vel = self.s.inflow_profile()
        return as_result(cells=cells, vel=vel)

    def g_viscosity(self):
        nu, sweeps = self.s.viscosity()
        return as_result(nu=np.float32(nu), sweeps=sweeps)

    def g_bodies(self):
        bodies, labelled = self.s.bodies_info()
        return as_result(labels=self.s.bodies(), bodies=bodies, labelled=labelled)

    def g_loads(self): return as_result(records=load_bytes(self.s.loads()))

    def g_loads_history(self):
        return as_result(records=load_bytes(self.s.loads_history()), info=np.array(self.s.loads_info(), np.int64))

    def g_poisson_solve_until(self, dx, iters, omega, tol, every):
        k, u = self.s.poisson_solve_until(dx, iters, omega, tol=tol, every=every)
        return as_result(iterations=np.int32(k), norm=np.float32(u))

    def g_queue_forces(self, step, cells, vels):
        if step == 0:
            self.s.queue_forces(cells, vels)              # the call from before there was a timeline
        else:
            self.s.queue_forces(cells, vels, step=step)

    def g_queue_drags(self, step, drags):
        self.s.queue_drags(drags, step=step)

    def g_download(self, field): return as_result(field=self._cat(field))
    def g_residual(self, dx): return as_result(norm=self.s.residual(dx))
    def g_flow_stats(self, dx): return _record(self.s.flow_stats(dx), STATS_NAMES)
    def g_view_scalar(self, what, dx): return as_result(scalar=self.s.view_scalar(what, dx))
    def g_view_texels(self, what, dx): return as_result(texels=self.s.view_texels(self._view(what, dx)))
    def g_render_rgb565(self, scaling, byteswap): return as_result(image=self.s.render_rgb565(scaling, byteswap))
    def g_sample_tracers(self, field, no_slip): return as_result(samples=self.s.sample_tracers(field, no_slip))
    def g_tracers(self): return as_result(xy=self.s.tracers())
    def g_trail(self): return as_result(slots=self.s.trail())

    def g_solids(self):
        on, cells = self.s.solids_info()
        return as_result(mask=self.s.solids(), set=on, solid_cells=cells)

    def g_history(self):
        rec = self.s.history()
        return dict({name: np.ascontiguousarray(rec[name]) for name in HISTORY_FIELDS}, info=np.array(self.s.history_info(), np.int64))

    def g_forces_pending(self):
        records, last = self.s.forces_pending()
        return as_result(records=records, last_step=last)

    def g_last_solve_info(self):
        self.s.last_solve_info()
        return {}

    def g_distance(self):
        """The distance to a twin that holds the model's fields: all zero when the handle holds them too."""
        if self.twin is None:
            self.twin = self.sfl.Solver(self.dim_x, self.dim_y)
        for f, name in FIELDS.items():
            self.twin.upload(f, self.peer.fields()[name])
        return _record(self.s.distance(self.twin), DIST_NAMES)


class LibraryBatch:
    def __init__(self, sfl, dim_x, dim_y, batch, large=False):
        self.sfl, self.dim_x, self.dim_y, self.batch, self.peer = sfl, dim_x, dim_y, batch, None
        self.b = sfl.BatchSolver(dim_x, dim_y, batch, large=large)

    def close(self):
        self.b.close()

    def apply(self, op):
        kind, args = op
        try:
            return getattr(self, "g_" + kind)(**args)
        except self.sfl.capi.SflError as e:      # a refusal is a result like any other: the runner compares the state behind it
            return as_result(refused=np.int32(e.code))

    def snapshot(self):
        out = as_result(**{name: self.b.download(f) for f, name in FIELDS.items()})
        if self.b.tracer_count():
            out["tracers"] = self.b.tracers()
        return out

    def _view(self, what):
        lo, hi = VIEW_RANGE[what]
        return self.sfl.View(what, lo, hi, PALETTE, dx=1.0, nan_colour=NAN_COLOUR)

    def g_upload(self, field, texture_kind, seed):
        self.b.upload(field, np.stack([texture(texture_kind, field, self.dim_x, self.dim_y, seed + k) for k in range(self.batch)]))

    def g_step_n(self, n, dt, dx, iters, omega): self.b.step_n(n, dt, dx, iters, omega)
    def g_step_n_each(self, n, dt, dx, iters, omega): self.b.step_n_each(n, dt, dx, iters, omega)
    def g_step_n_until(self, n, dt, dx, iters, omega, tol, every): self.b.step_n_until(n, dt, dx, iters, omega, tol=tol, every=every)
    def g_poisson_solve(self, dx, iters, omega): self.b.poisson_solve(dx, iters, omega)
    def g_poisson_solve_each(self, dx, iters, omega): self.b.poisson_solve_each(dx, iters, omega)
    def g_poisson_solve_until(self, dx, iters, omega, tol, every): self.b.poisson_solve_until(dx, iters, omega, tol=tol, every=every)
    def g_forget_forces(self): self.b.forget_forces()
    def g_record_start(self, every, first, count, scaling, byteswap): self.b.record_start(every, first, count, scaling, byteswap, CAPACITY)
    def g_record_view(self, what): self.b.record_view(None if what is None else self._view(what))
    def g_record_stop(self): self.b.record_stop()
    def g_set_tracers(self, xy, follow): self.b.set_tracers(np.array(xy, np.float32), follow)
    def g_envelope(self, first, count): self.b.envelope(first, count)
    def g_clear_solids(self): self.b.set_solids(None)
    def g_history_start(self, every, capacity, first, count): self.b.history_start(every, capacity, first, count)
    def g_history_stop(self): self.b.history_stop()
    def g_set_viscosity(self, nu, sweeps, per_member): self.b.set_viscosity(np.array(nu, np.float32) if per_member else nu, sweeps)
    def g_clear_viscosity(self): self.b.set_viscosity(None, 0)
    def g_clear_bodies(self): self.b.set_bodies(None)
    def g_loads_start(self, every, capacity, first, count): self.b.loads_start(every, capacity, first, count)
    def g_loads_stop(self): self.b.loads_stop()

    def g_set_bodies(self, label_kind, bodies, seed, per_member):
        if label_kind == "all one":
            return self.b.set_bodies(None)
        labels = [body_labels(label_kind, self.dim_x, self.dim_y, seed, k) for k in (range(self.batch) if per_member else [None])]
        self.b.set_bodies(np.stack(labels) if per_member else labels[0], bodies)

    def g_friction_start(self, every, capacity, first, count): self.b.friction_start(every, capacity, first, count)
    def g_friction_stop(self): self.b.friction_stop()
    def g_torque_start(self, every, capacity, first, count): self.b.torque_start(every, capacity, first, count)
    def g_torque_stop(self): self.b.torque_stop()
    def g_mean_start(self, what, every, first, count): self.b.mean_start(what, every, first, count)
    def g_mean_stop(self): self.b.mean_stop()
    def g_mean_sample(self): self.b.mean_sample()
    def g_clear_openings(self): self.b.set_openings(None)
    def g_set_inflow(self, inflow, per_member): self.b.set_inflow(np.array(inflow, np.float32))
    def g_set_inflow_profile(self, members, cells, vels): self.b.set_inflow_profile(cells, vels, members)

    def g_set_body_pivots(self, pivot_kind, bodies, seed, per_member):
        """(straight to the C call: the package's method takes `bodies` from the handle, and the op may name another)"""
        if pivot_kind is None:
            return self.b.set_body_pivots(None)
        members = range(self.batch) if per_member else [None]
        p2 = np.ascontiguousarray(np.stack([body_pivots_of(pivot_kind, bodies, self.dim_x, self.dim_y, seed, k) for k in members]), np.int32)
        self.sfl.capi.check(self.b._lib.sfl_batch_set_body_pivots(self.b._h, p2.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), int(bool(per_member)), bodies))

    def g_set_openings(self, open_kind, seed, per_member, inflow, inflow_per_member):
        maps = [open_map(open_kind, self.dim_x, self.dim_y, seed, k) for k in (range(self.batch) if per_member else [None])]
        self.b.set_openings(np.stack(maps) if per_member else maps[0], np.array(inflow, np.float32))

    def g_friction(self, first, count): return as_result(records=raw_bytes(self.b.friction(first, count)))
    def g_torque(self, first, count): return as_result(records=raw_bytes(self.b.torque(first, count)))
    def g_body_pivots(self): return as_result(pivot2=np.round(self.b.body_pivots() * 2).astype(np.int32))
    def g_mean_info(self): return as_result(info=np.array(self.b.mean_info(), np.int64))
    def g_mean_sums(self, plane, first, count): return as_result(plane=self.b.mean_sums(plane, first, count))
    def g_openings_flux(self, first, count): return as_result(records=raw_bytes(self.b.openings_flux(first, count)))

    def g_friction_history(self):
        return as_result(records=raw_bytes(self.b.friction_history()), info=np.array(self.b.friction_info(), np.int64))

    def g_torque_history(self):
        return as_result(records=raw_bytes(self.b.torque_history()), info=np.array(self.b.torque_info(), np.int64))

    def g_openings(self):
        (on, per_member, inflow_per_member, live_in, live_out), (held, inflow) = self.b.openings_info(), self.b.openings()
        return as_result(map=held, inflow=inflow, set=on, per_member=per_member, inflow_per_member=inflow_per_member, live=np.array([live_in, live_out], np.int64))

    def g_inflow_profile(self, member):
        (on, held), (cells, vel) = self.b.inflow_profile_info(), self.b.inflow_profile(member)
        return as_result(cells=cells, vel=vel, set=on, held=held)

    def g_viscosity(self):
        nu, sweeps = self.b.viscosity()
        on, per_member = ctypes.c_int(0), ctypes.c_int(0)
        self.sfl.capi.check(self.b._lib.sfl_batch_viscosity_info(self.b._h, ctypes.byref(on), ctypes.byref(per_member), None))
        return as_result(nu=nu, sweeps=sweeps, set=bool(on.value), per_member=bool(per_member.value))

    def g_bodies(self):
        bodies, labelled, per_member = self.b.bodies_info()
        return as_result(labels=self.b.bodies(), bodies=bodies, labelled=labelled, per_member=per_member)

    def g_loads(self, first, count): return as_result(records=load_bytes(self.b.loads(first, count)))

    def g_loads_history(self):
        return as_result(records=load_bytes(self.b.loads_history()), info=np.array(self.b.loads_info(), np.int64))

    def g_set_solids(self, mask_kind, seed, per_member):
        members = range(self.batch) if per_member else [None]
        masks = np.stack([solid_mask(mask_kind, self.dim_x, self.dim_y, seed, k) for k in members])
        self.b.set_solids(masks if per_member else masks[0])

    def g_queue_forces(self, step, members, cells, vels):
        if step == 0:
            self.b.queue_forces(members, cells, vels)
        else:
            self.b.queue_forces(members, cells, vels, step=step)

    def g_download(self, field): return as_result(field=self.b.download(field))
    def g_flow_stats(self, dx): return _record(self.b.flow_stats(dx), STATS_NAMES)
    def g_distance(self, ref_member): return _record(self.b.distance(ref_member=ref_member), DIST_NAMES)
    def g_envelope_field(self, which): return as_result(field=self.b.envelope_field(which))
    def g_residual(self): return as_result(norms=self.b.residual())
    def g_iterations(self): return as_result(iterations=self.b.iterations())
    def g_render_members(self, scaling, byteswap): return as_result(images=self.b.render_members(scaling=scaling, byteswap=byteswap))
    def g_view_render_members(self, what, scaling): return as_result(images=self.b.view_render_members(self._view(what), scaling=scaling))
    def g_frames(self): return as_result(frames=self.b.frames())
    def g_tracers(self): return as_result(xy=self.b.tracers())

    def g_solids(self):
        on, per_member = self.b.solids_info()
        return as_result(mask=self.b.solids(), set=on, per_member=per_member)

    def g_history(self):
        rec = self.b.history()
        return dict({name: np.ascontiguousarray(rec[name]) for name in HISTORY_FIELDS}, info=np.array(self.b.history_info(), np.int64))

    def g_forces_pending(self):
        records, last = self.b.forces_pending()
        return as_result(records=records, last_step=last)


# ---- subjects --------------------------------------------------------------------------------------------------------
class Subject:
    """What a set of sequences runs on: `cases` = [(dim_x, dim_y, seed)], one sequence each."""

    def __init__(self, name, kind, cases, options=(), nranks=1, batch=0, large=False, still_solves=False, length=30, solids=False, viscous=False,
                 records=False, opens=False):
        self.name, self.kind, self.cases, self.options, self.nranks, self.batch, self.large = name, kind, cases, tuple(options), nranks, batch, large
        self.still_solves, self.length = still_solves, length   # still_solves: steps on a lattice velocity run iters = 0 (it stays on the lattice)
        self.solids = solids                                    # the solids' and the histories' calls are in the vocabulary
        self.viscous = viscous                                  # ... and the viscosity's and the loads' (on top of the solids')
        self.records = records                                  # ... and the friction's, the torque's and the averages' (on top of the viscous deck)
        self.opens = opens                                      # the openings', the profiles' and the flux's (on top of the solids' deck)

    def model(self, oracle, case):
        dim_x, dim_y, _ = case
        if self.kind == "batch":
            model = BatchModel(oracle, dim_x, dim_y, self.batch)
        else:
            model = (ContextModel if self.kind == "context" else SlabsModel)(oracle, dim_x, dim_y)
        model.viscous, model.records, model.opens = self.viscous, self.records, self.opens
        return model

    def library(self, sfl, case):
        dim_x, dim_y, _ = case
        if self.kind == "batch":
            return LibraryBatch(sfl, dim_x, dim_y, self.batch, self.large)
        return LibraryContext(sfl, dim_x, dim_y, self.nranks, self.options)

    def kinds(self):
        own = {"context": CONTEXT_WRITERS + CONTEXT_QUERIES, "slabs": SLAB_WRITERS + SLAB_QUERIES, "batch": BATCH_WRITERS + BATCH_QUERIES}[self.kind]
        if not self.solids:
            return own
        own = tuple(k for k in own if k not in SOLID_LEFT_OUT) + SOLID_WRITERS + SOLID_QUERIES
        if self.opens:
            return own + OPEN_WRITERS + OPEN_QUERIES
        if not self.viscous:
            return own
        own += (VISCOUS_WRITERS if self.kind == "context" else BATCH_VISCOUS_WRITERS) + VISCOUS_QUERIES
        return own + RECORD_WRITERS + RECORD_QUERIES if self.records else own

    def option_values(self):
        return {"context": OPTION_VALUES, "slabs": SLAB_OPTION_VALUES, "batch": {}}[self.kind]


VISCOUS_LENGTH = {"context": 50, "batch": 48}     # ops of a sequence of the viscous subjects: the shortest the deck fits in
RECORD_LENGTH = {"context": 69, "batch": 76}      # ... of the subjects with friction, torque and averages, found in the same way
OPEN_LENGTH = {"context": 60, "batch": 67}       # ... and of the subjects with openings


def _cases(dim_x, dim_y, seeds, base):
    return [(dim_x, dim_y, base + k) for k in range(seeds)]


SUBJECTS = [
    Subject("general", "context", _cases(130, 70, 4, 100), options=[("OPT_SMALL_GRID", 0)]),
    Subject("seams", "context", _cases(300, 141, 4, 200), still_solves=True),
    Subject("one-workgroup", "context", _cases(61, 81, 4, 300) + _cases(2, 2, 2, 350)),
    Subject("slabs", "slabs", _cases(200, 131, 4, 400), nranks=3),
    Subject("small-batch", "batch", _cases(61, 81, 4, 500) + _cases(7, 9, 2, 550), batch=3),
    Subject("large-batch", "batch", _cases(96, 96, 4, 600), batch=2, large=True),
    # solids and histories: a mask set, replaced and cleared on a handle that goes on stepping.  130 x 70 is 3 x 3 ragged tiles of
    # the masked solve and, cleared, the general kernels and the step seams; 61 x 81 three tiles in a column and, cleared, the
    # one-launch step of a small grid; the batch's members 61 x 81 and 7 x 9 (a large batch refuses solids)
    Subject("solid-context", "context", _cases(130, 70, 3, 700) + _cases(61, 81, 2, 750), length=36, solids=True),
    Subject("solid-batch", "batch", _cases(61, 81, 3, 800) + _cases(7, 9, 2, 850), batch=3, length=36, solids=True),
    # viscosity and loads, on top of the solids' vocabulary: a viscosity set, cleared and set again with masks coming and going,
    # the diffusion as an operator of one, two and three launches, labels, and a loads recorder counted across calls.  130 x 70 is
    # 3 x 3 ragged diffusion tiles (64 x 32: the last column two cells wide, the last row six deep) and, cleared, the general
    # kernels and the step seams; 61 x 81 one tile column of three rows and, cleared, the one-launch step of a small grid; 7 x 9 a
    # batch member smaller than a wavefront (slabs and large batches refuse viscosity)
    Subject("viscous-context", "context", _cases(130, 70, 3, 900) + _cases(61, 81, 2, 950), length=VISCOUS_LENGTH["context"], solids=True, viscous=True),
    Subject("viscous-batch", "batch", _cases(61, 81, 3, 1000) + _cases(7, 9, 2, 1050), batch=3, length=VISCOUS_LENGTH["batch"], solids=True, viscous=True),
    # friction, torque and averages, on top of the viscous vocabulary and at its shapes: three more recorders with buffers, step
    # counts and admission of their own beside the loads' and a history, pivots that follow the number of bodies, and averages
    # that cut a batch's one-launch replay and a context's fused seams while every >= 1 and give them back when stopped
    Subject("record-context", "context", _cases(130, 70, 3, 1100) + _cases(61, 81, 2, 1150), length=RECORD_LENGTH["context"], solids=True, viscous=True, records=True),
    Subject("record-batch", "batch", _cases(61, 81, 3, 1200) + _cases(7, 9, 2, 1250), batch=3, length=RECORD_LENGTH["batch"], solids=True, viscous=True, records=True),
    # openings, inflow profiles and the flux, on top of the solids' vocabulary and at its shapes (openings and a viscosity refuse
    # each other): 130 x 70 is 3 x 3 ragged tiles of the masked solve, whose rim cells lie in the two-cell-wide last column and the
    # six-deep last row; 61 x 81 one tile column; 7 x 9 a member smaller than a wavefront.  A map before and behind a mask, masks
    # replaced and cleared behind a map, inflow cells that go solid and come back, profiles replaced, dropped and kept
    Subject("open-context", "context", _cases(130, 70, 3, 1300) + _cases(61, 81, 2, 1350), length=OPEN_LENGTH["context"], solids=True, opens=True),
    Subject("open-batch", "batch", _cases(61, 81, 3, 1400) + _cases(7, 9, 2, 1450), batch=3, length=OPEN_LENGTH["batch"], solids=True, opens=True),
]


# ---- the generator ---------------------------------------------------------------------------------------------------
class Gate:
    """What the generator and the census follow of a handle with solids and histories, from the op list alone: the masks, the
    history's counts, the recorder's view, the trail, a batch's reports, the viscosity set, the label kind, the loads recorder's
    counts and how many two-launch diffusions the handle has made -- enough to say which calls include/sfl.h refuses
    (the models decide the same from their own state; tests/test_sequences.py holds the two against each other)."""

    def __init__(self, batch, dim_x, dim_y):
        self.batch, self.dim_x, self.dim_y = batch, dim_x, dim_y
        self.masks, self.hist = None, None                    # [mask] or one per member; [every, capacity, steps]
        self.rec, self.view, self.trail = False, None, False
        self.norms = self.iters = False
        self.visc = None                                      # {"nu": [one per member, or one], "sweeps", "per_member"} while one is set
        self.labels, self.loads = None, None                  # the label kind while labels are set; [every, capacity, steps]
        self.two_launches = 0                                 # two-launch diffusions made so far: the third buffer has held a velocity
        self.bodies, self.pivots = 1, None                    # the number of bodies; the set_body_pivots arguments while pivots are set
        self.friction, self.torque = None, None               # [every, capacity, steps], as the loads recorder
        self.ranges = {}                                      # a batch: recorder -> (first, count)
        self.means = None                                     # {"what", "every", "first", "count", "steps", "samples"}
        self.open, self.inflow, self.profile = None, None, None   # [map] or one per member; [(u, v)] likewise; the set_inflow_profile arguments

    def mixed(self):
        return self.masks is not None and any(mixed(m) for m in self.masks)

    def maps_of(self, members):
        """The map of every member named (a context: [0])."""
        return [self.open[m if len(self.open) > 1 else 0] for m in members]

    def mask_of(self, member):
        return None if self.masks is None else self.masks[member if len(self.masks) > 1 else 0]

    def live(self):
        """(live inflow cells, live outflow cells) over all members, as `openings` reports them; (0, 0) without a map."""
        if self.open is None:
            return 0, 0
        each = [live_cells(self.maps_of([m])[0], self.mask_of(m)) for m in range(max(self.batch, 1))]
        return tuple(int(x) for x in np.sum(each, axis=0))

    def profile_fits(self, a):
        """Whether every record of a set_inflow_profile names an INFLOW cell of the map of every member it applies to."""
        for k, cell in enumerate(a["cells"]):
            members = range(max(self.batch, 1)) if a.get("members") is None else [a["members"][k]]
            if any(inflow_rule.check_profile([(tuple(cell), None)], m) is not None for m in self.maps_of(members)):
                return False
        return True

    def code(self, kind, a):
        """The code of the refusal remedy() announces: SFL_ERR_INVALID for the three the library checks behind the state."""
        if kind == "set_body_pivots" or (kind == "mean_sums" and self.means is not None) or (kind == "set_inflow_profile" and self.open is not None):
            return ERR_INVALID
        return ERR_STATE

    def remedy(self, kind, a):
        """None when the header takes the call, else the kind of a call to make in its place: the one that ends what it is
        refused for, or (the _until calls under a mask, step_n_until under a viscosity) its sibling that honours them."""
        on = self.masks is not None
        if self.batch:
            if on and kind in ("step_n_until", "poisson_solve_until"): return kind.replace("until", "each")
            if on and kind == "history_start": return "clear_solids"
            if on and kind in ("record_view", "view_render_members") and a["what"] == VIEW_DIVERGENCE: return "clear_solids"
            if kind == "set_solids" and self.hist is not None: return "history_stop"
            if kind == "set_solids" and self.rec and self.view == VIEW_DIVERGENCE: return "record_stop"
            if kind == "step_n_until" and self.visc is not None: return "step_n_each"      # "VISCOSITY": refused while one is set
        elif on and kind in ("view_scalar", "view_texels") and a["what"] == VIEW_DIVERGENCE:
            return "clear_solids"
        if self.open is not None:                   # "OPENINGS": what is refused while a map is set ...
            if self.batch:
                if kind in ("step_n_until", "poisson_solve_until"): return kind.replace("until", "each")
                if kind in ("history_start", "set_viscosity"): return "clear_openings"
                if kind in ("record_view", "view_render_members") and a["what"] == VIEW_DIVERGENCE: return "clear_openings"
            else:
                if kind in ("view_scalar", "view_texels") and a["what"] == VIEW_DIVERGENCE: return "clear_openings"
                if kind == "set_viscosity" and not (a["nu"] == 0 or a["sweeps"] == 0): return "clear_openings"
            if kind == "set_inflow_profile" and a["cells"] and not self.profile_fits(a): return "inflow_profile"    # (SFL_ERR_INVALID; planted only)
        else:                                       # ... and what is refused without one
            if kind == "set_inflow" or (kind == "set_inflow_profile" and a["cells"]): return "set_openings"
        if kind == "set_openings":                  # ... and what refuses the map
            if self.batch and self.hist is not None: return "history_stop"
            if self.batch and self.rec and self.view == VIEW_DIVERGENCE: return "record_stop"
            if self.visc is not None: return "clear_viscosity"
        if kind in ("set_bodies", "clear_bodies") and self.loads is not None: return "loads_stop"   # "LOADS": the samples' layout
        if kind in ("set_bodies", "clear_bodies") and self.friction is not None: return "friction_stop"
        if kind in ("set_bodies", "clear_bodies") and self.torque is not None: return "torque_stop"
        for name, stop in (("hist", "history_stop"), ("loads", "loads_stop"), ("friction", "friction_stop"), ("torque", "torque_stop")):
            recorder = getattr(self, name)          # the admission checks, in the library's order
            if recorder is not None and kind in STEPS:
                every, capacity, steps = recorder
                if (steps + a.get("n", 1)) // every - steps // every > capacity - steps // every: return stop
        if kind == "set_body_pivots" and a["pivot_kind"] is not None and a["bodies"] != self.bodies: return "body_pivots"    # (SFL_ERR_INVALID; planted only)
        if kind == "mean_sums" and self.means is not None:                                               # (SFL_ERR_INVALID; planted only)
            inside = self.means["first"] <= a.get("first", 0) and a.get("first", 0) + a.get("count", 1) <= self.means["first"] + self.means["count"]
            if not (self.means["what"] & mean_rule.GROUP_OF[a["plane"]] and inside): return "mean_info"
        return None

    def missing(self, kind):
        """A query of something the handle does not hold now: the kind of the call that makes it."""
        need = {"history": (self.hist is not None, "history_start"), "trail": (self.trail or self.batch > 0, "trail_start"),
                "frames": (self.rec, "record_start"), "record_view": (self.rec, "record_start"),
                "loads_history": (self.loads is not None, "loads_start"), "friction_history": (self.friction is not None, "friction_start"),
                "torque_history": (self.torque is not None, "torque_start"), "mean_sums": (self.means is not None, "mean_start"),
                "mean_sample": (self.means is not None, "mean_start")}
        if self.batch:
            need.update(residual=(self.norms, "step_n_each"), iterations=(self.iters, "step_n_until"))
        have, maker = need.get(kind, (True, None))
        return None if have else maker

    def after(self, kind, a):
        """The state behind a call the header took."""
        if kind == "set_solids":
            members = range(self.batch) if a.get("per_member") else [None]
            self.masks = [solid_mask(a["mask_kind"], self.dim_x, self.dim_y, a["seed"], k) for k in members]
        if kind == "clear_solids": self.masks = None
        if kind == "history_start": self.hist = [a["every"], a["capacity"], 0]
        if kind == "history_stop": self.hist = None
        if kind in STEPS and self.hist is not None: self.hist[2] += a.get("n", 1)
        if kind == "record_start": self.rec, self.view = True, None
        if kind == "record_view": self.view = a["what"]
        if kind == "record_stop": self.rec, self.view = False, None
        if kind == "trail_start": self.trail = True
        if kind in ("trail_stop", "set_tracers"): self.trail = False
        if kind == "set_viscosity":
            self.visc = {"nu": list(a["nu"]) if a.get("per_member") else [a["nu"]], "sweeps": a["sweeps"], "per_member": bool(a.get("per_member"))}
            if not self.batch and (a["nu"] == 0 or a["sweeps"] == 0): self.visc = None      # (a context: cleared)
        if kind == "clear_viscosity": self.visc = None
        if kind == "diffuse_velocity" and launches_of(a["nu"], a["sweeps"]) == 2: self.two_launches += 1
        if kind == "set_bodies": self.labels = None if a["label_kind"] == "all one" else a["label_kind"]
        if kind == "clear_bodies": self.labels = None
        if kind == "loads_start": self.loads = [a["every"], a["capacity"], 0]
        if kind == "loads_stop": self.loads = None
        if kind in STEPS and self.loads is not None: self.loads[2] += a.get("n", 1)
        if kind in ("set_bodies", "clear_bodies"):
            bodies = LABEL_KINDS[a["label_kind"]] if kind == "set_bodies" else 1
            if bodies != self.bodies: self.bodies, self.pivots = bodies, None      # "TORQUE": another number of bodies: every pivot back to (0, 0)
        if kind == "set_body_pivots": self.pivots = None if a["pivot_kind"] is None else dict(a)
        if kind in ("loads_start", "friction_start", "torque_start", "mean_start"): self.ranges[kind[:-len("_start")]] = (a.get("first", 0), a.get("count", 1))
        if kind == "friction_start": self.friction = [a["every"], a["capacity"], 0]
        if kind == "friction_stop": self.friction = None
        if kind == "torque_start": self.torque = [a["every"], a["capacity"], 0]
        if kind == "torque_stop": self.torque = None
        for recorder in (self.friction, self.torque):
            if kind in STEPS and recorder is not None: recorder[2] += a.get("n", 1)
        if kind == "mean_start": self.means = {"what": a["what"], "every": a["every"], "first": a.get("first", 0), "count": a.get("count", 1), "steps": 0, "samples": 0}
        if kind == "mean_stop": self.means = None
        if kind == "mean_sample": self.means["samples"] += 1
        if kind in STEPS and self.means is not None and self.means["every"] >= 1:
            m, n = self.means, a.get("n", 1)
            m["samples"] += (m["steps"] + n) // m["every"] - m["steps"] // m["every"]
            m["steps"] += n
        if kind == "set_openings":
            members = range(self.batch) if a.get("per_member") else [None]
            self.open = [open_map(a["open_kind"], self.dim_x, self.dim_y, a["seed"], k) for k in members]
            self.inflow, self.profile = [tuple(u) for u in a["inflow"]] if a.get("inflow_per_member") else [tuple(a["inflow"])], None
        if kind == "clear_openings": self.open, self.inflow, self.profile = None, None, None
        if kind == "set_inflow": self.inflow = [tuple(u) for u in a["inflow"]] if a.get("per_member") else [tuple(a["inflow"])]
        if kind == "set_inflow_profile": self.profile = dict(a) if a["cells"] else None
        if self.batch:
            if kind in ("step_n", "poisson_solve") or (kind == "upload" and a["field"] in (FD, FP)): self.norms = self.iters = False
            if kind in ("step_n_each", "poisson_solve_each"): self.norms, self.iters = True, False
            if kind in ("step_n_until", "poisson_solve_until"): self.norms = self.iters = True


def gated(ops, subject, case):
    """For the census of a subject with solids: (index, op, the Gate WHILE the op runs, whether the header refuses it)."""
    gate = Gate(subject.batch, case[0], case[1])
    for k, (kind, a) in enumerate(ops):
        refused = gate.remedy(kind, a) is not None
        yield k, (kind, a), gate, refused
        if not refused:
            gate.after(kind, a)


class _Draw:
    """Literal arguments of one case's ops; it follows the little state the choice of valid arguments needs."""

    def __init__(self, subject, case, oracle):
        self.sub, (self.dim_x, self.dim_y, seed) = subject, case
        self.rng = np.random.default_rng([seed, 7])
        self.lattice = False          # the velocity came from a landing / whole-cell upload: steps take dt = 0.25
        self.halo_fixed = False
        self.shadow = subject.model(oracle, case) if subject.kind == "slabs" else None   # slabs: the reach of every advection under a fixed halo
        self.gate = Gate(subject.batch, self.dim_x, self.dim_y) if subject.solids else None
        self.hints = {}

    def pick(self, values):
        v = values[int(self.rng.integers(len(values)))]
        return v if v is None or isinstance(v, (str, bool)) else (int(v) if isinstance(v, (int, np.integer)) else float(v))

    def dt(self): return 0.25 if self.lattice else self.pick(DTS)
    def iters(self, still=False): return 0 if (still and self.lattice and self.sub.still_solves) else int(self.rng.integers(0, MAX_ITERS + 1))
    def solve(self, still=False): return {"dx": self.pick(DXS), "iters": self.iters(still), "omega": self.pick(OMEGAS)}
    def stepargs(self): return dict({"dt": self.dt()}, **self.solve(True))
    def each(self, f): return [f() for _ in range(self.sub.batch)]

    def cells(self, n):
        edge = [(0, 0), (self.dim_x - 1, self.dim_y - 1), (self.dim_x, 1), (self.dim_x // 2, self.dim_y // 2)]
        if self.sub.nranks > 1:       # both sides of the first cut
            cut = self.dim_y // self.sub.nranks
            edge += [(3, cut), (4, cut - 1)]
        out = [edge[int(self.rng.integers(len(edge)))] if self.rng.integers(3) == 0 else
               (int(self.rng.integers(self.dim_x)), int(self.rng.integers(self.dim_y))) for _ in range(n)]
        return [list(c) for c in out]

    def vels(self, n):
        return [[float(x) for x in np.round(self.rng.uniform(-60, 60, 2) * 2) / 2] for _ in range(n)]

    def positions(self, n):
        return [[float(np.round(self.rng.uniform(-1.5, self.dim_x + 0.5) * 8) / 8), float(np.round(self.rng.uniform(-1.5, self.dim_y + 0.5) * 8) / 8)]
                for _ in range(n)]

    def make(self, kind, **fixed):
        """The op of `kind` with drawn arguments (those in `fixed` as given; a key that starts with "_" is a hint to the draw
        and no argument).  plan() has ordered the kinds so that it is valid here."""
        self.hints = {k: fixed.pop(k) for k in list(fixed) if k.startswith("_")}
        a = self._args(kind, self.sub.kind == "batch")
        a.update(fixed)
        if kind == "set_bodies":
            a["bodies"] = LABEL_KINDS[a["label_kind"]]
        if kind in ("set_openings", "set_inflow") and self.sub.kind == "batch":      # one (u, v), or one per member: as the flag says
            each, nested = a["inflow_per_member" if kind == "set_openings" else "per_member"], isinstance(a["inflow"][0], list)
            if each and not nested:
                a["inflow"] = [list(INFLOWS[(INFLOWS.index(tuple(a["inflow"])) + k) % len(INFLOWS)]) for k in range(self.sub.batch)]
            elif nested and not each:
                a["inflow"] = a["inflow"][0]
        op = (kind, a)
        if self.shadow is not None:
            op = self._under_the_halo(op)
        if self.gate is not None:
            op = self._give_way(op)
        self._follow(op)
        return op

    def _give_way(self, op):
        """Solids and histories: only the refusals that were planted happen.  Any other call the header would refuse in the
        state the sequence has reached, and a query of what the handle does not hold, gives way to the call that ends the
        cause (a mask cleared, a history stopped or started, a report written)."""
        planted_refusal = self.hints.get("_refused", False)
        for _ in range(4):
            kind, a = op
            instead = self.gate.missing(kind) or (None if planted_refusal else self.gate.remedy(kind, a))
            if instead is None:
                break
            if a.get("what") == VIEW_DIVERGENCE and instead in ("clear_solids", "clear_openings"):     # (another view will do)
                op = (kind, dict(a, what=int(self.rng.integers(VIEW_DIVERGENCE))))
                continue
            self.hints, planted_refusal = {}, False
            op = (instead, self._args(instead, self.sub.kind == "batch"))
        if self.gate.remedy(*op) is None:
            self.gate.after(*op)
        return op

    def pick_pair(self, values):
        return values[int(self.rng.integers(len(values)))]

    def profile_args(self, batch):
        """The records of a set_inflow_profile on INFLOW cells of the map held -- of every member's map where a record goes to
        all: three drawn cells, the first once more (of two records on one cell the later wins) and the second with the uniform
        inflow as its velocity.  Hints: "_mask" (kind, seed): the first cell is one that this mask, set by a later link, makes
        solid; "_off": one more record on an interior cell, whose byte is not INFLOW (refused with SFL_ERR_INVALID); "_clear":
        n == 0; "_members": every record names its member.  A map without an inflow cell leaves n == 0."""
        r, B, gate = self.rng, max(self.sub.batch, 1), self.gate
        shared = {"members": None} if batch else {}
        if gate.open is None:               # (without openings: refused where planted, else the call gives way to set_openings)
            return dict({"cells": [[0, self.dim_y // 2]], "vels": [[1.0, 0.0]]}, **shared)
        if self.hints.get("_clear"):
            return dict({"cells": [], "vels": []}, **shared)
        per_record = bool(batch and self.hints.get("_members", bool(r.integers(2))))
        cells, vels, members = [], [], []
        for at in range(3):
            m = int(r.integers(B)) if per_record else None
            inflow = np.all([held == opening_rule.INFLOW for held in gate.maps_of(range(B) if m is None else [m])], axis=0)
            pool = np.argwhere(inflow)
            if at == 0 and "_mask" in self.hints:
                solid = np.argwhere(inflow & solid_mask(self.hints["_mask"][0], self.dim_x, self.dim_y, self.hints["_mask"][1]))
                pool = solid if len(solid) else pool
            if len(pool):
                j, i = pool[int(r.integers(len(pool)))]
                cells.append([int(i), int(j)]), vels.append(self.vels(1)[0]), members.append(m)
        if cells:
            if len(cells) >= 2:
                vels[1] = [float(x) for x in gate.inflow[members[1] if members[1] is not None and len(gate.inflow) > 1 else 0]]
            cells.append(list(cells[0])), vels.append(self.vels(1)[0]), members.append(members[0])
        if self.hints.get("_off"):
            cells.append([1, 1]), vels.append(self.vels(1)[0]), members.append(members[0] if members else (0 if per_record else None))
        return dict({"cells": cells, "vels": vels}, **({"members": members if per_record else None} if batch else {}))

    def cells_on(self, masks, members):
        """One cell per entry of `members`, in turn a solid and a fluid cell of the member's mask (any cell where it has none)."""
        out = []
        for at, m in enumerate(members):
            mask = masks[m if len(masks) > 1 else 0]
            pool = np.argwhere(mask if at % 2 == 0 else ~mask)
            j, i = pool[int(self.rng.integers(len(pool)))] if len(pool) else (int(self.rng.integers(self.dim_y)), int(self.rng.integers(self.dim_x)))
            out.append([int(i), int(j)])
        return out

    def _args(self, kind, batch):
        r, B = self.rng, self.sub.batch
        if kind == "upload":
            return {"field": int(r.integers(4)), "texture_kind": self.pick(TEXTURES), "seed": int(r.integers(1000))}
        if kind in ("advect_velocity", "advect_color"): return {"dt": self.dt(), "no_slip": bool(r.integers(2))}
        if kind in ("calculate_divergence", "subtract_gradient"): return {"dx": self.pick(DXS)}
        if kind in ("poisson_solve", "poisson_continue"): return self.solve()
        if kind == "poisson_solve_until" and not batch: return dict(self.solve(), tol=self.pick(TOLS), every=self.pick(EVERYS))
        if kind == "step": return self.stepargs()
        if kind == "step_n" : return dict({"n": int(r.integers(1, 5))}, **self.stepargs())
        if kind in ("step_n_each", "step_n_until", "poisson_solve_each", "poisson_solve_until"):
            a = {"dx": self.each(lambda: self.pick(DXS)), "iters": self.each(self.iters), "omega": self.each(lambda: self.pick(OMEGAS))}
            if kind.startswith("step"):
                a = dict({"n": int(r.integers(1, 5)), "dt": self.each(self.dt)}, **a)
            if kind.endswith("until"):
                a.update(tol=self.each(lambda: self.pick(TOLS)), every=self.each(lambda: self.pick(EVERYS)))
            return a
        if kind == "queue_forces" and self.hints.get("_open"):
            # under a map, by the hint: a record on an inflow cell, one on a profiled cell and one on an outflow cell (items 2 and 2a)
            members, cells, held = [int(r.integers(B)) for _ in range(3)] if batch else [0] * 3, [], self.gate.profile
            for at, m in enumerate(members):
                byte = opening_rule.OUTFLOW if at == 2 else opening_rule.INFLOW
                pool = [[i, j] for j, i in np.argwhere(self.gate.maps_of([m])[0] == byte)]
                if at == 1 and held is not None:
                    named = [c for k, c in enumerate(held["cells"]) if held.get("members") is None or held["members"][k] == m]
                    pool = named or pool
                cells.append([int(x) for x in pool[int(r.integers(len(pool)))]] if pool else self.cells(1)[0])
            a = {"step": int(r.integers(0, 2)), "cells": cells, "vels": self.vels(3)}
            return dict(a, members=members) if batch else a
        if kind == "queue_forces" and self.gate is not None and ("_mask" in self.hints or self.gate.masks is not None):
            # with a mask in force (or, by the hint, about to be set): records on solid cells and on fluid ones
            masks = [solid_mask(self.hints["_mask"][0], self.dim_x, self.dim_y, self.hints["_mask"][1])] if "_mask" in self.hints else self.gate.masks
            n = int(r.integers(2, 4))
            members = [int(r.integers(B)) for _ in range(n)] if batch else [0] * n
            a = {"step": int(r.integers(0, 4)), "cells": self.cells_on(masks, members), "vels": self.vels(n)}
            return dict(a, members=members) if batch else a
        if kind == "set_solids":
            a = {"mask_kind": self.pick(MIXED_KINDS), "seed": int(r.integers(100))}
            return dict(a, per_member=bool(r.integers(2))) if batch else a
        if kind == "history_start":
            a = {"every": self.pick((1, 2, 3)), "capacity": self.pick((2, CAPACITY))}
            if batch:
                first = int(r.integers(B))
                a.update(first=first, count=int(r.integers(1, B - first + 1)))
            return a
        if kind == "set_viscosity":
            if not batch: return {"nu": self.pick(NUS), "sweeps": self.pick(CONTEXT_SWEEPS)}
            per_member = bool(r.integers(2))
            return {"nu": self.each(lambda: self.pick(NUS)) if per_member else self.pick(NUS), "sweeps": self.pick(BATCH_SWEEPS), "per_member": per_member}
        if kind == "diffuse_velocity": return {"nu": self.pick(NUS), "dt": self.dt(), "dx": self.pick(DXS), "sweeps": self.pick(CONTEXT_SWEEPS)}
        if kind == "set_bodies":
            a = {"label_kind": self.pick(sorted(LABEL_KINDS)), "seed": int(r.integers(100))}
            a["bodies"] = LABEL_KINDS[a["label_kind"]]
            return dict(a, per_member=bool(r.integers(2))) if batch else a
        if kind == "loads_start":
            a = {"every": self.pick((1, 2, 3)), "capacity": self.pick((2, CAPACITY))}
            if batch:
                first = int(r.integers(B))
                a.update(first=first, count=int(r.integers(1, B - first + 1)))
            return a
        if kind in ("loads", "friction", "torque", "openings_flux") and batch:
            first = int(r.integers(B))
            return {"first": first, "count": int(r.integers(1, B - first + 1))}
        if kind in ("friction_start", "torque_start"):      # (room for every sample of a sequence: a full one is planted, with its stop)
            a = {"every": self.pick((1, 2, 3)), "capacity": CAPACITY}
            if batch:
                first = int(r.integers(B))
                a.update(first=first, count=int(r.integers(1, B - first + 1)))
            return a
        if kind == "set_body_pivots":       # `bodies` as the handle holds them ("_wrong": another number, refused with SFL_ERR_INVALID)
            a = {"pivot_kind": self.pick(PIVOT_KINDS), "bodies": self.gate.bodies + (1 if self.hints.get("_wrong") else 0), "seed": int(r.integers(100))}
            return dict(a, per_member=bool(r.integers(2))) if batch else a
        if kind == "mean_start":
            a = {"what": self.pick(MEAN_WHATS), "every": self.pick((0, 1, 2, 3))}
            if batch:
                first = int(r.integers(B))
                a.update(first=first, count=int(r.integers(1, B - first + 1)))
            return a
        if kind == "mean_sums":             # a plane of the groups held ("_outside": of another group, refused with SFL_ERR_INVALID)
            held = self.gate.means or {"what": mean_rule.ALL, "first": 0, "count": max(B, 1)}
            planes = [k for k in range(mean_rule.PLANES) if bool(held["what"] & mean_rule.GROUP_OF[k]) != bool(self.hints.get("_outside"))]
            a = {"plane": int(planes[int(r.integers(len(planes)))])}
            if batch:                       # a range inside the recorded one
                first = held["first"] + int(r.integers(held["count"]))
                a.update(first=first, count=int(r.integers(1, held["first"] + held["count"] - first + 1)))
            return a
        if kind == "set_openings":
            a = {"open_kind": self.pick(OPEN_KINDS), "seed": int(r.integers(100)), "inflow": list(self.pick_pair(INFLOWS))}
            return dict(a, per_member=bool(r.integers(2)), inflow_per_member=bool(r.integers(2))) if batch else a
        if kind == "set_inflow":
            a = {"inflow": list(self.pick_pair(INFLOWS))}
            return dict(a, per_member=bool(r.integers(2))) if batch else a
        if kind == "set_inflow_profile":
            return self.profile_args(batch)
        if kind == "inflow_profile" and batch: return {"member": int(r.integers(B))}
        if kind == "queue_forces":
            n = int(r.integers(1, 4))
            a = {"step": int(r.integers(0, 4)), "cells": self.cells(n), "vels": self.vels(n)}
            return dict(a, members=[int(r.integers(B)) for _ in range(n)]) if batch else a
        if kind == "queue_drags":
            return {"step": int(r.integers(0, 3)), "drags": [[int(r.integers(self.dim_y)), int(r.integers(self.dim_x))] + self.vels(1)[0] for _ in range(2)]}
        if kind == "set_tracers":
            return {"xy": self.each(lambda: self.positions(4)) if batch else self.positions(5), "follow": bool(r.integers(2))}
        if kind == "advance_tracers": return {"dt": self.dt()}
        if kind == "trail_start": return {"every": int(r.integers(1, 3))}
        if kind == "set_option":
            name = self.pick(sorted(self.sub.option_values()))
            return {"name": name, "value": self.pick(self.sub.option_values()[name])}
        if kind == "record_start":
            first = int(r.integers(B))
            return {"every": int(r.integers(1, 3)), "first": first, "count": int(r.integers(1, B - first + 1)), "scaling": int(r.integers(1, 3)), "byteswap": bool(r.integers(2))}
        if kind == "record_view": return {"what": self.pick([None, 0, 1, 2, 3])}
        if kind == "envelope":
            first = int(r.integers(B))
            return {"first": first, "count": int(r.integers(1, B - first + 1))}
        if kind == "download": return {"field": int(r.integers(4))}
        if kind == "residual": return {} if batch else {"dx": self.pick(DXS)}
        if kind == "flow_stats": return {"dx": self.pick(DXS)}
        if kind in ("view_scalar", "view_texels"): return {"what": int(r.integers(4)), "dx": self.pick(DXS)}
        if kind in ("render_rgb565", "render_members"): return {"scaling": int(r.integers(1, 3)), "byteswap": bool(r.integers(2))}
        if kind == "view_render_members": return {"what": int(r.integers(4)), "scaling": int(r.integers(1, 3))}
        if kind == "sample_tracers": return {"field": int(r.integers(4)), "no_slip": bool(r.integers(2))}
        if kind == "distance": return {"ref_member": int(r.integers(B))} if batch else {}
        if kind == "envelope_field": return {"which": int(r.integers(4))}
        return {}

    def _under_the_halo(self, op):
        """Slabs: include/sfl.h makes a back-trace that leaves a FIXED advection halo an error, so no op may make one: under
        a fixed halo such an op takes the shortest dt, and where that is still too far it gives way to the option change
        that ends the fixed halo; the halo is not fixed while the velocity held is too fast for it."""
        kind, a = op
        if kind == "set_option" and a["name"] == "OPT_ADVECT_HALO" and a["value"] > 0:
            with np.errstate(all="ignore"):
                if float(np.max(np.abs(self.shadow.v[..., 1]))) * min(DTS) > SAFE_REACH:
                    op = (kind, dict(a, value=0))
        trial = _copy_model(self.shadow)
        if kind not in QUERIES:
            trial.apply(op)
            if self.halo_fixed and trial.reach > SAFE_REACH and "dt" in a:
                op, trial = (kind, dict(a, dt=min(DTS))), _copy_model(self.shadow)
                trial.apply(op)
            if self.halo_fixed and trial.reach > SAFE_REACH:
                op, trial = ("set_option", {"name": "OPT_ADVECT_HALO", "value": 0}), self.shadow
        if op[0] == "set_option" and op[1]["name"] == "OPT_ADVECT_HALO":
            self.halo_fixed = op[1]["value"] > 0
        self.shadow = trial
        return op

    def _follow(self, op):
        """Whether the velocity is still on the lattice its upload put it on (steps without a solve and advections by dt = 0.25 keep it there)."""
        kind, a = op
        if kind == "upload" and a["field"] == FV: self.lattice = a["texture_kind"] in ("landing", "whole-cell")
        if kind in ("subtract_gradient", "queue_forces", "queue_drags"): self.lattice = False
        if kind in ("step", "step_n", "step_n_each", "step_n_until") and not self.sub.still_solves: self.lattice = False


def _copy_model(m):
    twin = type(m)(m.o, m.dim_x, m.dim_y)
    twin.v, twin.c, twin.d, twin.p = m.v, m.c, m.d, m.p          # (every op replaces arrays, none writes into one)
    twin.timeline = {s: list(r) for s, r in m.timeline.items()}
    return twin


# a hand-over is a list of (kind, fixed arguments, predicate on the finished op)
def _n2(a): return a["n"] >= 2


HANDOVERS = {
    "upload(velocity) -> step": [("upload", {"field": FV}, None), ("step", {}, None)],
    "upload(pressure) -> poisson_continue": [("upload", {"field": FP, "texture_kind": "noise"}, None), ("poisson_continue", {"iters": 3}, None)],
    "query -> poisson_continue": [("residual", {}, None), ("poisson_continue", {"iters": 2}, None)],
    "set_option -> step_n(n >= 2)": [("set_option", {}, None), ("step_n", {}, _n2)],
    "queue_forces(step >= 1) -> step_n(n >= 2) -> step": [("queue_forces", {"step": 2}, None), ("step_n", {"n": 2}, None), ("step", {}, None)],
    "step_n -> queue_forces(step = 0) -> step": [("step_n", {}, None), ("queue_forces", {"step": 0}, None), ("step", {}, None)],
    "set_tracers(follow) -> step_n(n >= 2) -> set_tracers(follow=False) -> step_n(n >= 2)":
        [("set_tracers", {"follow": True}, None), ("step_n", {"n": 2}, None), ("set_tracers", {"follow": False}, None), ("step_n", {"n": 3}, None)],
    "advect_color -> upload(velocity) -> step": [("advect_color", {}, None), ("upload", {"field": FV}, None), ("step", {}, None)],
}
SLAB_HANDOVERS = ("upload(velocity) -> step", "set_option -> step_n(n >= 2)", "queue_forces(step >= 1) -> step_n(n >= 2) -> step",
                  "step_n -> queue_forces(step = 0) -> step", "advect_color -> upload(velocity) -> step")
BATCH_HANDOVERS = {   # a call that runs one launch per step, a replay of the timeline in one launch (no following set, a record in
                      # a later step), and a per-step call again, with the recorder started in between
    "per-step call -> record_start -> one-launch replay -> per-step call":
        [("set_tracers", {"follow": False}, None), ("step_n", {"n": 1}, None), ("record_start", {}, None),
         ("queue_forces", {"step": 1}, None), ("step_n", {"n": 3}, None), ("step_n", {"n": 1}, None)],
}


def _link(kind, pred=None, **fixed): return (kind, fixed, pred)


_DIV, _STEP2 = {"what": VIEW_DIVERGENCE}, _link("step_n", _n2)
SOLID_HANDOVERS = {
    "context": {
        "set_solids -> step_n(n >= 2) -> set_solids (no clear) -> step -> clear_solids -> step_n(n >= 2)":
            [_link("set_solids"), _STEP2, _link("set_solids"), _link("step"), _link("clear_solids"), _STEP2],
        "clear_solids -> set_option(OPT_ADVECT_KERNEL, 2) -> step_n(n >= 2) -> set_solids -> step":
            [_link("clear_solids"), _link("set_option", name="OPT_ADVECT_KERNEL", value=2), _STEP2, _link("set_solids"), _link("step")],
        "clear_solids -> step -> set_solids -> poisson_solve -> clear_solids -> poisson_solve":
            [_link("clear_solids"), _link("step"), _link("set_solids"), _link("poisson_solve"), _link("clear_solids"), _link("poisson_solve")],
        "upload(pressure) -> set_solids -> poisson_continue(3) -> download(pressure) -> poisson_continue(9) -> residual -> poisson_solve_until":
            [_link("upload", field=FP, texture_kind="noise"), _link("set_solids"), _link("poisson_continue", iters=3), _link("download", field=FP),
             _link("poisson_continue", iters=9), _link("residual"), _link("poisson_solve_until")],
        "queue_forces(step = 2) -> set_solids -> step_n(n = 2) -> step": [_link("queue_forces", step=2), _link("set_solids"), _link("step_n", n=2), _link("step")],
        "set_tracers(follow) -> trail_start -> set_solids -> step_n(2) -> clear_solids -> step_n(2)":
            [_link("set_tracers", follow=True), _link("trail_start"), _link("set_solids"), _link("step_n", n=2), _link("clear_solids"), _link("step_n", n=2)],
        "history_start(every = 1) -> step -> set_solids -> step_n(2) -> history -> clear_solids -> step_n(2) -> history":
            [_link("history_start", every=1), _link("step"), _link("set_solids"), _link("step_n", n=2), _link("history"), _link("clear_solids"),
             _link("step_n", n=2), _link("history")],
        "view_scalar(divergence), refused -> step": [_link("view_scalar", **_DIV), _link("step")],
        "view_texels(divergence), refused -> step_n": [_link("view_texels", **_DIV), _link("step_n")],
        "history_start(capacity = 2) -> step_n(3), refused -> step -> history": [_link("history_start", every=1, capacity=2), _link("step_n", n=3), _link("step"), _link("history")],
    },
    "batch": {
        "set_solids -> step_n(n >= 2) -> set_solids (no clear) -> step_n -> clear_solids -> step_n(n >= 2)":
            [_link("set_solids", per_member=False), _STEP2, _link("set_solids", per_member=True), _link("step_n"), _link("clear_solids"), _STEP2],
        "queue_forces(step = 2) -> set_solids -> step_n(n = 2) -> step_n": [_link("queue_forces", step=2), _link("set_solids"), _link("step_n", n=2), _link("step_n", n=1)],
        "set_tracers(follow) -> set_solids -> step_n(2) -> clear_solids -> step_n(2)":
            [_link("set_tracers", follow=True), _link("set_solids"), _link("step_n", n=2), _link("clear_solids"), _link("step_n", n=2)],
        "history_start -> set_solids, refused -> step_n -> history_stop -> set_solids -> history_start, refused -> step_n_each -> residual":
            [_link("history_start"), _link("set_solids"), _link("step_n"), _link("history_stop"), _link("set_solids"), _link("history_start"),
             _link("step_n_each"), _link("residual")],
        "set_solids -> step_n_until, refused -> step_n -> poisson_solve_until, refused -> step_n_each":
            [_link("set_solids"), _link("step_n_until"), _link("step_n"), _link("poisson_solve_until"), _link("step_n_each")],
        "record_start -> set_solids -> record_view(divergence), refused -> step_n": [_link("record_start"), _link("set_solids"), _link("record_view", **_DIV), _link("step_n")],
        "view_render_members(divergence), refused -> step_n": [_link("view_render_members", **_DIV), _link("step_n")],
        "record_view(divergence) -> set_solids, refused -> step_n": [_link("record_view", **_DIV), _link("set_solids"), _link("step_n")],
        "history_start(capacity = 2) -> step_n(3), refused -> step_n(1) -> history": [_link("history_start", every=1, capacity=2), _link("step_n", n=3), _link("step_n", n=1), _link("history")],
    },
}


def handovers_of(subject):
    if subject.viscous or subject.opens:
        return viscous_handovers(subject)
    if subject.solids:
        return SOLID_HANDOVERS[subject.kind]
    if subject.kind == "batch":
        return BATCH_HANDOVERS
    return HANDOVERS if subject.kind == "context" else {k: HANDOVERS[k] for k in SLAB_HANDOVERS}


def has_handover(ops, chain):
    """The chain's ops stand next to each other somewhere in ops."""
    fits = lambda op, link: op[0] == link[0] and all(op[1].get(k) == v for k, v in link[1].items()) and (link[2] is None or link[2](op[1]))
    return any(all(fits(ops[at + k], link) for k, link in enumerate(chain)) for at in range(len(ops) - len(chain) + 1))


def _opt(name, value, **hints): return ("set_option", dict({"name": name, "value": value}, **hints))
def _up(texture_kind, field=FV): return ("upload", {"field": field, "texture_kind": texture_kind})


def planted(subject):
    """The items the generator plants whole (the ops of an item stay next to each other): the hand-overs, and every option
    value in front of a writer it affects, so that no value is only ever set."""
    kind = subject.kind
    if subject.viscous or subject.opens:
        return planted_viscous(subject)
    if subject.solids:
        return planted_solids(subject)
    if kind == "batch":
        pairs = [[(w, {}), (q, {})] for w, q in (("step_n_each", "residual"), ("poisson_solve_each", "residual"), ("step_n_each", "residual"),
                                                  ("step_n_until", "iterations"), ("poisson_solve_until", "iterations"), ("step_n_until", "iterations"))]
        return [[(k, dict(f)) for k, f, _ in BATCH_HANDOVERS["per-step call -> record_start -> one-launch replay -> per-step call"]]] + pairs
    step, step2 = ("step", {}), ("step_n", {"n": 2})
    items = [
        [("forget_forces", {}), ("queue_forces", {"step": 2}), step2, step],     # (nothing else pending: both steps of the call are joined)
        ([("forget_forces", {})] if subject.still_solves else []) + [("advect_color", {}), _up("landing"), step] + ([step2] if subject.still_solves else []),
        # (the switches the fused step boundary depends on are only off inside their own items)
        [_opt("OPT_FUSE_DIVERGENCE", 0), _opt("OPT_FUSE_PROJECTION", 0), step, _opt("OPT_FUSE_DIVERGENCE", 1), _opt("OPT_FUSE_PROJECTION", 1)],
        [_opt("OPT_ADVECT_KERNEL", 2), ("advect_velocity", {}), ("calculate_divergence", {}), ("subtract_gradient", {}), ("advect_color", {})] +
        ([step] if subject.name == "general" else []),
        [_opt("OPT_ADVECT_KERNEL", 1), ("advect_velocity", {}), _opt("OPT_ADVECT_KERNEL", 0), ("advect_velocity", {})],
        [_opt("OPT_SOR_KERNEL", 1), ("poisson_solve", {})], [_opt("OPT_SOR_KERNEL", 2), _opt("OPT_SOR_FUSE", 2), ("poisson_solve", {})],
        [_opt("OPT_SOR_FUSE", 16), ("poisson_solve", {})],
    ]
    if kind == "context":
        items += [
            [_up("noise", FP), ("poisson_continue", {"iters": 3}), ("residual", {}), ("poisson_continue", {"iters": 2})],
            [("set_tracers", {"follow": True}), step2, ("set_tracers", {"follow": False}), ("step_n", {"n": 3}), ("queue_forces", {"step": 0}), step],
            [_opt("OPT_SOR_KERNEL", 0), ("poisson_solve_until", {})], [_opt("OPT_SOR_FUSE", 0), ("poisson_solve_until", {})],
        ]
        if subject.still_solves:    # exact sources at the fused step boundary: every condition of the seam set in front of it
            items += [[("forget_forces", {}), _up("whole-cell"), ("step_n", {"n": 3})],
                      [_opt("OPT_STEP_SEAMS", 0), step2, _opt("OPT_STEP_SEAMS", 1)], [_opt("OPT_SMALL_GRID", 0)], [_opt("OPT_SMALL_GRID", 1)]]
        elif subject.name == "general":
            items += [[_opt("OPT_STEP_SEAMS", 0), ("step_n", {"n": 3})], [_opt("OPT_STEP_SEAMS", 1), step2], [_opt("OPT_SMALL_GRID", 0)], [_opt("OPT_SMALL_GRID", 1)]]
        else:                       # the one-workgroup path, the general kernels and back, a writer after each flip
            items += [[_opt("OPT_STEP_SEAMS", 0), ("step_n", {"n": 3})], [_opt("OPT_STEP_SEAMS", 1), step2],
                      [_up("noise"), _opt("OPT_SOR_KERNEL", 0), _opt("OPT_SOR_FUSE", 0), _opt("OPT_ADVECT_KERNEL", 0), _opt("OPT_SMALL_GRID", 1), step,
                       _opt("OPT_SMALL_GRID", 0), step, ("poisson_solve", {}), _opt("OPT_SMALL_GRID", 1), step2, ("poisson_solve", {})],
                      [_opt("OPT_SOR_KERNEL", 2), step, _opt("OPT_SOR_KERNEL", 0), step]]
    else:                           # slabs: the velocity flips by upload on a handle that has stepped; both advection halos; both solve halos
        items += [
            [("step_n", {}), ("queue_forces", {"step": 0}), step],
            [_opt("OPT_STEP_SEAMS", 0), ("step_n", {"n": 3})], [_opt("OPT_STEP_SEAMS", 1), step2], [_opt("OPT_SMALL_GRID", 0), step], [_opt("OPT_SMALL_GRID", 1), step],
            [_opt("OPT_ADVECT_HALO", 0), step, _up("fast"), step, step, _up("still"), step, _up("noise"), step, step, _up("fast"), step],
            [_up("noise"), _opt("OPT_ADVECT_HALO", FIXED_HALO), step, step, ("advect_velocity", {}), ("advect_color", {})],
            [_opt("OPT_SOR_KERNEL", 0), _opt("OPT_SOR_FUSE", 0), _opt("OPT_SOR_HALO", 16), ("poisson_solve", {}), step],
            [_opt("OPT_SOR_HALO", 32), ("poisson_solve", {}), step], [_opt("OPT_SOR_HALO", 0), ("poisson_solve", {}), step],
        ]
    return items


def _solid(mask_kind, **more): return ("set_solids", dict({"mask_kind": mask_kind}, **more))


def planted_solids(subject):
    """The items of the subjects with solids and histories.  A link may carry hints to the draw: "_refused" (the header
    refuses the call here, on purpose), "_mask" (the mask the next link sets), "_shape" on an item's first link (the item goes
    to a case of that shape).  Every item that needs the mask clear, the history off or nothing pending says so itself."""
    clear, refused = ("clear_solids", {}), {"_refused": True}
    div = dict(what=VIEW_DIVERGENCE, **refused)
    if subject.kind == "context":
        step, step2 = ("step", {}), ("step_n", {"n": 2})
        return [
            # a mask replaced without a clear in between, and cleared, on fields left as they are (no upload anywhere)
            [_solid("disc"), step2, _solid("seeded"), step, clear, ("step_n", {"n": 3}), ("flow_stats", {})],
            # cleared: the step seams run again (every condition of the seam set in front), then a mask again
            [("forget_forces", {"_shape": (130, 70)}), ("history_stop", {}), ("set_tracers", {"follow": False}), clear, _opt("OPT_ADVECT_KERNEL", 2), step2,
             _solid("plate"), step],
            # cleared: the one-launch step of a small grid, and the small grid's solve behind a masked one
            [_opt("OPT_SOR_KERNEL", 0, _shape=(61, 81)), _opt("OPT_SOR_FUSE", 0), _opt("OPT_ADVECT_KERNEL", 0), _opt("OPT_SMALL_GRID", 1), clear, step,
             _solid("channel"), ("poisson_solve", {}), clear, ("poisson_solve", {}), ("residual", {})],
            # a held pressure over one launch of the masked solve (it ends in the partner's buffer), then over two
            [_up("noise", FP), _solid("seeded"), ("poisson_continue", {"iters": 3}), ("download", {"field": FP}), ("poisson_continue", {"iters": 9}),
             ("residual", {}), ("poisson_solve_until", {})],
            # a record queued for a later step on a solid cell and one on a fluid cell of the mask set behind it
            [("forget_forces", {}), ("queue_forces", {"step": 2, "_mask": ("plate", 5)}), _solid("plate", seed=5), step2, step],
            [("set_tracers", {"follow": True}), ("trail_start", {}), _solid("disc"), step2, clear, step2, ("trail", {})],
            [("history_start", {"every": 1, "capacity": CAPACITY}), step, _solid("isolated"), step2, ("history", {}), clear, step2, ("history", {})],
            # a full history refuses the call whole; the next one fits
            [("history_start", {"every": 1, "capacity": 2}), ("step_n", dict(n=3, **refused)), step, ("history", {}), ("history_stop", {})],
            # every mask kind in front of a step call, and under it every value of every option in front of a writer it
            # would otherwise affect (no effect while solids are set); the divergence view refused in between
            [_solid("one"), _opt("OPT_ADVECT_KERNEL", 1), ("calculate_divergence", {}), ("subtract_gradient", {}), _opt("OPT_ADVECT_KERNEL", 0), step],
            [_solid("disc"), _opt("OPT_ADVECT_KERNEL", 2), ("calculate_divergence", {}), ("view_scalar", dict(div)), step, ("subtract_gradient", {}),
             ("view_texels", dict(div)), step2],
            [_solid("plate"), _opt("OPT_FUSE_DIVERGENCE", 0), _opt("OPT_FUSE_PROJECTION", 0), step, _opt("OPT_FUSE_DIVERGENCE", 1), _opt("OPT_FUSE_PROJECTION", 1)],
            [_solid("channel"), _opt("OPT_STEP_SEAMS", 0), step2, _opt("OPT_STEP_SEAMS", 1), step2],
            [_solid("isolated"), _opt("OPT_SMALL_GRID", 0), ("poisson_solve", {}), step, _opt("OPT_SMALL_GRID", 1), ("poisson_solve", {"iters": 0})],
            [_solid("all"), _opt("OPT_SOR_KERNEL", 1), ("poisson_solve", {}), _opt("OPT_SOR_KERNEL", 2), ("poisson_continue", {}), _opt("OPT_SOR_KERNEL", 0), step],
            [_solid("seeded"), _opt("OPT_SOR_FUSE", 2), ("poisson_solve", {}), _opt("OPT_SOR_FUSE", 16), ("poisson_solve_until", {}), _opt("OPT_SOR_FUSE", 0), step],
            [_solid("empty"), step],
        ]
    s1, s2, sn = ("step_n", {"n": 1}), ("step_n", {"n": 2}), ("step_n", {})
    again = ("set_solids", {})      # (an item that had to clear the mask sets one again: most of a sequence runs under a mask)
    return [
        [_solid("disc", per_member=False), s2, _solid("seeded", per_member=True), s1, clear, ("step_n", {"n": 3}), ("flow_stats", {}), again],
        [("forget_forces", {}), ("queue_forces", {"step": 2, "_mask": ("plate", 5)}), _solid("plate", seed=5, per_member=False), s2, s1],
        [("set_tracers", {"follow": True}), _solid("disc", per_member=True), s2, clear, s2, ("set_tracers", {"follow": False}), again],
        [clear, ("history_start", {"capacity": CAPACITY}), _solid("one", **refused), sn, ("history_stop", {}), _solid("channel"),
         ("history_start", dict(refused)), ("step_n_each", {}), ("residual", {})],
        [_solid("one", per_member=True), ("step_n_until", dict(refused)), sn, ("poisson_solve_until", dict(refused)), ("step_n_each", {}), ("residual", {})],
        # the recorder (the dye, then a view that is not the divergence) and the envelope next to a mask
        [("record_start", {}), _solid("isolated", per_member=False), ("record_view", dict(div)), s2, ("frames", {}), ("record_view", {"what": 1}), s2, ("frames", {}),
         ("view_render_members", dict(div)), sn, ("envelope", {}), ("envelope_field", {})],
        [clear, ("record_start", {}), ("record_view", {"what": VIEW_DIVERGENCE}), _solid("disc", **refused), sn, ("record_view", {"what": None}), again],
        [clear, ("history_start", {"every": 1, "capacity": 2, "first": 0, "count": 3}), ("step_n", dict(n=3, **refused)), s1, ("history", {}), ("history_stop", {}), again],
        [clear, ("history_start", {"every": 1, "capacity": CAPACITY}), ("step_n_until", {}), ("iterations", {}), ("history", {}), ("step_n_each", {}), ("history", {}),
         ("history_stop", {}), again, sn, ("poisson_solve", {})],
        [_solid("all", per_member=False), ("step_n_each", {}), ("residual", {})], [_solid("empty", per_member=True), sn],
        [_solid("seeded", per_member=False), ("poisson_solve", {}), ("poisson_solve_each", {}), ("residual", {}), ("flow_stats", {})],
        [_solid("plate", per_member=True), ("step_n_each", {}), ("residual", {}), ("poisson_solve", {})],
        [_solid("channel", per_member=True), ("poisson_solve_each", {}), ("residual", {}), s2],
        [clear, ("poisson_solve_until", {}), ("iterations", {}), again, sn], [clear, ("step_n_until", {}), ("iterations", {}), again, ("step_n_each", {})],
        [clear, ("poisson_solve_until", {}), ("iterations", {}), again, ("poisson_solve_each", {}), sn],
    ]


def _visc(nu, sweeps, **more): return ("set_viscosity", dict({"nu": nu, "sweeps": sweeps}, **more))
def _diff(nu, sweeps): return ("diffuse_velocity", {"nu": nu, "sweeps": sweeps})
def _bodies(label_kind, **more): return ("set_bodies", dict({"label_kind": label_kind}, **more))
def _loads(every, capacity=CAPACITY, **more): return ("loads_start", dict({"every": every, "capacity": capacity}, **more))


def viscous_items(subject):
    """{what it walks: item} of the subjects with viscosity and loads, hints as in planted_solids.  An item says itself what it
    needs ended in front of it (a recorder that refuses set_bodies, a history that refuses a batch's mask, a following set that
    keeps the seams away); every history_start, loads_start and record_view of a sequence stands in one of these items, so that
    no recorder of two samples is left on behind one."""
    clear, clear_nu, refused = ("clear_solids", {}), ("clear_viscosity", {}), {"_refused": True}
    no_loads, no_hist, noise = ("loads_stop", {}), ("history_stop", {}), _up("noise")
    A, B = subject.cases[0][:2], subject.cases[-1][:2]
    if subject.kind == "context":
        step, step2, step3 = ("step", {}), ("step_n", {"n": 2}), ("step_n", {"n": 3})
        solved = ("step", {"iters": 5})          # (a pressure that is not all zeros in front of a load)
        return {
            # the operator in each launch class, a reader of the velocity right behind each: the result of one launch lies in the
            # step's second buffer, of two in the third, of three in the second again -- the second two-launch call finds the
            # third buffer holding the velocity it was swapped for
            "diffusions of two, three, two and one launches at 130 x 70":
                [("upload", {"field": FV, "texture_kind": "noise", "_shape": A}), _diff(0.3, 9), ("advect_velocity", {}), _diff(0.05, 17), step, _diff(2.5, 9),
                 ("calculate_divergence", {}), _diff(0.3, 1), ("advance_tracers", {}), step2],
            "diffusions of three, two, two and one launches at 61 x 81":
                [("upload", {"field": FV, "texture_kind": "noise", "_shape": B}), _diff(2.5, 17), step, _diff(0.3, 9), ("advance_tracers", {}), _diff(0.05, 9),
                 ("advect_velocity", {}), _diff(0.3, 1), ("calculate_divergence", {}), step2],
            # a viscosity of two launches in force: no mask, a mask set behind it, the mask cleared while it stays; a history samples
            "a viscosity in force while masks come and go":
                [clear, noise, ("history_start", {"every": 2, "capacity": CAPACITY}), _visc(0.3, 9), step, step2, _solid("disc"), step, step2, clear, step, step2,
                 ("history", {})],
            # cleared: each plain path again.  The seams (every condition set in front) with a loads recorder on: zero records
            "cleared at 130 x 70: the step seams, and samples without solids inside their loop":
                [("forget_forces", {"_shape": A}), no_hist, ("set_tracers", {"follow": False}), clear, _opt("OPT_ADVECT_KERNEL", 2), _loads(1), _visc(0.05, 8), step2,
                 clear_nu, step3, ("loads_history", {})],
            "cleared at 61 x 81: the one-launch step of a small grid":
                [_opt("OPT_SOR_KERNEL", 0, _shape=B), _opt("OPT_SOR_FUSE", 0), _opt("OPT_ADVECT_KERNEL", 0), _opt("OPT_SMALL_GRID", 1), clear, _visc(0.3, 1), step,
                 clear_nu, step, step2],
            "cleared with OPT_FUSE_PROJECTION = 0":
                [_opt("OPT_ADVECT_KERNEL", 1), _opt("OPT_FUSE_DIVERGENCE", 0), _opt("OPT_FUSE_PROJECTION", 0), _visc(0.3, 3), step, clear_nu, step, step2, _opt("OPT_FUSE_DIVERGENCE", 1),
                 _opt("OPT_FUSE_PROJECTION", 1)],
            "cleared with a mask still set": [_solid("plate"), _visc(2.5, 9), step2, clear_nu, step, ("flow_stats", {})],
            "the solver's options in front of a solve":
                [_opt("OPT_SOR_KERNEL", 1), ("poisson_solve", {}), _opt("OPT_SOR_KERNEL", 2), _opt("OPT_SOR_FUSE", 2), ("poisson_continue", {}), _opt("OPT_SOR_FUSE", 16),
                 ("poisson_solve_until", {})],
            # (the switch the seams depend on is only off inside its own item)
            "a viscous step_n with the seams switched off": [_opt("OPT_STEP_SEAMS", 0), _visc(0.05, 3), step2, _opt("OPT_STEP_SEAMS", 1)],
            # the companions of a step, all at once under a viscosity and a mask; the recorder spans three calls that leave remainders
            "a history, a trail and a loads recorder under a viscosity and a mask":
                [no_loads, ("clear_bodies", {}), noise, ("set_tracers", {"follow": True}), ("trail_start", {}), ("history_start", {"every": 1, "capacity": CAPACITY}), _solid("disc"),
                 _bodies("halves"), _loads(2), _visc(0.3, 3), solved, step2, step3, ("history", {}), ("trail", {}), ("loads_history", {}), ("loads", {})],
            "labels before the mask, a mask replaced and cleared under labels, labels replaced and reset":
                [clear, no_loads, _bodies("sixteen"), _solid("disc"), solved, ("loads", {}), _solid("seeded"), ("loads", {}), clear, ("loads", {}),
                 _bodies("with zeros"), _solid("channel"), solved, ("loads", {}), ("clear_bodies", {}), ("loads", {}), ("bodies", {})],
            "a loads recorder across calls that leave remainders, restarted while on":
                [_solid("isolated"), _loads(3), step2, solved, step2, ("loads_history", {}), _loads(2), step, step2, ("loads_history", {})],
            "set_bodies, refused while the recorder is on": [_loads(1), _bodies("halves", **refused), step, ("bodies", {}), no_loads, ("clear_bodies", {})],
            # three admission checks in a row: the third refuses, and the two counters in front of it and every field stay
            "a full loads recorder refuses the call whole, a history and a trail on":
                [("set_tracers", {"follow": True}), ("trail_start", {}), ("history_start", {"every": 1, "capacity": CAPACITY}), _loads(1, 2),
                 ("step_n", dict(n=3, **refused)), ("history", {}), ("trail", {}), ("loads_history", {}), no_loads, step, no_hist],
        }
    s1, s2, sn, each = ("step_n", {"n": 1}), ("step_n", {"n": 2}), ("step_n", {}), ("step_n_each", {})
    solved, whole = ("step_n", {"n": 1, "iters": 5}), {"first": 0, "count": subject.batch}
    return {
        # the coefficient table staged through its two slots by calls queued back to back: nothing is read in between
        "four step calls back to back under a per-member nu, one member at 0":
            [no_hist, noise, ("history_start", dict(every=2, capacity=CAPACITY, **whole)), _visc([0.3, 0.0, 2.5], 3, per_member=True), sn, each, sn, each,
             ("download", {"field": FV}), ("history", {}), no_hist],
        "three step calls back to back under a per-member nu and a mask":
            [no_hist, ("record_start", {}), ("record_view", {"what": 2}), _solid("plate", per_member=False), _visc([0.0, 0.05, 0.3], 10, per_member=True), each, sn, each, ("residual", {})],
        "a per-member nu replaced by a shared one":
            [_visc([2.5, 0.0, 0.05], 3, per_member=True), sn, _visc(0.3, 1, per_member=False), each, ("residual", {}), ("viscosity", {})],
        # cleared: the calls that are refused or switched off while a viscosity is set -- the step to a tolerance and the replay
        # of a timeline in one launch (a record in a later step, no following set, no mask), a loads recorder counting through
        "cleared: step_n_until and the one-launch replay":
            [clear, no_hist, _visc(0.3, 3, per_member=False), sn, clear_nu, _loads(2, **whole), ("step_n_until", {}), ("iterations", {}), ("set_tracers", {"follow": False}),
             ("forget_forces", {}), ("queue_forces", {"step": 1}), ("step_n", {"n": 3}), ("loads_history", {}), s1],
        "step_n_until, refused while a viscosity is set": [clear, _visc(0.05, 1, per_member=False), ("step_n_until", dict(refused)), each, ("residual", {})],
        "a history, the recorder and a following set under a viscosity":
            [clear, ("record_start", {}), ("record_view", {"what": 1}), ("history_start", dict(every=1, capacity=CAPACITY, **whole)), ("set_tracers", {"follow": True}),
             _visc(0.3, 3, per_member=False), sn, each, ("history", {}), ("frames", {}), ("tracers", {}), no_hist],
        "a loads recorder under a per-member viscosity, mask and labels":
            [no_hist, no_loads, ("clear_bodies", {}), ("record_start", {}), _solid("disc", per_member=True), _bodies("halves", per_member=True), _loads(2, **whole),
             _visc([0.3, 0.0, 0.05], 3, per_member=True), solved, s2, ("step_n_each", {"n": 3}), ("loads_history", {}), ("loads", dict(whole))],
        "labels before the mask, a mask replaced and cleared under labels, labels replaced and reset":
            [clear, no_hist, no_loads, _bodies("sixteen", per_member=False), _solid("disc", per_member=False), solved, ("loads", dict(whole)),
             _solid("seeded", per_member=True), ("loads", dict(whole)), clear, ("loads", dict(whole)), _bodies("with zeros", per_member=True), _solid("channel"), solved,
             ("loads", dict(whole)), ("clear_bodies", {}), ("loads", dict(whole)), ("bodies", {})],
        "a loads recorder across calls that leave remainders, restarted while on":
            [no_hist, _solid("isolated", per_member=False), _loads(3), s2, solved, ("step_n_each", {"n": 2}), ("loads_history", {}), _loads(2), s1, s2, ("loads_history", {})],
        "set_bodies, refused while the recorder is on": [_loads(1), _bodies("halves", **refused), sn, ("bodies", {}), no_loads, ("clear_bodies", {})],
        # four admission checks in a row (frames, trail, history, loads): the last refuses, and the counters in front of it stay
        "a full loads recorder refuses the call whole, a history and the recorder on":
            [clear, ("record_start", {}), ("record_view", {"what": 0}), ("history_start", dict(every=1, capacity=CAPACITY, **whole)), _loads(1, 2, **whole), ("step_n", dict(n=3, **refused)), ("history", {}),
             ("frames", {}), ("loads_history", {}), no_loads, s1, no_hist],
        # (the calls to a tolerance need the mask and the viscosity gone: they stand in items that say so)
        "cleared: a solve to a tolerance, then a viscosity again": [clear, clear_nu, ("poisson_solve_until", {}), ("iterations", {}), ("set_viscosity", {}), sn],
        "cleared: a step to a tolerance, then a viscosity again": [clear, clear_nu, ("step_n_until", {}), ("iterations", {}), ("set_viscosity", {}), each],
        "cleared: a solve to a tolerance": [clear, clear_nu, ("poisson_solve_until", {}), ("iterations", {}), sn],
        "cleared: a solve to a tolerance behind a step call": [clear, clear_nu, sn, ("poisson_solve_until", {}), ("iterations", {})],
    }


def _fr(every, capacity=CAPACITY, **more): return ("friction_start", dict({"every": every, "capacity": capacity}, **more))
def _tq(every, capacity=CAPACITY, **more): return ("torque_start", dict({"every": every, "capacity": capacity}, **more))
def _mean(what, every, **more): return ("mean_start", dict({"what": what, "every": every}, **more))
def _piv(pivot_kind, **more): return ("set_body_pivots", dict({"pivot_kind": pivot_kind}, **more))
def _open(open_kind, **more): return ("set_openings", dict({"open_kind": open_kind}, **more))


def record_items(subject):
    """{what it walks: item} of the subjects with friction, torque and averages, hints as in planted_solids ("_wrong": pivots of
    another number of bodies, "_outside": a plane outside `what`).  An item says itself what it needs ended in front of it; every
    recorder of two samples is stopped inside the item that started it."""
    clear, clear_nu, refused = ("clear_solids", {}), ("clear_viscosity", {}), {"_refused": True}
    no_loads, no_fr, no_tq, no_hist, noise = ("loads_stop", {}), ("friction_stop", {}), ("torque_stop", {}), ("history_stop", {}), _up("noise")
    stop3 = [no_loads, no_fr, no_tq]
    reads = [("friction_history", {}), ("torque_history", {}), ("mean_info", {}), ("mean_sums", {})]
    A, B = subject.cases[0][:2], subject.cases[-1][:2]
    if subject.kind == "context":
        step, step2, step3 = ("step", {}), ("step_n", {"n": 2}), ("step_n", {"n": 3})
        solved = ("step", {"iters": 5})          # (a pressure that is not all zeros in front of a torque)
        seam = [("forget_forces", {"_shape": A}), no_hist, ("set_tracers", {"follow": False}), clear, clear_nu, _opt("OPT_ADVECT_KERNEL", 2)]
        return {
            # five counters with five periods over 10 steps in four calls: samples 10, 5, 3, 2 and 2, remainders in every call
            "a history, the loads, the friction, the torque and the averages on at once, each with its own every, behind viscous steps":
                stop3 + [noise, ("history_start", {"every": 1, "capacity": CAPACITY}), _solid("disc"), _bodies("halves"), _piv("seeded"), _loads(2), _fr(3), _tq(4),
                         _mean(15, 5), _visc(0.3, 3), solved, step2, step3, ("step_n", {"n": 4}), ("history", {}), ("loads_history", {})] + reads + [no_hist],
            "a full friction recorder refuses the call whole while the others have room":
                [("history_start", {"every": 1, "capacity": CAPACITY}), _loads(1), _tq(1), _mean(3, 1), _fr(1, 2), ("step_n", dict(n=3, **refused)), step2, ("history", {}),
                 ("loads_history", {})] + reads + [no_fr, no_hist],
            "a full torque recorder refuses the call whole while the others have room":
                [("history_start", {"every": 1, "capacity": CAPACITY}), _loads(1), _fr(1), _mean(12, 1), _tq(1, 2), ("step_n", dict(n=3, **refused)), step2, ("history", {}),
                 ("loads_history", {})] + reads + [no_tq, no_hist],
            "the friction recorder across calls that leave remainders, restarted while on":
                [_solid("isolated"), _loads(1), step, _fr(3), step2, solved, step2, ("friction_history", {}), _fr(2), step, step2, ("friction_history", {})],
            "the torque recorder across calls that leave remainders, restarted while on":
                [_solid("plate"), _tq(3), step2, solved, step2, ("torque_history", {}), _tq(2), step, step2, ("torque_history", {})],
            "the averages restarted while on: the sums and the counts start from zero":
                [_mean(3, 1), step2, ("mean_sample", {}), ("mean_info", {}), _mean(3, 2), step, step2, ("mean_info", {}), ("mean_sums", {})],
            "set_bodies and clear_bodies, refused while the friction recorder is on":
                [no_loads, no_tq, _fr(1), _bodies("halves", **refused), step, ("clear_bodies", dict(refused)), step, ("bodies", {}), no_fr],
            "set_bodies and clear_bodies, refused while the torque recorder is on":
                [no_loads, no_fr, _tq(1), _bodies("sixteen", **refused), step, ("clear_bodies", dict(refused)), step, ("bodies", {}), no_tq],
            "the same number of bodies keeps the pivots, another puts them back to zero":
                stop3 + [_solid("disc"), _bodies("with zeros", seed=1), _piv("seeded"), ("body_pivots", {}), _bodies("with zeros", seed=2), ("body_pivots", {}), solved,
                         ("torque", {}), _bodies("sixteen"), ("body_pivots", {}), ("torque", {}), _bodies("with zeros", seed=3), ("body_pivots", {}), ("torque", {}), _piv("centre"),
                         ("clear_bodies", {}), ("body_pivots", {})],
            "pivots set while the torque recorder is on hold from the next sample":
                [_solid("plate"), _tq(1), _piv("seeded", seed=1), solved, _piv("seeded", seed=2), step, ("torque_history", {}), _piv(None), step, ("torque_history", {})],
            "set_body_pivots with another number of bodies, refused: the pivots stay":
                [_piv("centre"), _piv("seeded", _wrong=True, **refused), step, ("body_pivots", {})],
            "samples under a mask that is replaced and cleared while recording":
                [_fr(1), _tq(1), _mean(15, 1), _solid("disc"), solved, _solid("seeded"), step, clear, step] + reads[:2] + reads[3:],
            # the seam shape with every condition of the seam in front: with every >= 1 step_n runs without its fused boundaries,
            # stopped it takes them again; with every == 0 it keeps them and mean_sample adds between the calls
            "averages with every >= 1 on the seam shape, then stopped: the seams again":
                seam + [_mean(7, 1), step2, ("mean_sums", {}), ("mean_stop", {}), step2, ("mean_info", {})],
            "averages with every == 0 on the seam shape: mean_sample between fused calls":
                seam + [_mean(9, 0), step2, ("mean_sample", {}), step3, ("mean_sample", {}), ("mean_info", {}), ("mean_sums", {})],
            "a plane outside what, refused": [_mean(1, 1), step, ("mean_sums", dict(_outside=True, **refused)), step, ("mean_sums", {})],
            # (the switches the seams depend on are only off inside their own items)
            "the switches of the fused step off and on again":
                [_opt("OPT_ADVECT_KERNEL", 1), _opt("OPT_FUSE_DIVERGENCE", 0), _opt("OPT_FUSE_PROJECTION", 0), step, _opt("OPT_FUSE_DIVERGENCE", 1), _opt("OPT_FUSE_PROJECTION", 1)],
            "a step_n with the seams switched off": [_opt("OPT_STEP_SEAMS", 0), step2, _opt("OPT_STEP_SEAMS", 1)],
            "the solver's options in front of a solve":
                [_opt("OPT_SOR_KERNEL", 1), ("poisson_solve", {}), _opt("OPT_SOR_KERNEL", 2), _opt("OPT_SOR_FUSE", 2), ("poisson_continue", {}), _opt("OPT_SOR_FUSE", 16),
                 ("poisson_solve_until", {})],
        }
    s1, s2, sn, each = ("step_n", {"n": 1}), ("step_n", {"n": 2}), ("step_n", {}), ("step_n_each", {})
    solved, whole = ("step_n", {"n": 1, "iters": 5}), {"first": 0, "count": subject.batch}
    replay = [clear, clear_nu, no_hist, ("record_stop", {}), ("set_tracers", {"follow": False}), ("forget_forces", {}), ("queue_forces", {"step": 1})]      # (frames would cut it too)
    again = [("forget_forces", {}), ("queue_forces", {"step": 1})]
    return {
        # (a batch's history and its masks refuse each other: all five without a mask -- zero records but for pivot2 --, the four
        # under one below); the ranges of the five differ
        "a history, the loads, the friction, the torque and the averages on at once, each with its own every and its own range, behind viscous steps":
            stop3 + [clear, noise, ("history_start", dict(every=1, capacity=CAPACITY, **whole)), _bodies("halves", per_member=True), _piv("seeded", per_member=True),
                     _loads(2, **whole), _fr(3, first=1, count=2), _tq(4, first=0, count=1), _mean(15, 5, first=1, count=1), _visc([0.3, 0.0, 0.05], 3, per_member=True),
                     solved, s2, ("step_n_each", {"n": 3}), ("step_n", {"n": 4}), ("history", {}), ("loads_history", {})] + reads + [no_hist],
        "the four recorders under a per-member mask, labels, pivots and viscosity":
            stop3 + [no_hist, _solid("disc", per_member=True), _bodies("halves", per_member=True), _piv("seeded", per_member=True), _loads(1, first=0, count=2),
                     _fr(2, first=1, count=2), _tq(1, first=2, count=1), _mean(15, 2, first=0, count=2), _visc([0.3, 0.0, 0.05], 3, per_member=True), solved, s2,
                     ("step_n_each", {"n": 3}), ("loads_history", {})] + reads,
        "a full friction recorder refuses the call whole while the others have room":
            [clear, ("record_start", {}), ("history_start", dict(every=1, capacity=CAPACITY, **whole)), _loads(1, **whole), _tq(1, **whole), _mean(3, 1, **whole), _fr(1, 2, **whole),
             ("step_n", dict(n=3, **refused)), s2, ("history", {}), ("frames", {}), ("loads_history", {})] + reads + [no_fr, no_hist],
        "a full torque recorder refuses the call whole while the others have room":
            [clear, ("record_start", {}), ("history_start", dict(every=1, capacity=CAPACITY, **whole)), _loads(1, **whole), _fr(1, **whole), _mean(12, 1, **whole), _tq(1, 2, **whole),
             ("step_n_each", dict(n=3, **refused)), s2, ("history", {}), ("frames", {}), ("loads_history", {})] + reads + [no_tq, no_hist],
        "the friction recorder across calls that leave remainders, restarted while on":
            [no_hist, _solid("isolated", per_member=False), _loads(1), s1, _fr(3), s2, solved, ("step_n_each", {"n": 2}), ("residual", {}), ("friction_history", {}), _fr(2), s1, s2,
             ("friction_history", {})],
        "the torque recorder across calls that leave remainders, restarted while on":
            [no_hist, _solid("plate", per_member=True), _tq(3), s2, solved, ("step_n_each", {"n": 2}), ("torque_history", {}), _tq(2), s1, s2, ("torque_history", {})],
        "the averages restarted while on: the sums and the counts start from zero":
            [_mean(3, 1, **whole), s2, ("mean_sample", {}), ("mean_info", {}), _mean(3, 2, first=1, count=2), s1, s2, ("mean_info", {}), ("mean_sums", {})],
        "set_bodies and clear_bodies, refused while the friction recorder is on":
            [no_loads, no_tq, _fr(1), _bodies("halves", **refused), sn, ("clear_bodies", dict(refused)), sn, ("bodies", {}), no_fr],
        "set_bodies and clear_bodies, refused while the torque recorder is on":
            [no_loads, no_fr, _tq(1), _bodies("sixteen", **refused), sn, ("clear_bodies", dict(refused)), sn, ("bodies", {}), no_tq],
        "the same number of bodies keeps the pivots, another puts them back to zero":
            stop3 + [no_hist, _solid("disc", per_member=False), _bodies("with zeros", seed=1, per_member=False), _piv("seeded", per_member=True), ("body_pivots", {}),
                     _bodies("with zeros", seed=2, per_member=True), ("body_pivots", {}), solved, ("torque", dict(whole)), _bodies("sixteen"), ("body_pivots", {}),
                     ("torque", dict(whole)), _bodies("with zeros", seed=3, per_member=False), ("body_pivots", {}), ("torque", dict(whole)), _piv("centre", per_member=False),
                     ("clear_bodies", {}), ("body_pivots", {})],
        "pivots set while the torque recorder is on hold from the next sample":
            [no_hist, _solid("plate", per_member=False), _tq(1, **whole), _piv("seeded", seed=1, per_member=False), solved, _piv("seeded", seed=2, per_member=True), s1,
             ("torque_history", {}), _piv(None), s1, ("torque_history", {})],
        "set_body_pivots with another number of bodies, refused: the pivots stay":
            [_piv("centre", per_member=True), _piv("seeded", _wrong=True, **refused), sn, ("body_pivots", {})],
        "samples under a mask that is replaced and cleared while recording":
            [no_hist, _fr(1, **whole), _tq(1, **whole), _mean(15, 1, **whole), _solid("disc", per_member=False), solved, _solid("seeded", per_member=True), s1, clear, s1]
            + reads[:2] + reads[3:],
        # a record in a later step, no following set, no mask, no viscosity: the one-launch replay.  With every >= 1 it is cut where
        # a sample is due inside the call, stopped it runs whole again; with every == 0 it stays whole and mean_sample adds
        "averages with every >= 1 while a timeline is pending: the replay is cut; stopped: whole again":
            replay + [_mean(7, 2, **whole), ("step_n", {"n": 3}), ("mean_info", {}), ("mean_sums", {})] + again + [("mean_stop", {}), ("step_n", {"n": 3}), ("mean_info", {})],
        "averages with every == 0 while a timeline is pending: mean_sample between one-launch replays":
            replay + [_mean(9, 0, first=1, count=2), ("step_n", {"n": 3}), ("mean_sample", {})] + again + [("step_n", {"n": 2}), ("mean_sample", {}), ("mean_info", {}),
                                                                                                         ("mean_sums", {})],
        "a plane outside what, refused": [_mean(1, 1), sn, ("mean_sums", dict(_outside=True, **refused)), sn, ("mean_sums", {})],
        # (the calls to a tolerance need the mask and the viscosity gone: they stand in items that say so)
        "cleared: a solve to a tolerance, then a viscosity again": [clear, clear_nu, ("poisson_solve_until", {}), ("iterations", {}), ("set_viscosity", {}), sn],
        "cleared: a step to a tolerance, then a viscosity again": [clear, clear_nu, ("step_n_until", {}), ("iterations", {}), ("set_viscosity", {}), each, ("residual", {})],
        "cleared: a solve to a tolerance": [clear, clear_nu, ("poisson_solve_until", {}), ("iterations", {}), sn],
        "cleared: a step to a tolerance behind a step call": [clear, clear_nu, sn, ("step_n_until", {}), ("iterations", {}), ("residual", {})],
        "cleared: the averages count through a step to a tolerance": [clear, clear_nu, _mean(12, 1), ("step_n_until", {}), ("iterations", {}), ("mean_info", {}), ("poisson_solve_until", {}), ("iterations", {})],
    }


def open_items(subject):
    """{what it walks: item} of the subjects with openings, hints as in planted_solids ("_mask" on a profile: a cell the mask of a
    later link makes solid, "_off": a record off the inflow cells, "_clear": n == 0, "_open" on queue_forces: records on an inflow,
    a profiled and an outflow cell).  Every item that sets a map clears the viscosity first: the two refuse each other."""
    clear, clear_nu, clear_open, refused = ("clear_solids", {}), ("clear_viscosity", {}), ("clear_openings", {}), {"_refused": True}
    div, no_hist, profile, flux = dict(what=VIEW_DIVERGENCE, **refused), ("history_stop", {}), ("set_inflow_profile", {}), ("openings_flux", {})
    A, B = subject.cases[0][:2], subject.cases[-1][:2]
    if subject.kind == "context":
        step, step2 = ("step", {}), ("step_n", {"n": 2})
        return {
            "a map set before the mask": [clear_nu, clear, _open("channel", inflow=[12.5, 0.0]), step2, _solid("disc"), step, ("openings", {}), flux],
            "a mask set before the map": [clear_nu, clear_open, _solid("plate"), _open("every rim cell", inflow=[-3.0, 2.5]), step2, ("openings", {}), ("flow_stats", {}), clear_open, step],
            "a mask replaced, and cleared, behind a map, a step right after each":
                [clear_nu, _open("seeded", inflow=[12.5, 0.0]), _solid("disc"), step, _solid("seeded"), step, clear, step, flux],
            "an inflow cell goes solid and comes back: the live counts move, a profile record on it is kept":
                [clear_nu, clear, _open("channel", seed=3, inflow=[12.5, 0.0]), ("set_inflow_profile", {"_mask": ("seeded", 5)}), ("openings", {}), step, _solid("seeded", seed=5),
                 ("openings", {}), step, flux, ("inflow_profile", {}), clear, ("openings", {}), step, flux],
            "set_inflow without and with a profile held, a step after each":
                [clear_nu, _open("channel", inflow=[12.5, 0.0]), ("set_inflow", {"inflow": [-3.0, 2.5]}), step, profile, ("set_inflow", {"inflow": [40.0, -7.25]}), step,
                 ("inflow_profile", {}), ("openings", {})],
            "a new map under a profile: the profile is gone": [clear_nu, _open("channel"), profile, step, _open("inflow only"), ("inflow_profile", {}), step],
            "a profile replaced and a profile cleared":
                [clear_nu, _open("every rim cell"), profile, step, profile, step, ("set_inflow_profile", {"_clear": True}), step, ("inflow_profile", {})],
            "a queued force record on an inflow cell, on a profiled cell and on an outflow cell":
                [clear_nu, ("forget_forces", {}), _open("channel"), profile, ("queue_forces", {"_open": True}), step2, ("forces_pending", {})],
            "every operator and poisson_solve_until under a map":
                [clear_nu, _open("seeded", inflow=[40.0, -7.25]), ("calculate_divergence", {}), ("poisson_solve", {}), ("poisson_continue", {}), ("subtract_gradient", {}),
                 ("poisson_solve_until", {}), ("residual", {}), ("flow_stats", {})],
            "a history, a trail and following tracers behind steps with openings":
                [clear_nu, ("set_tracers", {"follow": True}), ("trail_start", {}), ("history_start", {"every": 1, "capacity": CAPACITY}), _open("channel", inflow=[12.5, 0.0]), step,
                 step2, ("history", {}), ("trail", {}), ("tracers", {}), no_hist],
            "a history's samples under a map and a mask":
                [clear_nu, ("history_start", {"every": 2, "capacity": CAPACITY}), _open("every rim cell"), _solid("channel"), step2, ("history", {}), step, step, ("history", {}), no_hist],
            # a cleared map gives every plain path back
            "cleared at 130 x 70: the step seams":
                [("forget_forces", {"_shape": A}), no_hist, ("set_tracers", {"follow": False}), clear, clear_nu, _opt("OPT_ADVECT_KERNEL", 2), _open("channel"), step2, clear_open,
                 step2],
            "cleared at 61 x 81: the one-launch step of a small grid":
                [_opt("OPT_SOR_KERNEL", 0, _shape=B), _opt("OPT_SOR_FUSE", 0), _opt("OPT_ADVECT_KERNEL", 0), _opt("OPT_SMALL_GRID", 1), clear, clear_nu, _open("seeded"), step,
                 clear_open, step, step2],
            "cleared with the switches of the fused step off":
                [clear_nu, clear, _opt("OPT_ADVECT_KERNEL", 1), _opt("OPT_FUSE_DIVERGENCE", 0), _opt("OPT_FUSE_PROJECTION", 0), _open("every rim cell"), step, clear_open, step, step2,
                 _opt("OPT_FUSE_DIVERGENCE", 1), _opt("OPT_FUSE_PROJECTION", 1)],
            "cleared with the seams switched off": [clear_nu, _opt("OPT_STEP_SEAMS", 0), _open("channel"), step2, clear_open, step2, _opt("OPT_STEP_SEAMS", 1)],
            "the solver's options in front of a solve under a map":
                [clear_nu, _open("channel"), _opt("OPT_SOR_KERNEL", 1), ("poisson_solve", {}), _opt("OPT_SOR_KERNEL", 2), _opt("OPT_SOR_FUSE", 2), ("poisson_continue", {}),
                 _opt("OPT_SOR_FUSE", 16), ("poisson_solve_until", {})],
            "outflow only": [clear_nu, _open("outflow only"), step, flux], "a single inflow cell": [clear_nu, _open("single inflow"), step, flux],
            "a map with no opening": [clear_nu, _solid("disc"), _open("none"), step2, ("openings", {}), flux],
            "inflow only: the incompatible Neumann problem": [clear_nu, _open("inflow only", inflow=[-3.0, 2.5]), step, ("residual", {})],
            # the refusals, a step call behind each
            "set_openings, refused while a viscosity is set": [clear_open, _visc(0.3, 3), _open("channel", **refused), step, clear_nu],
            "the divergence view and set_viscosity with a nu, refused while openings are set":
                [clear_nu, _open("channel"), ("view_scalar", dict(div)), step, ("view_texels", dict(div)), step, _visc(0.3, 3, **refused), step, _visc(0.0, 3), step],
            "set_inflow and set_inflow_profile, refused without openings": [clear_open, ("set_inflow", dict(refused)), step, ("set_inflow_profile", dict(refused)), step],
            "a profile with a record off the inflow cells, refused: the profile stays":
                [clear_nu, _open("channel"), profile, ("set_inflow_profile", dict(_off=True, **refused)), step, ("inflow_profile", {})],
        }
    s1, s2, sn, each = ("step_n", {"n": 1}), ("step_n", {"n": 2}), ("step_n", {}), ("step_n_each", {})
    whole = {"first": 0, "count": subject.batch}
    flux = ("openings_flux", dict(whole))
    fresh = [clear_nu, no_hist, ("record_start", {})]                  # what refuses a batch's map, ended (a fresh recorder draws the dye)
    return {
        "a map set before the mask": fresh + [clear, _open("channel", per_member=False, inflow=[12.5, 0.0], inflow_per_member=False), s2, _solid("disc", per_member=True), s1, ("openings", {}), flux],
        "a mask set before the map": fresh + [clear_open, _solid("plate", per_member=False), _open("every rim cell", per_member=True, inflow=[-3.0, 2.5], inflow_per_member=False), s2, ("openings", {}), ("flow_stats", {}), clear_open, s1],
        "a mask replaced, and cleared, behind a map, a step right after each":
            fresh + [_open("seeded", per_member=True, inflow=[12.5, 0.0], inflow_per_member=False), _solid("disc", per_member=False), s1, _solid("seeded", per_member=True), s1, clear, s1, flux],
        "an inflow cell goes solid and comes back: the live counts move, a profile record on it is kept":
            fresh + [clear, _open("channel", seed=3, per_member=False, inflow=[12.5, 0.0], inflow_per_member=False), ("set_inflow_profile", {"_mask": ("seeded", 5)}), ("openings", {}), s1,
                     _solid("seeded", seed=5, per_member=False), ("openings", {}), s1, flux, ("inflow_profile", {}), clear, ("openings", {}), s1, flux],
        "set_inflow without and with a profile held, a step after each":
            fresh + [_open("channel", per_member=False, inflow=[12.5, 0.0], inflow_per_member=False), ("set_inflow", {"per_member": True}), s1, profile, ("set_inflow", {"per_member": False, "inflow": [40.0, -7.25]}), s1, ("inflow_profile", {}),
                     ("openings", {})],
        "a new map under a profile: the profile is gone": fresh + [_open("channel", per_member=False), profile, s1, _open("inflow only", per_member=False), ("inflow_profile", {}), s1],
        "a profile replaced and a profile cleared":
            fresh + [_open("every rim cell", per_member=False), ("set_inflow_profile", {"_members": False}), s1, ("set_inflow_profile", {"_members": True}), s1,
                     ("set_inflow_profile", {"_clear": True}), s1, ("inflow_profile", {})],
        "a queued force record on an inflow cell, on a profiled cell and on an outflow cell":
            fresh + [("forget_forces", {}), _open("channel", per_member=False), profile, ("queue_forces", {"_open": True}), s2, ("forces_pending", {})],
        "step_n_each and poisson_solve_each under per-member maps and inflows":
            fresh + [("set_tracers", {"follow": True}), _open("channel", per_member=True, inflow_per_member=True), each, ("tracers", {}), ("residual", {}), ("poisson_solve_each", {}), ("residual", {}), flux,
                     ("poisson_solve", {}), sn],
        # a cleared map gives every plain path back: the step to a tolerance, the one-launch replay of a timeline, a history
        "cleared: step_n_until, the one-launch replay and history_start":
            fresh + [clear, _open("channel"), s2, clear_open, ("poisson_solve_until", {}), ("iterations", {}), ("step_n_until", {}), ("iterations", {}), ("set_tracers", {"follow": False}), ("forget_forces", {}),
                     ("queue_forces", {"step": 1}), ("step_n", {"n": 3}), ("history_start", dict(every=1, capacity=CAPACITY, **whole)), s1, ("history", {}), no_hist],
        "cleared behind a step under a map: a step to a tolerance": fresh + [clear, _open("seeded"), sn, clear_open, ("step_n_until", {}), ("iterations", {}), ("poisson_solve_until", {}), ("iterations", {})],
        "cleared: a viscosity between two maps": [clear_open, _visc([0.05, 0.0, 0.3], 1, per_member=True), sn, clear_nu, _open("channel"), sn],
        "cleared: a history across two calls": fresh + [clear, clear_open, ("history_start", dict(every=1, capacity=CAPACITY, **whole)), s2, ("history", {}), sn, ("history", {}), no_hist],
        "outflow only": fresh + [_open("outflow only", per_member=False), s1, flux], "a single inflow cell": fresh + [_open("single inflow", per_member=False), s1, flux],
        "a map with no opening": fresh + [_solid("disc", per_member=False), _open("none", per_member=False), s2, ("openings", {}), flux],
        "inflow only: the incompatible Neumann problem": fresh + [_open("inflow only", per_member=False, inflow=[-3.0, 2.5], inflow_per_member=False), each, ("residual", {})],
        # the refusals, a step call behind each
        "set_openings, refused while a history is on":
            [clear, clear_open, clear_nu, ("history_start", dict(every=1, capacity=CAPACITY, **whole)), _open("channel", **refused), sn, no_hist],
        "set_openings, refused while the recorder draws the divergence view":
            [clear, clear_open, clear_nu, ("record_start", {}), ("record_view", {"what": VIEW_DIVERGENCE}), _open("channel", **refused), sn, ("record_view", {"what": None})],
        "set_openings, refused while a viscosity is set": [clear_open, _visc(0.3, 3, per_member=False), _open("channel", **refused), sn, clear_nu],
        "the calls to a tolerance, history_start, the divergence view and set_viscosity, refused while openings are set":
            fresh + [clear, ("record_start", {}), _open("channel"), ("step_n_until", dict(refused)), sn, ("poisson_solve_until", dict(refused)), sn, ("history_start", dict(refused)), sn,
                     ("record_view", dict(div)), sn, ("view_render_members", dict(div)), sn, _visc(0.3, 3, per_member=False, **refused), sn],
        "set_inflow and set_inflow_profile, refused without openings": [clear_open, ("set_inflow", dict(refused)), sn, ("set_inflow_profile", dict(refused)), sn],
        "a profile with a record off the inflow cells, refused: the profile stays":
            fresh + [_open("channel", per_member=False), profile, ("set_inflow_profile", dict(_off=True, **refused)), sn, ("inflow_profile", {})],
    }


def items_of(subject):
    return record_items(subject) if subject.records else open_items(subject) if subject.opens else viscous_items(subject)


def planted_viscous(subject):
    return list(items_of(subject).values())


def viscous_handovers(subject):
    """The items as chains for has_handover: the fixed arguments without the hints."""
    return {what: [_link(kind, **{k: v for k, v in fixed.items() if not k.startswith("_")}) for kind, fixed in item]
            for what, item in items_of(subject).items()}


def _prologue(subject, index):
    """What every sequence starts with: fields and a tracer set with a trail; a batch a recording and an envelope."""
    common = [_up(("noise", "still", "fast", "whole-cell", "noise", "fast")[index % 6]), ("upload", {"field": FC})]
    if subject.kind == "slabs":
        return common
    common.append(("set_tracers", {"follow": False}))
    return common + ([("trail_start", {})] if subject.kind == "context" else [("record_start", {}), ("envelope", {})])


def _epilogue(subject):
    """What every sequence of the viscous subjects ends with: a velocity that is not still, a mask with solid and fluid cells, a
    viscosity, a step that diffuses and solves, and the loads of the pressure it left -- so that no sequence compares only loads
    without a face or without a force, or steps without a diffusion that changes a bit."""
    whole = {"first": 0, "count": subject.batch}
    if subject.opens:
        # ... of the subjects with openings: a channel with every rim cell live, a profile on it, a step that solves and the flux
        # it leaves -- so that no sequence steps only under maps without a live cell, or compares only empty flux records
        front = [("clear_viscosity", {}), _up("noise"), ("clear_solids", {})]
        if subject.kind == "context":
            return front + [_open("channel", inflow=[12.5, 0.0]), ("set_inflow_profile", {}), ("step", {"iters": 5}), ("openings_flux", {})]
        return [("history_stop", {}), ("record_start", {})] + front + [_open("channel", inflow=[12.5, 0.0], per_member=False, inflow_per_member=False), ("set_inflow_profile", {}),
                                                                        ("step_n", {"n": 1, "iters": 5}), ("openings_flux", dict(whole))]
    if not subject.viscous:
        return []
    if subject.records:
        # ... of the subjects with the three recorders: pivots away from (0, 0), averages of every group, two steps under a mask and
        # a viscosity, and the friction, the torque and a plane of two samples they leave
        if subject.kind == "context":
            return [_up("noise"), ("set_solids", {}), _piv("seeded"), _mean(15, 1), _visc(0.3, 3), ("step_n", {"n": 2, "iters": 5}), ("friction", {}), ("torque", {}), ("mean_sums", {})]
        return [("history_stop", {}), _up("noise"), ("set_solids", {}), _piv("seeded", per_member=True), _mean(15, 1, **whole), _visc([0.3, 0.0, 0.05], 3, per_member=True),
                ("step_n", {"n": 2, "iters": 5}), ("friction", dict(whole)), ("torque", dict(whole)), ("mean_sums", {})]
    if subject.kind == "context":
        return [_up("noise"), ("set_solids", {}), _visc(0.3, 3), ("step", {"iters": 5}), ("loads", {})]
    return [("history_stop", {}), _up("noise"), ("set_solids", {}), _visc([0.3, 0.0, 0.05], 3, per_member=True), ("step_n", {"n": 1, "iters": 5}),
            ("loads", {"first": 0, "count": subject.batch})]


NEEDS = {"trail": "trail", "frames": "rec", "record_view": "rec", "residual": "norms", "iterations": "iters", "history": "hist",
         "loads_history": "loads"}


def _state_after(kind, fixed, st, batch):
    """What the op of `kind` ends: the names of NEEDS that are gone behind it."""
    before = dict(st)
    if kind == "trail_start": st["trail"] = True
    if kind in ("trail_stop", "set_tracers"): st["trail"] = False
    if kind == "record_start": st["rec"] = True
    if kind == "record_stop": st["rec"] = False
    if kind == "history_start": st["hist"] = True
    if kind == "history_stop": st["hist"] = False
    if kind == "loads_start": st["loads"] = True
    if kind == "loads_stop": st["loads"] = False
    if batch:
        if kind in ("step_n", "poisson_solve") or (kind == "upload" and fixed.get("field") in (FD, FP)): st["norms"] = st["iters"] = False
        if kind in ("step_n_each", "poisson_solve_each"): st["norms"], st["iters"] = True, False
        if kind in ("step_n_until", "poisson_solve_until"): st["norms"] = st["iters"] = True
    return [name for name in st if before.get(name) and not st[name]]


def _settle(subject, index, items):
    """The sequence's items in an order in which every op is valid: a query that comes when what it reads is gone (a trail,
    a recording, a report) moves in front of the item that ended it -- the last moment it can be asked."""
    batch = subject.kind == "batch"
    st = {"trail": True, "rec": True, "norms": not batch, "iters": False, "hist": False, "loads": False}      # (behind the prologue)
    out, ended_by = [], {}                       # ended_by: name -> the item (its position in out) that ended it
    for item in items:
        if len(item) == 1 and item[0][0] in NEEDS and not st[NEEDS[item[0][0]]] and NEEDS[item[0][0]] in ended_by:
            at = ended_by[NEEDS[item[0][0]]]
            out.insert(at, item)
            ended_by = {n: (k + 1 if k >= at else k) for n, k in ended_by.items()}
            continue
        out.append(item)
        for kind, fixed in item:
            for name in _state_after(kind, fixed, st, batch):
                ended_by.setdefault(name, len(out) - 1)
            for name in [n for n in ended_by if st[n]]:
                del ended_by[name]
    return [link for item in out for link in item]


def _under_masks(items):
    def leaves(item):           # True: the item leaves a mask set, False: it leaves none, None: it leaves what it found
        ends = [kind == "set_solids" for kind, fixed in item if kind in ("set_solids", "clear_solids") and not fixed.get("_refused")]
        return ends[-1] if ends else None
    setters, clearers, others = ([item for item in items if leaves(item) is which] for which in (True, False, None))
    if not setters:             # (no item of the sequence leaves a mask set: nothing to stand behind)
        return items
    part = lambda group, at: group[at * len(group) // len(setters):(at + 1) * len(group) // len(setters)]
    return [x for at, item in enumerate(setters) for x in [item] + part(others, at) + part(clearers, at)]


def plan(subject):
    """Which kinds every case's sequence holds, in order: [[(kind, fixed arguments)]] -- a seeded permutation of a deck that
    has every kind three times, every value of every option in front of a writer, every texture and every hand-over; what
    room is left goes to writers."""
    rng = np.random.default_rng([len(subject.name), subject.cases[0][2]])
    batch = subject.kind == "batch"
    items = planted(subject)
    starts = [_prologue(subject, k) for k in range(len(subject.cases))]
    have, set_already, textures = {}, set(), set()
    for kind, fixed in [link for item in items + starts for link in item]:
        have[kind] = have.get(kind, 0) + 1
        if kind == "set_option": set_already.add((fixed["name"], fixed["value"]))
        if kind == "upload" and fixed.get("field") == FV: textures.add(fixed["texture_kind"])
    items += [[_opt(name, value)] for name, values in subject.option_values().items() for value in values if (name, value) not in set_already]
    items += [[_up(t)] for t in TEXTURES if t not in textures]
    for item in items:
        if len(item) == 1 and item[0][0] in ("set_option", "upload"): have[item[0][0]] = have.get(item[0][0], 0) + 1
    for kind in subject.kinds():
        items += [[(kind, {})] for _ in range(max(0, 3 - have.get(kind, 0)))]
    ends = [_epilogue(subject) for _ in starts]
    room = [subject.length - len(p) - len(e) for p, e in zip(starts, ends)]
    dealt = [[] for _ in starts]
    order = sorted(rng.permutation(len(items)), key=lambda at: -len(items[at]))   # (stable: the long items first, so that they fit)
    # with the fused step boundaries: the items that reach it go round first, one to every sequence
    seam = [at for at in order if subject.still_solves and any(k == "step_n" and f.get("n", 0) >= 2 for k, f in items[at])
            and ("set_option", {"name": "OPT_STEP_SEAMS", "value": 0}) not in items[at]]
    order = seam + [at for at in order if at not in seam]
    for turn, at in enumerate(order):                   # to the sequence with the most room left
        k = turn % len(room) if turn < len(seam) else int(np.argmax(room))
        shape = items[at][0][1].get("_shape")           # (an item for one shape of the subject's: to the roomiest case of that shape)
        if shape is not None:
            k = max((c for c in range(len(room)) if subject.cases[c][:2] == shape), key=lambda c: room[c])
        assert room[k] >= len(items[at]), f"{subject.name}: the deck does not fit {len(subject.cases)} sequences of {subject.length}"
        dealt[k].append([(kind, dict(fixed)) for kind, fixed in items[at]])
        room[k] -= len(items[at])
    writers = [k for k in subject.kinds() if k not in QUERIES and k not in ("set_option", "forget_forces", "trail_stop", "record_stop", "clear_solids", "history_stop", "clear_viscosity",
                                                                   "clear_bodies", "loads_stop", "friction_stop", "torque_stop", "mean_stop", "clear_openings") and
               not (subject.still_solves and k == "set_tracers") and not (subject.opens and k == "set_viscosity")]      # (a viscosity would end the map)
    plans = []
    for k, mine in enumerate(dealt):
        mine += [[(writers[int(rng.integers(len(writers)))], {})] for _ in range(room[k])]
        # the planted items anywhere in the sequence, not in front, and the reads spread evenly between the items that write
        mine = [mine[at] for at in rng.permutation(len(mine))]
        if subject.solids:      # most of a sequence runs under a mask: the items that neither set nor clear one stand behind those that leave one set
            mine = _under_masks(mine)
        loud = [item for item in mine if any(kind not in QUERIES and kind != "set_option" for kind, _ in item)]
        quiet = [item for item in mine if item not in loud]
        mine = [x for at, item in enumerate(loud) for x in [item] + quiet[at * len(quiet) // len(loud):(at + 1) * len(quiet) // len(loud)]]
        for item in mine:
            for kind, fixed in item:
                if kind == "upload" and "field" not in fixed: fixed["field"] = int(rng.integers(4))
        plans.append(starts[k] + _settle(subject, k, mine) + ends[k])
    return plans


OPTION_DEFAULTS = {"OPT_ADVECT_KERNEL": 0, "OPT_FUSE_DIVERGENCE": 1, "OPT_FUSE_PROJECTION": 1, "OPT_STEP_SEAMS": 1, "OPT_SMALL_GRID": 1,
                   "OPT_SOR_KERNEL": 0, "OPT_SOR_FUSE": 0, "OPT_ADVECT_HALO": 0, "OPT_SOR_HALO": 0}
STEPS = ("step", "step_n", "step_n_each", "step_n_until")
SOLVES = ("poisson_solve", "poisson_continue", "poisson_solve_until") + STEPS
AFFECTS = {"OPT_ADVECT_KERNEL": ("advect_velocity", "advect_color", "calculate_divergence", "subtract_gradient") + STEPS,
           "OPT_FUSE_DIVERGENCE": STEPS, "OPT_FUSE_PROJECTION": STEPS, "OPT_STEP_SEAMS": ("step_n",), "OPT_SMALL_GRID": SOLVES,
           "OPT_SOR_KERNEL": SOLVES, "OPT_SOR_FUSE": SOLVES, "OPT_SOR_HALO": SOLVES, "OPT_ADVECT_HALO": ("advect_velocity", "advect_color") + STEPS}


def option_applies(subject, name):
    """Whether the option changes the path of any call on the subject (the one-workgroup path needs at most 6144 cells, the
    fused step boundary a whole-domain context, the halos a slab)."""
    if name == "OPT_SMALL_GRID": return subject.name == "one-workgroup"
    if name == "OPT_STEP_SEAMS": return subject.kind == "context"
    return True


def path_states(ops):
    """For the census: (index, op, state in force WHILE the op runs) -- the option block, whether a set follows, the texture
    the velocity is still on the lattice of (None otherwise), whether a step call has run, the steps of the timeline that
    hold records -- followed from the op list alone."""
    options, follow, lattice, stepped, pending = dict(OPTION_DEFAULTS), False, None, False, set()
    for k, (kind, a) in enumerate(ops):
        yield k, (kind, a), {"options": dict(options), "follow": follow, "lattice": lattice, "stepped": stepped, "pending": set(pending)}
        if kind == "set_option": options[a["name"]] = a["value"]
        if kind == "set_tracers": follow = a["follow"]
        if kind == "upload" and a["field"] == FV: lattice = a["texture_kind"] if a["texture_kind"] in ("landing", "whole-cell") else None
        if kind in ("subtract_gradient", "queue_forces", "queue_drags"): lattice = None
        if kind in ("advect_velocity",) + STEPS and a["dt"] != 0.25: lattice = None
        if kind in STEPS and a["iters"] != 0: lattice = None
        if kind in ("queue_forces", "queue_drags"): pending.add(a["step"])
        if kind == "forget_forces": pending = set()
        if kind in STEPS:
            stepped, n = True, a.get("n", 1)
            pending = {step - n for step in pending if step >= n}


def on_small_grid(state):
    o = state["options"]
    return o["OPT_SMALL_GRID"] == 1 and o["OPT_SOR_KERNEL"] == o["OPT_SOR_FUSE"] == o["OPT_ADVECT_KERNEL"] == 0


def takes_the_seam(op, state):
    """sfl_step_n joins its steps by the fused kernel: n >= 2, the four switches on, the tiled kernels, no following set, no
    record in its steps."""
    (kind, a), o = op, state["options"]
    return (kind == "step_n" and a["n"] >= 2 and o["OPT_STEP_SEAMS"] == o["OPT_FUSE_DIVERGENCE"] == o["OPT_FUSE_PROJECTION"] == 1 and
            o["OPT_ADVECT_KERNEL"] != 1 and not state["follow"] and not any(step < a["n"] for step in state["pending"]))


def generate(subject, oracle):
    """{case: ops}: the subject's sequences.  Deterministic: the same lists on every machine."""
    out = {}
    for case, kinds in zip(subject.cases, plan(subject)):
        draw = _Draw(subject, case, oracle)
        out[case] = [draw.make(kind, **fixed) for kind, fixed in kinds]
        assert len(out[case]) == subject.length
    return out


# ---- the runner ------------------------------------------------------------------------------------------------------
MODES = ("eager", "lazy", "probing")


def _probe(model, seed, k):
    rng = np.random.default_rng([seed, k, 11])
    candidates = model.queries(rng)
    return candidates[int(rng.integers(len(candidates)))]


def _ask(model, handle, query, what):
    handle.peer = model
    compare(handle.apply(query), model.apply(query), what)


def replay(model, handle, ops, mode, seed=0, label="", check_finite=False):
    """Apply ops to the model and to the handle and compare: `eager` after every op all four fields and the tracers, `lazy`
    nothing before the last op, `probing` after every op one query chosen by the seed; at the end everything, in every
    mode.  An op that is a query is checked when issued (lazy skips it)."""
    assert mode in MODES
    k, op = -1, None
    try:
        for k, op in enumerate(ops):
            if op[0] in QUERIES:
                if mode != "lazy":
                    _ask(model, handle, op, f"query {op[0]}")
                continue
            want, got = model.apply(op), handle.apply(op)
            if want is not None or got is not None:      # (a refusal on one side only is a disagreement)
                compare({} if got is None else got, {} if want is None else want, f"what {op[0]} returned")
            if check_finite:
                assert model.finite(), "the model holds a NaN or an Inf"
            if mode == "eager":
                compare(handle.snapshot(), model.snapshot(), "fields after the op")
            elif mode == "probing":
                query = _probe(model, seed, k)
                _ask(model, handle, query, f"probe {query!r}")
        k, op = len(ops), ("the final comparison", {})
        compare(handle.snapshot(), model.snapshot(), "fields at the end")
        for query in model.queries(np.random.default_rng([seed, 13])):
            _ask(model, handle, query, f"at the end, {query!r}")
    except AssertionError as e:
        raise AssertionError(f"{label} seed {seed}, mode {mode}: op {k} ({op[0]}) disagrees: {e}\n"
                             f"replay(model, handle, ops, {mode!r}, seed={seed}) with ops =\n{list(ops[:k + 1])!r}") from None


def run(subject, case, ops, mode, oracle, make_handle, check_finite=False):
    """One sequence on a fresh model and a fresh handle (make_handle(subject, case))."""
    model, handle = subject.model(oracle, case), make_handle(subject, case)
    try:
        replay(model, handle, ops, mode, seed=case[2], label=f"{subject.name} {case[0]} x {case[1]}", check_finite=check_finite)
    finally:
        handle.close()


# ---- three models with one planted fault each: what a state bug looks like to the runner -----------------------------
# Each fault needs HISTORY on the handle: the first call of the faulty method on a fresh handle is right.
class ContinuesFromTheOldPressure(ContextModel):
    """Once a solve or a step has written the pressure, poisson_continue behind an upload of the pressure goes on from the
    pressure held before that upload (a stale 'the solver's own pressure is current' flag)."""
    solved, stale = False, None

    def apply(self, op):
        kind = op[0]
        if kind == "upload" and op[1]["field"] == FP and self.solved:
            self.stale = self.p
        if kind == "poisson_continue" and self.stale is not None and op[1]["iters"] > 0:
            self.p = self.stale
        out = super().apply(op)
        if kind in SOLVES:
            self.solved, self.stale = True, None
        return out


class TimelineStaysAfterStepN(ContextModel):
    """On a handle that has stepped before, step_n consumes its records but does not move the later ones down."""
    stepped = False

    def do_step(self, dt, dx, iters, omega):
        super().do_step(dt, dx, iters, omega)
        self.stepped = True

    def do_step_n(self, n, dt, dx, iters, omega):
        later = {s: r for s, r in self.timeline.items() if s >= n}
        super().do_step_n(n, dt, dx, iters, omega)
        if self.stepped:
            self.timeline = later
        self.stepped = True


class ResidualLeavesItsTarget(ContextModel):
    """From its second call on, residual leaves p_gs in the pressure."""
    calls = 0

    def q_residual(self, dx):
        out = super().q_residual(dx)
        self.calls += 1
        if self.calls > 1:
            with np.errstate(all="ignore"):
                self.p = gs_target(self.p, self.d, dx).astype(np.float32)
        return out


STAND_INS = (ContinuesFromTheOldPressure, TimelineStaysAfterStepN, ResidualLeavesItsTarget)


# ---- three more, for the state the solids add to a context --------------------------------------------------------------
class ClearedSolidsStillWall(ContextModel):
    """The first residual or flow_stats after clear_solids still follows the mask that was cleared (a stale hook)."""
    stale = None

    def apply(self, op):
        kind = op[0]
        if kind == "clear_solids":
            self.stale = self.mask
        if kind == "set_solids":
            self.stale = None
        if kind in ("residual", "flow_stats") and self.mask is None and self.stale is not None:
            self.mask, self.stale = self.stale, None
            try:
                return super().apply(op)
            finally:
                self.mask = None
        return super().apply(op)


class SolidPressureFromThePartner(ContextModel):
    """While a mask is set, a poisson_continue of an odd number of launches leaves in the solid cells what the pressure held
    before its previous write (the ping-pong partner's contents)."""

    def __init__(self, *args):
        super().__init__(*args)
        self.held, self.partner = self.p, self.p

    def apply(self, op):
        out = super().apply(op)
        if self.p is not self.held:                     # (every op that writes the pressure replaces the array)
            before, self.held = self.held, self.p
            if op[0] == "poisson_continue" and self.mask is not None and -(-op[1]["iters"] // D_SOLID) % 2 == 1:
                self.p = self.held = np.where(self.mask, self.partner, self.p).astype(np.float32)
            self.partner = before
        return out


class ReplacedMaskIsIgnored(ContextModel):
    """set_solids while a mask is set keeps the old mask."""

    def do_set_solids(self, mask_kind, seed):
        if self.mask is None:
            super().do_set_solids(mask_kind, seed)


SOLID_STAND_INS = (ClearedSolidsStillWall, SolidPressureFromThePartner, ReplacedMaskIsIgnored)


# ---- and five for the state the viscosity and the loads add ----------------------------------------------------------------
class ThirdBufferComesBack(ContextModel):
    """After a two-launch diffuse_velocity on a handle that has made one before, the velocity is what the third buffer held
    before the call: the velocity the previous such call was given (the swap names the wrong buffer)."""
    third = None

    def do_diffuse_velocity(self, nu, dt, dx, sweeps):
        before = self.v
        super().do_diffuse_velocity(nu, dt, dx, sweeps)
        if launches_of(nu, sweeps) == 2:
            if self.third is not None:
                self.v = self.third
            self.third = before


class ClearedViscosityStillDiffuses(ContextModel):
    """The first step after clear_viscosity still diffuses where a mask is set (a stale hook in front of the solids')."""
    stale = None

    def do_clear_viscosity(self):
        self.stale = self.visc
        super().do_clear_viscosity()

    def do_set_viscosity(self, nu, sweeps):
        self.stale = None
        super().do_set_viscosity(nu, sweeps)

    def step_once(self, dt, dx, iters, omega, until=None):
        if self.visc is None and self.stale is not None and self.mask is not None:
            self.visc, self.stale = self.stale, None
            try:
                return super().step_once(dt, dx, iters, omega, until)
            finally:
                self.visc = None
        self.stale = None
        return super().step_once(dt, dx, iters, omega, until)


class _MemberOfStaleCoefficients(ContextModel):
    coefficients_of = None      # (dt, dx) the coefficients are formed from, where they are not the step's own

    def _diffuse(self, va, dt, dx):
        return super()._diffuse(va, *(self.coefficients_of or (dt, dx)))


class EachKeepsThePreviousCoefficients(BatchModel):
    """A step_n_each right behind a step_n diffuses with the a and c of that step_n (the table's other slot)."""
    previous = None

    def __init__(self, oracle, dim_x, dim_y, batch):
        super().__init__(oracle, dim_x, dim_y, batch)
        self.m = [_MemberOfStaleCoefficients(oracle, dim_x, dim_y) for _ in range(batch)]

    def apply(self, op):
        kind, a = op
        if kind == "step_n_each" and self.previous is not None and not self.refuses(kind, a):
            for m in self.m:
                m.coefficients_of = self.previous
        out = super().apply(op)
        for m in self.m:
            m.coefficients_of = None
        self.previous = (a["dt"], a["dx"]) if kind == "step_n" and out is None else None     # (any other call in between: the fault sleeps)
        return out


class LoadsCountStartsAgainEveryCall(ContextModel):
    """The loads recorder counts the steps of one call, not across calls."""

    def apply(self, op):
        if op[0] in ("step", "step_n") and self.loads is not None and not self.refuses(*op):
            self.loads["steps"] = 0
        return super().apply(op)


class LabelsCountWhereSolidAtSetBodies(ContextModel):
    """A label counts where the cell was solid when set_bodies was called, not at the time of the sample."""
    counted = None

    def _remember(self):
        held = np.zeros((self.dim_y, self.dim_x), bool) if self.mask is None else self.mask
        self.counted = np.where(held, np.uint8(1) if self.labels is None else self.labels, np.uint8(0)).astype(np.uint8)

    def do_set_bodies(self, label_kind, bodies, seed):
        super().do_set_bodies(label_kind, bodies, seed)
        self._remember()

    def do_clear_bodies(self):
        super().do_clear_bodies()
        self._remember()

    def load_records(self):
        if self.mask is None or self.counted is None:
            return super().load_records()
        return load_rule.loads(self.p, self.mask, self.counted, self.bodies)


VISCOUS_STAND_INS = (ThirdBufferComesBack, ClearedViscosityStillDiffuses, EachKeepsThePreviousCoefficients)
LOAD_STAND_INS = (LoadsCountStartsAgainEveryCall, LabelsCountWhereSolidAtSetBodies)


def stand_in_subject(cls):
    """The name of the subject whose sequences a faulty model of the viscosity or the loads is walked through."""
    return "viscous-batch" if issubclass(cls, BatchModel) else "viscous-context"


def viscous_fresh_handle_check(oracle, make_handle, dim_x=61, dim_y=81, seed=3):
    """The kind of check the direct tests of the viscosity and the loads are: a fresh handle and every new call once, in one
    fixed order -- mask, labels, recorder, viscosity, one step call, the reads; one diffusion of each launch class; cleared
    ONCE with the mask cleared too, every field uploaded again, one step."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": seed})
    solve = {"dx": 0.5, "iters": 5, "omega": 1.5}
    ops = [up(FV), up(FC), ("set_solids", {"mask_kind": "disc", "seed": 7}), ("set_bodies", {"label_kind": "halves", "bodies": 2, "seed": 1}), ("bodies", {}),
           ("loads_start", {"every": 2, "capacity": 4}), ("set_viscosity", {"nu": 0.3, "sweeps": 3}), ("viscosity", {}),
           ("step_n", dict({"n": 3, "dt": 1 / 30.0}, **solve)), ("loads", {}), ("loads_history", {}), ("loads_stop", {}), ("clear_bodies", {}), ("loads", {}),
           ("diffuse_velocity", {"nu": 0.3, "dt": 0.1, "dx": 0.5, "sweeps": 1}), ("download", {"field": FV}),
           ("diffuse_velocity", {"nu": 0.3, "dt": 0.1, "dx": 0.5, "sweeps": 9}), ("download", {"field": FV}),
           ("diffuse_velocity", {"nu": 0.3, "dt": 0.1, "dx": 0.5, "sweeps": 17}), ("download", {"field": FV}),
           ("clear_solids", {}), ("clear_viscosity", {}), ("viscosity", {}), up(FV), up(FC), up(FD), up(FP), ("step", dict({"dt": 1 / 30.0}, **solve))]
    model, handle = ContextModel(oracle, dim_x, dim_y), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            compare(got, want, f"a fresh handle, one order: {op[0]}")
    compare(handle.snapshot(), model.snapshot(), "a fresh handle, one order")


def viscous_batch_fresh_handle_check(oracle, make_handle, dim_x=7, dim_y=9, batch=3, seed=3):
    """The same for a batch: a per-member nu, one step_n, the reads, one step_n_each on other numbers, its norms; cleared once."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": seed})
    ops = [up(FV), up(FC), ("set_solids", {"mask_kind": "disc", "seed": 7, "per_member": False}),
           ("set_bodies", {"label_kind": "halves", "bodies": 2, "seed": 1, "per_member": True}), ("bodies", {}),
           ("loads_start", {"every": 2, "capacity": 4, "first": 0, "count": batch}), ("set_viscosity", {"nu": [0.3, 0.0, 2.5], "sweeps": 3, "per_member": True}),
           ("viscosity", {}), ("step_n", {"n": 3, "dt": 1 / 30.0, "dx": 0.5, "iters": 5, "omega": 1.5}), ("loads", {"first": 0, "count": batch}), ("loads_history", {}),
           ("download", {"field": FV}),
           ("step_n_each", {"n": 2, "dt": [0.1, 0.25, 1 / 30.0], "dx": [1.0, 0.5, 1.0], "iters": [3, 4, 5], "omega": [1.0, 1.5, 1.96]}), ("residual", {}),
           ("loads_stop", {}), ("clear_bodies", {}), ("clear_solids", {}), ("clear_viscosity", {}), ("viscosity", {}),
           ("step_n", {"n": 1, "dt": 1 / 30.0, "dx": 0.5, "iters": 5, "omega": 1.5})]
    model, handle = BatchModel(oracle, dim_x, dim_y, batch), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            compare(got, want, f"a fresh batch, one order: {op[0]}")
    compare(handle.snapshot(), model.snapshot(), "a fresh batch, one order")


def fresh_handle_check(oracle, make_handle, dim_x=61, dim_y=81, seed=3):
    """The kind of check the suite had: a fresh handle, one fixed order that calls everything once -- options, uploads, a
    pressure uploaded and continued (the clause of tests/test_context_until.py), its update norm, a stroke queued over the
    steps to come, step_n -- every read compared, and every field at the end."""
    ops = [("set_option", {"name": "OPT_SOR_KERNEL", "value": 2}), ("upload", {"field": FV, "texture_kind": "noise", "seed": seed}),
           ("upload", {"field": FC, "texture_kind": "noise", "seed": seed}), ("upload", {"field": FD, "texture_kind": "noise", "seed": seed}),
           ("upload", {"field": FP, "texture_kind": "noise", "seed": seed}), ("poisson_continue", {"dx": 0.5, "iters": 3, "omega": 1.5}),
           ("residual", {"dx": 0.5}), ("download", {"field": FP}),
           ("queue_forces", {"step": 0, "cells": [[3, 4]], "vels": [[20.0, -10.0]]}), ("queue_forces", {"step": 2, "cells": [[30, 40]], "vels": [[-15.0, 5.0]]}),
           ("queue_forces", {"step": 4, "cells": [[7, 7]], "vels": [[1.0, 2.0]]}),
           ("step_n", {"n": 3, "dt": 1 / 30.0, "dx": 1.0, "iters": 5, "omega": 1.96}), ("forces_pending", {}),
           ("step", {"dt": 1 / 30.0, "dx": 1.0, "iters": 5, "omega": 1.96}), ("step", {"dt": 1 / 30.0, "dx": 1.0, "iters": 5, "omega": 1.96})]
    model, handle = ContextModel(oracle, dim_x, dim_y), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            compare(got, want, f"a fresh handle, one order: {op[0]}")
    compare(handle.snapshot(), model.snapshot(), "a fresh handle, one order")


# ---- five for the state the friction, the torque and the averages add -----------------------------------------------------
class PivotsSurviveAChangeOfTheBodies(ContextModel):
    """set_bodies to another number of bodies keeps the pivots of the bodies both numbers have (no reset to (0, 0))."""

    def do_set_bodies(self, label_kind, bodies, seed):
        held = self.pivots
        super().do_set_bodies(label_kind, bodies, seed)
        if held is not None and self.pivots is None:
            self.pivots = np.zeros((self.bodies, 2), np.int32)
            self.pivots[:min(len(held), self.bodies)] = held[:self.bodies]


class NewPivotsReachBack(ContextModel):
    """set_body_pivots while the torque recorder is on writes the new pivots into the sample already taken."""

    def do_set_body_pivots(self, pivot_kind, bodies, seed):
        super().do_set_body_pivots(pivot_kind, bodies, seed)
        if self.torque is not None and self.torque["records"]:
            last = self.torque["records"][-1].copy()
            last["pivot2"] = 0 if self.pivots is None else self.pivots
            self.torque["records"][-1] = last


class FrictionSharesTheLoadsCount(ContextModel):
    """The friction recorder counts with the loads recorder's step counter while that one is on."""

    def do_friction_start(self, every, capacity):
        super().do_friction_start(every, capacity)
        if self.loads is not None:
            self.friction["steps"] = self.loads["steps"]


class MeanCountStartsAgainEveryCall(ContextModel):
    """The averages count the steps of one call, not across calls."""

    def apply(self, op):
        if op[0] in ("step", "step_n") and self.means is not None and self.means["every"] >= 1 and not self.refuses(*op):
            self.means["steps"] = 0
        return super().apply(op)


class MeanRestartKeepsTheSums(ContextModel):
    """mean_start while on zeroes the counts and keeps the sums of the planes both masks have."""

    def do_mean_start(self, what, every):
        held = self.means
        super().do_mean_start(what, every)
        if held is not None:
            self.means["sums"].update({k: a for k, a in held["sums"].items() if k in self.means["sums"]})


RECORD_STAND_INS = (PivotsSurviveAChangeOfTheBodies, NewPivotsReachBack, FrictionSharesTheLoadsCount, MeanCountStartsAgainEveryCall, MeanRestartKeepsTheSums)


# ---- and five for the state the openings and the profiles add --------------------------------------------------------------
class OldCodesBehindAMap(ContextModel):
    """A change of the mask behind a map does not form the openings' codes again: while the map stays, every call that follows
    the openings' rule, and the live counts, go by the mask that was held when the map was set."""
    coded = None

    def do_set_openings(self, open_kind, seed, inflow):
        super().do_set_openings(open_kind, seed, inflow)
        self.coded = self.mask

    def apply(self, op):
        stale = self.open is not None and op[0] in SOLVES + ("calculate_divergence", "subtract_gradient", "residual", "flow_stats", "openings", "openings_flux")
        if not stale or self.refuses(*op):
            return super().apply(op)
        held, self.mask = self.mask, self.coded
        try:
            return super().apply(op)
        finally:
            self.mask = held


class NewMapKeepsTheProfile(ContextModel):
    """A new map keeps the records of the profile that still name an inflow cell."""

    def do_set_openings(self, open_kind, seed, inflow):
        held = self.profile
        super().do_set_openings(open_kind, seed, inflow)
        self.profile = [r for r in held or [] if self.open[r[0][1], r[0][0]] == opening_rule.INFLOW] or None


class SetInflowDropsTheProfile(ContextModel):
    """A new uniform inflow drops the profile."""

    def do_set_inflow(self, inflow):
        super().do_set_inflow(inflow)
        self.profile = None


class SolidInflowRecordIsForgotten(ContextModel):
    """A record on an inflow cell that a new mask makes solid is forgotten, not kept for the day the cell is fluid again."""

    def do_set_solids(self, mask_kind, seed):
        super().do_set_solids(mask_kind, seed)
        if self.profile:
            self.profile = [r for r in self.profile if not self.mask[r[0][1], r[0][0]]] or None


class ClearedOpeningsStillOpen(ContextModel):
    """The first step after clear_openings still follows the map that was cleared where a mask is set (a stale hook)."""
    stale = None

    def do_clear_openings(self):
        self.stale = (self.open, self.inflow, self.profile)
        super().do_clear_openings()

    def do_set_openings(self, open_kind, seed, inflow):
        self.stale = None
        super().do_set_openings(open_kind, seed, inflow)

    def step_once(self, dt, dx, iters, omega, until=None):
        if self.open is None and self.stale is not None and self.stale[0] is not None and self.mask is not None:
            (self.open, self.inflow, self.profile), self.stale = self.stale, None
            try:
                return super().step_once(dt, dx, iters, omega, until)
            finally:
                self.open, self.inflow, self.profile = None, (0.0, 0.0), None
        self.stale = None
        return super().step_once(dt, dx, iters, omega, until)


OPEN_STAND_INS = (OldCodesBehindAMap, NewMapKeepsTheProfile, SetInflowDropsTheProfile, SolidInflowRecordIsForgotten, ClearedOpeningsStillOpen)


def later_stand_in_subject(cls):
    return "record-context" if cls in RECORD_STAND_INS else "open-context"


def record_fresh_handle_check(oracle, make_handle, dim_x=61, dim_y=81, seed=3):
    """The kind of check the direct tests of the friction, the torque and the averages are: a fresh handle and every new call
    once, in one fixed order -- mask, labels, pivots, the recorders and the averages started together, ONE step call, the reads,
    the stops."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": seed})
    ops = [up(FV), up(FC), ("set_solids", {"mask_kind": "disc", "seed": 7}), ("set_bodies", {"label_kind": "halves", "bodies": 2, "seed": 1}),
           ("set_body_pivots", {"pivot_kind": "seeded", "bodies": 2, "seed": 4}), ("body_pivots", {}), ("loads_start", {"every": 2, "capacity": 4}),
           ("friction_start", {"every": 2, "capacity": 4}), ("torque_start", {"every": 1, "capacity": 4}), ("mean_start", {"what": 15, "every": 2}),
           ("step_n", {"n": 4, "dt": 1 / 30.0, "dx": 0.5, "iters": 5, "omega": 1.5}), ("friction", {}), ("torque", {}), ("friction_history", {}), ("torque_history", {}),
           ("mean_info", {})] + [("mean_sums", {"plane": k}) for k in range(mean_rule.PLANES)] + \
          [("mean_sample", {}), ("mean_sums", {"plane": 4}), ("mean_stop", {}), ("friction_stop", {}), ("torque_stop", {}), ("loads_stop", {}),
           ("set_body_pivots", {"pivot_kind": None, "bodies": 2, "seed": 0}), ("body_pivots", {}), ("torque", {})]
    model, handle = ContextModel(oracle, dim_x, dim_y), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            compare(got, want, f"a fresh handle, one order: {op[0]}")
    compare(handle.snapshot(), model.snapshot(), "a fresh handle, one order")


def open_fresh_handle_check(oracle, make_handle, dim_x=61, dim_y=81, seed=3):
    """The same for the openings: a mask, ONE map behind it, the inflow changed before the profile is set, one step call, the
    reads, every operator once; cleared once with the mask cleared too, every field uploaded again, one step."""
    up = lambda field: ("upload", {"field": field, "texture_kind": "noise", "seed": seed})
    solve = {"dx": 0.5, "iters": 5, "omega": 1.5}
    ops = [up(FV), up(FC), ("set_solids", {"mask_kind": "disc", "seed": 7}), ("set_openings", {"open_kind": "channel", "seed": 1, "inflow": [12.5, 0.0]}),
           ("set_inflow", {"inflow": [-3.0, 2.5]}), ("set_inflow_profile", {"cells": [[0, 5], [0, 40], [0, 5]], "vels": [[1.0, 2.0], [-3.0, 2.5], [7.5, -1.0]]}),
           ("openings", {}), ("inflow_profile", {}), ("step_n", dict({"n": 3, "dt": 1 / 30.0}, **solve)), ("openings_flux", {}), ("calculate_divergence", {"dx": 0.5}),
           ("poisson_solve", solve), ("residual", {"dx": 0.5}), ("poisson_continue", dict(solve, iters=9)), ("subtract_gradient", {"dx": 0.5}), ("flow_stats", {"dx": 0.5}),
           ("openings_flux", {}), ("clear_openings", {}), ("clear_solids", {}), ("openings", {}), ("inflow_profile", {}), up(FV), up(FC), up(FD), up(FP),
           ("step", dict({"dt": 1 / 30.0}, **solve))]
    model, handle = ContextModel(oracle, dim_x, dim_y), make_handle(dim_x, dim_y)
    for op in ops:
        want, got = model.apply(op), handle.apply(op)
        if want is not None:
            compare(got, want, f"a fresh handle, one order: {op[0]}")
    compare(handle.snapshot(), model.snapshot(), "a fresh handle, one order")
