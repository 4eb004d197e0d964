"""numpy-level front-end over the C ABI.

Three classes:

* :class:`Solver` -- one context (= one GPU's row slab, fields resident in HBM); thin, explicit.
* :class:`BatchSolver` -- a batch: many independent small grids of one shape, stepped by one launch.
* :class:`HostPath` -- the reference's operator interface on host arrays (same names, argument
  meaning and result layout as the oracle's ``CpuPath``), each call going through the
  ``sfl_host_*`` drop-ins or a temporary :class:`Solver`.  This is what the parity tests drive.

Array conventions (identical to the reference, operations.h:7-9): C-contiguous, row j major,
velocity ``float32[rows, dim_x, 2]``, dye ``uint32[rows, dim_x, 3]``, scalars ``float32[rows, dim_x]``.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi as capi

_FIELD_SPEC = {
    capi.FIELD_VELOCITY: (np.float32, 2),
    capi.FIELD_COLOR: (np.uint32, 3),
    capi.FIELD_DIVERGENCE: (np.float32, 1),
    capi.FIELD_PRESSURE: (np.float32, 1),
}


MEMBER_PARAMS_DTYPE = np.dtype([("dt", "<f4"), ("dx", "<f4"), ("omega", "<f4"), ("iters", "<i4")])   # sfl_member_params


def member_params(batch: int, dt, dx=1.0, iters=10, omega=1.96) -> np.ndarray:
    """The per-member records of ``BatchSolver.step_n_each`` / ``poisson_solve_each``: every argument a scalar (every
    member gets it) or a sequence of length `batch` (member m gets element m), as a C-contiguous structured array of
    `batch` records laid out as sfl_member_params.  Pure numpy: no GPU, no library."""
    out = np.empty(batch, MEMBER_PARAMS_DTYPE)
    for name, value in (("dt", dt), ("dx", dx), ("omega", omega), ("iters", iters)):
        a = np.asarray(value)
        if a.ndim > 1 or (a.ndim == 1 and len(a) != batch):
            raise ValueError(f"{name}: a scalar or a sequence of {batch} values (one per member), got shape {a.shape}")
        out[name] = a
    return out


MEMBER_STOP_DTYPE = np.dtype([("tol", "<f4"), ("every", "<i4")])   # sfl_member_stop


def member_stops(batch: int, tol, every=4) -> np.ndarray:
    """The per-member stopping records of ``BatchSolver.step_n_until`` / ``poisson_solve_until``: `tol` and `every` each a
    scalar or a sequence of length `batch`, as a C-contiguous structured array laid out as sfl_member_stop.  Pure numpy."""
    out = np.empty(batch, MEMBER_STOP_DTYPE)
    for name, value in (("tol", tol), ("every", every)):
        a = np.asarray(value)
        if a.ndim > 1 or (a.ndim == 1 and len(a) != batch):
            raise ValueError(f"{name}: a scalar or a sequence of {batch} values (one per member), got shape {a.shape}")
        out[name] = a
    return out


# struct sfl_flow_stats: what Solver.flow_stats returns (one record) and BatchSolver.flow_stats (one per member)
FLOW_STATS_DTYPE = np.dtype([("max_abs_vx", "<f4"), ("max_abs_vy", "<f4"), ("max_abs_div", "<f4"), ("what", "<u4"),
                             ("dye_sum", "<u8", (3,))])
# The tiles of the velocity pass of flow_stats (csrc/stats_kernels.h kStatsStripCols, kStatsChunkRows): a wave owns a strip
# of 128 columns and a chunk of 8 rows (16 or 32 on grids that fill the chip several times over).  Stated for the tests,
# which put extreme values on both sides of the boundaries; no result depends on them.
FLOW_STATS_STRIP_COLS, FLOW_STATS_CHUNK_ROWS = 128, 8


# struct sfl_field_distance: what Solver.distance returns (one record) and BatchSolver.distance (one per member)
FIELD_DISTANCE_DTYPE = np.dtype([("max_abs_dvx", "<f4"), ("max_abs_dvy", "<f4"), ("max_abs_dp", "<f4"), ("what", "<u4"),
                                 ("velocity_cells_differ", "<u4"), ("dye_cells_differ", "<u4"), ("pressure_cells_differ", "<u4"),
                                 ("max_abs_ddye", "<u4", (3,)), ("sum_abs_ddye", "<u8", (3,))])
# struct sfl_history_record: one sample of a history (Solver.history: one per sample; BatchSolver.history: one per sample
# and recorded member).  64 bytes; the first 40 are a FLOW_STATS_DTYPE record.
HISTORY_DTYPE = np.dtype({"names": ["max_abs_vx", "max_abs_vy", "max_abs_div", "what", "dye_sum", "update_norm", "iterations", "step",
                                    "dt", "dx"],
                          "formats": ["<f4", "<f4", "<f4", "<u4", ("<u8", (3,)), "<f4", "<i4", "<i8", "<f4", "<f4"],
                          "offsets": [0, 4, 8, 12, 16, 40, 44, 48, 56, 60], "itemsize": 64})
# struct sfl_body_load: the pressure load on one solid body (Solver.loads: one per body; BatchSolver.loads: one per member
# and body).  48 bytes; the load in pressure times cell widths is fx * 2^exp2, fy * 2^exp2.
BODY_LOAD_DTYPE = np.dtype([("fx", "<i8"), ("fy", "<i8"), ("exp2", "<i4"), ("max_abs_p", "<f4"), ("faces", "<u4", (4,)),
                            ("nonfinite", "<u4"), ("reserved", "<u4")])
# struct sfl_body_friction: the skin friction on one solid body (Solver.friction, BatchSolver.friction), laid out as the load.
# 48 bytes; the force per unit depth and density is nu * fx * 2^exp2 (no dx): friction_xy() does that arithmetic in float64.
BODY_FRICTION_DTYPE = np.dtype([("fx", "<i8"), ("fy", "<i8"), ("exp2", "<i4"), ("max_abs_t", "<f4"), ("faces", "<u4", (4,)),
                                ("nonfinite", "<u4"), ("reserved", "<u4")])
# struct sfl_body_torque: the moment of pressure and friction on one solid body about its pivot (Solver.torque,
# BatchSolver.torque).  64 bytes; the pressure torque in pressure times cell widths^2 is mp * 2^(exp2_p - 1), the friction
# torque per unit depth rho * nu * mf * 2^(exp2_f - 1) * dx: torque_xy() does that arithmetic in float64.
BODY_TORQUE_DTYPE = np.dtype([("mp", "<i8"), ("mf", "<i8"), ("exp2_p", "<i4"), ("exp2_f", "<i4"), ("max_abs_p", "<f4"), ("max_abs_t", "<f4"),
                              ("faces", "<u4"), ("max_arm2", "<u4"), ("nonfinite_p", "<u4"), ("nonfinite_t", "<u4"), ("pivot2", "<i4", (2,)),
                              ("reserved", "<u4", (2,))])
# struct sfl_open_flux: the flux through the live open cells of one grid (Solver.openings_flux: one record;
# BatchSolver.openings_flux: one per member).  40 bytes; the flux in velocity times cell widths is inflow * 2^exp2.
OPEN_FLUX_DTYPE = np.dtype([("inflow", "<i8"), ("outflow", "<i8"), ("exp2", "<i4"), ("max_abs_n", "<f4"), ("inflow_cells", "<u4"),
                            ("outflow_cells", "<u4"), ("nonfinite", "<u4"), ("reserved", "<u4")])
HISTORY_THREADS = 1024  # kHistoryThreads of csrc/history_kernels.h: threads of the sampler's workgroup (stated for the tests)


# The tiles of the distance passes and of the envelope (csrc/ensemble_kernels.h): a lane of a distance pass holds
# DIST_*_LANE_CELLS whole cells per load, a workgroup of DIST_THREADS lanes takes DIST_ITEM_LOADS loads per lane as one
# item; the envelope gives a workgroup ENV_BLOCK_WORDS words of a group of ENV_GROUP_MEMBERS members.  Stated for the
# tests, which put differing values on both sides of the boundaries; no result depends on them.
DIST_THREADS, DIST_ITEM_LOADS = 256, 8
DIST_VELOCITY_LANE_CELLS, DIST_PRESSURE_LANE_CELLS, DIST_DYE_LANE_CELLS = 2, 4, 1
ENV_BLOCK_WORDS, ENV_GROUP_MEMBERS = 256, 32


def _dist_what(velocity, dye, pressure) -> int:
    what = (capi.DIST_VELOCITY if velocity else 0) | (capi.DIST_DYE if dye else 0) | (capi.DIST_PRESSURE if pressure else 0)
    if not what:
        raise ValueError("distance: ask for the velocity, the dye, the pressure or several of them")
    return what


def _stats_what(velocity, dye) -> int:
    what = (capi.STATS_VELOCITY if velocity else 0) | (capi.STATS_DYE if dye else 0)
    if not what:
        raise ValueError("flow_stats: ask for the velocity, the dye or both")
    return what


def device_count() -> int:
    n = C.c_int(0)
    rc = capi.lib().sfl_device_count(C.byref(n))
    return n.value if rc == capi.OK else 0


def device_info(device: int = 0):
    name = C.create_string_buffer(256)
    cus, mem = C.c_int(0), C.c_size_t(0)
    capi.check(capi.lib().sfl_device_info(device, name, 256, C.byref(cus), C.byref(mem)))
    return name.value.decode(), cus.value, mem.value


def slab_rows(dim_y: int, nranks: int, rank: int):
    b, e = C.c_int(), C.c_int()
    capi.check(capi.lib().sfl_slab_rows(dim_y, nranks, rank, C.byref(b), C.byref(e)))
    return b.value, e.value


def sor_pass_plan(iters: int, fuse: int):
    n = C.c_int()
    capi.check(capi.lib().sfl_sor_pass_plan(iters, fuse, C.byref(n), None, 0))
    arr = (C.c_int * max(n.value, 1))()
    capi.check(capi.lib().sfl_sor_pass_plan(iters, fuse, C.byref(n), arr, n.value))
    return list(arr[: n.value])


def plan_poisson(dim_y: int, nranks: int, rank: int, iters: int, fuse: int = 8, kernel: int = 2,
                 halo: int = 0, tail: int = 0):
    """The launch / halo-exchange program of one poisson_solve for one rank (pure arithmetic).
    halo = rows of p exchanged per superstep (0: exchange before every launch); tail = ghost rows of p left
    exact at the end (early-exchange plans only)."""
    n = C.c_int()
    capi.check(capi.lib().sfl_plan_poisson_tail(dim_y, nranks, rank, iters, fuse, kernel, halo, tail, None, 0,
                                                C.byref(n)))
    steps = (capi.PlanStep * max(n.value, 1))()
    capi.check(capi.lib().sfl_plan_poisson_tail(dim_y, nranks, rank, iters, fuse, kernel, halo, tail, steps,
                                                n.value, C.byref(n)))
    return [steps[k] for k in range(n.value)]


class stdout_to_stderr:
    """RCCL prints a version banner on the C library's stdout while a communicator comes up (buffered: it would surface when
    the process exits).  A program whose stdout carries ONE JSON line wraps communicator creation in this: file descriptor 1
    points at stderr for the duration, and the C library's buffers are flushed before it is restored."""

    def __enter__(self):
        import os
        import sys
        sys.stdout.flush()
        self._saved = os.dup(1)
        os.dup2(2, 1)
        return self

    def __exit__(self, *exc):
        import os
        try:
            C.CDLL(None).fflush(None)
        finally:
            os.dup2(self._saved, 1)
            os.close(self._saved)


def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(capi.UNIQUE_ID_BYTES)
    capi.check(capi.lib().sfl_comm_unique_id(buf, capi.UNIQUE_ID_BYTES))
    return buf.raw


# ---- views: the flow itself as pictures (include/sfl.h "VIEWS") ----------------------------------------------------
_M = capi.VIEW_MAX_COLOUR   # the largest channel a palette may hold
PALETTE_GREY = np.array([[(n * _M) // 255] * 3 for n in range(256)], np.uint32)                    # black -> white
PALETTE_HEAT = np.array([[0, 0, 0], [_M, 0, 0], [_M, _M, 0], [_M, _M, _M]], np.uint32)             # black, red, yellow, white
PALETTE_BLUE_WHITE_RED = np.array([[0, 0, _M], [_M, _M, _M], [_M, 0, 0]], np.uint32)               # for lo = -hi: zero is white


class View:
    """A scalar of the flow and how it is drawn (struct sfl_view): `what` is capi.VIEW_SPEED, VIEW_VORTICITY,
    VIEW_PRESSURE or VIEW_DIVERGENCE; scalars lo .. hi map to the first .. last stop of `palette` (uint32[stops, 3], raw
    UQ32, every value <= capi.VIEW_MAX_COLOUR; 2..256 stops), linearly between neighbouring stops and clamped outside;
    a NaN gets `nan_colour`.  dx: the grid spacing of vorticity and divergence."""

    def __init__(self, what: int, lo: float, hi: float, palette=None, dx: float = 1.0, nan_colour=(0, _M, 0)):
        palette = PALETTE_GREY if palette is None else palette
        self.palette = np.array(palette, np.uint32, order="C")   # (a copy: the struct points into it)
        if self.palette.ndim != 2 or self.palette.shape[1] != 3:
            raise ValueError(f"a palette is uint32[stops, 3], got {self.palette.shape}")
        if len(nan_colour) != 3:
            raise ValueError("nan_colour is three UQ32 values")
        self.what, self.lo, self.hi, self.dx, self.nan_colour = int(what), float(lo), float(hi), float(dx), tuple(int(x) for x in nan_colour)

    def struct(self) -> "capi.View":
        """The C struct; it points into self.palette, which lives as long as this object."""
        return capi.View(self.what, self.dx, self.lo, self.hi, self.palette.shape[0], (C.c_uint32 * 3)(*self.nan_colour),
                         self.palette.ctypes.data_as(C.POINTER(C.c_uint32)))


def _u16p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint16))


class _Tracers:
    """Tracers: points that move with the flow and probes of the fields between the cell centres (include/sfl.h
    "TRACERS").  Shared by :class:`Solver` (``xy`` is ``float32[n, 2]``) and :class:`BatchSolver` (``float32[B, K, 2]``, K
    tracers in every member).  A position is (x along i, y along j) in grid coordinates, as ``sample()`` takes them."""

    _tracer_prefix = "sfl_tracers_"

    def _tracer_call(self, name):
        return getattr(self._lib, self._tracer_prefix + name)

    def _tracer_lead(self):   # the leading axes of every tracer array: () for a context, (B,) for a batch
        return ()

    def tracer_count(self) -> int:
        """Tracers attached: of the context, or of ONE member of the batch; 0 without a set."""
        n = C.c_size_t(0)
        capi.check(self._tracer_call("count")(self._h, C.byref(n)))
        return n.value

    def set_tracers(self, xy, follow: bool = True):
        """Attach tracers at `xy`, replacing the set held and ending its trail; an empty array removes the set.  With
        `follow` every step of every step call advances them by that step's dt on that step's projected velocity: they
        move as the dye does, and ``step_n(n)`` equals n x (``step``; ``advance_tracers(dt)``) bit for bit.  With a
        following set ``Solver.step_n`` runs without the fused step boundaries (OPT_STEP_SEAMS) and a batch's replay of
        a timeline runs one launch per step: same bits, the cost of single steps."""
        a = np.ascontiguousarray(xy, np.float32)
        lead = self._tracer_lead()
        if a.size == 0:
            capi.check(self._tracer_call("set")(self._h, None, 0, int(follow)))
            return
        if a.ndim != len(lead) + 2 or a.shape[:len(lead)] != lead or a.shape[-1] != 2:
            raise ValueError(f"tracers: float32{list(lead) + ['n', 2]}, got shape {a.shape}")
        capi.check(self._tracer_call("set")(self._h, _fp(a), a.shape[-2], int(follow)))

    def tracers(self) -> np.ndarray:
        """The positions now, ``float32[n, 2]`` (a batch: ``[B, K, 2]``).  Synchronous."""
        out = np.empty(self._tracer_lead() + (self.tracer_count(), 2), np.float32)
        capi.check(self._tracer_call("download")(self._h, _fp(out), out.size))
        return out

    def advance_tracers(self, dt):
        """One advance by `dt` on the current velocity: x += u.x * dt, y += u.y * dt with u = sample(velocity, x, y,
        no_slip=True); a tracer with a NaN coordinate stays as it is.  Asynchronous."""
        capi.check(self._tracer_call("advance")(self._h, dt))

    def sample_tracers(self, field: int, no_slip: bool = False) -> np.ndarray:
        """``sample()`` of one field at every tracer, bit for bit the header's: velocity ``float32[n, 2]``, dye
        ``uint32[n, 3]``, divergence and pressure ``float32[n]`` (a batch: a leading B).  A tracer with a NaN coordinate
        reads NaN (the dye: 0).  Reads only; synchronous."""
        dt, nc = _FIELD_SPEC.get(field, (np.float32, 1))
        out = np.empty(self._tracer_lead() + (self.tracer_count(),) + ((nc,) if nc > 1 else ()), dt)
        capi.check(self._tracer_call("sample")(self._h, field, int(no_slip), out.ctypes.data, out.nbytes))
        return out

    def trail_start(self, every: int = 1, capacity: int = 64):
        """Start a trail: after every `every`-th advance (followed or manual) the positions are also written to the
        next of `capacity` slots in device memory, by the advance's own launch.  A call whose advances would complete
        more slots than are free raises SflError with ERR_STATE and does nothing."""
        capi.check(self._tracer_call("trail_start")(self._h, every, capacity))

    def trail_info(self):
        """(slots written, capacity, advances counted since trail_start); zeros without a trail.  Never waits."""
        written, capacity, advances = C.c_int(), C.c_int(), C.c_int64()
        capi.check(self._tracer_call("trail_info")(self._h, C.byref(written), C.byref(capacity), C.byref(advances)))
        return written.value, capacity.value, advances.value

    def trail(self) -> np.ndarray:
        """The slots written so far, ``float32[slots, n, 2]`` (a batch: ``[slots, B, K, 2]``); not consumed.  Synchronous."""
        written = self.trail_info()[0]
        out = np.empty((written,) + self._tracer_lead() + (self.tracer_count(), 2), np.float32)
        capi.check(self._tracer_call("trail_read")(self._h, 0, written, _fp(out), out.size))
        return out

    def trail_stop(self):
        """Stop the trail and free its slots."""
        capi.check(self._tracer_call("trail_stop")(self._h))


class _History:
    """Histories: the flow statistics of every k-th step, recorded while stepping (include/sfl.h "HISTORIES").  Shared by
    :class:`Solver` (one record per sample) and :class:`BatchSolver` (one per sample and recorded member)."""

    _history_prefix = "sfl_history_"
    _hist = (0, 1)   # the recorded members (first, count); a context: its one record

    def _history_call(self, name):
        return getattr(self._lib, self._history_prefix + name)

    def _history_range(self, first, count):   # the arguments between `every` and `capacity`: none for a context
        if first != 0 or count not in (None, 1):
            raise ValueError("a context's history has one record per sample: first = 0, count = None")
        return (0, 1), ()

    def history_start(self, every: int, capacity: int, first: int = 0, count=None):
        """Start a history: after every `every`-th step of any step call -- counted across calls -- one launch on the
        stream writes one HISTORY_DTYPE record per recorded member (a batch: members [first, first + count), default all)
        from the fields that step left; `capacity` samples fit.  The step calls stay asynchronous.  A step call that
        would complete more samples than are free raises SflError with ERR_STATE and steps nothing: read them
        (:meth:`history`) and call history_start again.  Called while a history is on, it starts afresh.  With a history
        on, ``Solver.step_n`` runs without the fused step boundaries (OPT_STEP_SEAMS) and a batch's replay of a timeline
        is cut at the steps whose sample is due: same bits in every field."""
        hist, args = self._history_range(first, count)
        rc = self._history_call("start")(self._h, every, *args, capacity)
        if rc == capi.OK:
            self._hist = hist
        capi.check(rc)

    def history_info(self):
        """(samples written, capacity, steps counted since history_start); zeros without a history.  Never waits."""
        samples, capacity, steps = C.c_int(), C.c_int(), C.c_int64()
        capi.check(self._history_call("info")(self._h, C.byref(samples), C.byref(capacity), C.byref(steps)))
        return samples.value, capacity.value, steps.value

    def history(self) -> np.ndarray:
        """The samples written so far as a HISTORY_DTYPE array of shape ``(samples,)`` (a batch: ``(samples, count)``, the
        recorded members); not consumed.  A record equals, bit for bit, what ``flow_stats``, ``residual`` and
        ``iterations`` return right after the same step.  Synchronous."""
        samples = self.history_info()[0]
        first, count = self._hist
        out = np.zeros((samples, count), HISTORY_DTYPE)
        ptr = out.ctypes.data_as(C.POINTER(capi.HistoryRecord))
        if self._history_prefix == "sfl_history_":
            capi.check(self._history_call("read")(self._h, 0, samples, ptr, out.nbytes))
            return out[:, 0]
        capi.check(self._history_call("read")(self._h, 0, samples, first, count, ptr, out.nbytes))
        return out

    def history_stop(self):
        """Stop the history and free its samples."""
        capi.check(self._history_call("stop")(self._h))


class _Loads:
    """Loads: the pressure force on solid bodies, as figures and as curves recorded while stepping (include/sfl.h
    "LOADS").  Shared by :class:`Solver` (``[1, bodies]`` records per sample) and :class:`BatchSolver` (``[count, bodies]``)."""

    _loads_batch = False
    _loads_rec = (0, 1)   # the recorded members (first, count)

    def _loads_call(self, name):
        return getattr(self._lib, ("sfl_batch_" if self._loads_batch else "sfl_") + name)

    def _loads_members(self):
        return self.batch if self._loads_batch else 1

    def set_bodies(self, labels, bodies=None):
        """Label the bodies: a uint8 array of shape ``(dim_y, dim_x)`` (a batch: also ``(batch, dim_y, dim_x)``), 0 = in no
        body, 1..bodies = that body; `bodies` defaults to the largest label (at least 1).  None goes back to "every solid
        cell is body 1".  A label counts only where the cell is solid when a load is sampled.  Refused (ERR_STATE) while
        the loads recorder is on."""
        ptr = C.POINTER(C.c_uint8)
        if labels is None:
            args = (None, 0, 1) if self._loads_batch else (None, 1)
            capi.check(self._loads_call("set_bodies")(self._h, *args))
            return
        a = np.ascontiguousarray(labels)
        if a.dtype != np.uint8:
            raise ValueError(f"bodies: a uint8 array of labels, got {a.dtype}")
        shapes = [(self.dim_y, self.dim_x)] + ([(self.batch, self.dim_y, self.dim_x)] if self._loads_batch else [])
        if a.shape not in shapes:
            raise ValueError(f"bodies: shape {a.shape}, want one of {shapes}")
        if bodies is None:
            bodies = max(int(a.max()), 1)
        args = (int(a.ndim == 3), int(bodies)) if self._loads_batch else (int(bodies),)
        capi.check(self._loads_call("set_bodies")(self._h, a.ctypes.data_as(ptr), *args))

    def bodies_info(self):
        """(bodies, labelled) -- a batch: (bodies, labelled, per_member).  Never waits."""
        out = [C.c_int() for _ in range(3 if self._loads_batch else 2)]
        capi.check(self._loads_call("bodies_info")(self._h, *[C.byref(v) for v in out]))
        return (out[0].value,) + tuple(bool(v.value) for v in out[1:])

    def bodies(self, first: int = 0, count=None) -> np.ndarray:
        """The labels, uint8[dim_y, dim_x] (a batch: uint8[count, dim_y, dim_x] of members [first, first + count)); all 1
        without labels.  Synchronous."""
        ptr = C.POINTER(C.c_uint8)
        if not self._loads_batch:
            a = np.empty((self.dim_y, self.dim_x), np.uint8)
            capi.check(self._lib.sfl_bodies_download(self._h, a.ctypes.data_as(ptr), a.nbytes))
            return a
        count = self.batch - first if count is None else count
        a = np.empty((count, self.dim_y, self.dim_x), np.uint8)
        capi.check(self._lib.sfl_batch_bodies_download(self._h, first, count, a.ctypes.data_as(ptr), a.nbytes))
        return a

    def loads(self, first: int = 0, count=None) -> np.ndarray:
        """The pressure load on every body from the pressure held: a BODY_LOAD_DTYPE array of shape ``(count, bodies)`` --
        a context: ``(1, bodies)`` --, every field bit for bit what the rule of include/sfl.h "LOADS" gives on the
        downloaded pressure, mask and labels.  All zeros without solids.  Synchronous; changes no field."""
        n_bodies = self.bodies_info()[0]
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records: first = 0, count = None")
            out = np.zeros((1, n_bodies), BODY_LOAD_DTYPE)
            capi.check(self._lib.sfl_loads(self._h, out.ctypes.data_as(C.POINTER(capi.BodyLoad)), out.nbytes))
            return out
        count = self.batch - first if count is None else count
        out = np.zeros((count, n_bodies), BODY_LOAD_DTYPE)
        capi.check(self._lib.sfl_batch_loads(self._h, first, count, out.ctypes.data_as(C.POINTER(capi.BodyLoad)), out.nbytes))
        return out

    @staticmethod
    def _xy(rec):
        scale = np.ldexp(1.0, rec["exp2"].astype(np.int64))
        return np.stack([rec["fx"].astype(np.float64) * scale, rec["fy"].astype(np.float64) * scale], axis=-1)

    def loads_xy(self, first: int = 0, count=None) -> np.ndarray:
        """:meth:`loads` as float64 ``(count, bodies, 2)``: fx * 2^exp2, fy * 2^exp2, in pressure times cell widths
        (multiply by dx).  fx and fy have at most 63 bits: the product is rounded to double once."""
        return self._xy(self.loads(first, count))

    def loads_start(self, every: int, capacity: int, first: int = 0, count=None):
        """Start the loads recorder: after every `every`-th step of any step call -- counted across calls -- one launch on
        the stream writes the records of members [first, first + count) (a context: its own) from the fields that step
        left; `capacity` samples fit.  The step calls stay asynchronous.  A step call that would complete more samples
        than are free raises SflError with ERR_STATE and steps nothing.  A sample taken without solids set is zeros."""
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records per sample: first = 0, count = None")
            rc = self._lib.sfl_loads_start(self._h, every, capacity)
            rec = (0, 1)
        else:
            count = self.batch - first if count is None else count
            rc = self._lib.sfl_batch_loads_start(self._h, every, first, count, capacity)
            rec = (first, count)
        if rc == capi.OK:
            self._loads_rec = rec
        capi.check(rc)

    def loads_info(self):
        """(samples written, capacity, steps counted since loads_start, bodies).  Never waits."""
        samples, capacity, steps, n = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        capi.check(self._loads_call("loads_info")(self._h, C.byref(samples), C.byref(capacity), C.byref(steps), C.byref(n)))
        return samples.value, capacity.value, steps.value, n.value

    def loads_history(self) -> np.ndarray:
        """The samples written so far, BODY_LOAD_DTYPE of shape ``(samples, count, bodies)`` (a context: count = 1); sample
        s belongs to step (s + 1) * every since loads_start.  Not consumed.  Synchronous."""
        samples, _, _, n_bodies = self.loads_info()
        out = np.zeros((samples, self._loads_rec[1], n_bodies), BODY_LOAD_DTYPE)
        capi.check(self._loads_call("loads_read")(self._h, 0, samples, out.ctypes.data_as(C.POINTER(capi.BodyLoad)), out.nbytes))
        return out

    def loads_history_xy(self) -> np.ndarray:
        """:meth:`loads_history` as float64 ``(samples, count, bodies, 2)``."""
        return self._xy(self.loads_history())

    def loads_stop(self):
        """Stop the loads recorder and free its samples."""
        capi.check(self._loads_call("loads_stop")(self._h))


class _Friction:
    """Friction: the skin friction on solid bodies, beside the pressure load of :class:`_Loads` and with its bodies, as
    figures and as curves recorded while stepping (include/sfl.h "FRICTION").  Shared by :class:`Solver` (``[1, bodies]``
    records per sample) and :class:`BatchSolver` (``[count, bodies]``)."""

    _friction_rec = (0, 1)   # the recorded members (first, count)

    def _friction_ptr(self, a):
        return a.ctypes.data_as(C.POINTER(capi.BodyFriction))

    def friction(self, first: int = 0, count=None) -> np.ndarray:
        """The friction on every body from the velocity held: a BODY_FRICTION_DTYPE array of shape ``(count, bodies)`` --
        a context: ``(1, bodies)`` --, every field bit for bit what the rule of include/sfl.h "FRICTION" gives on the
        downloaded velocity, mask and labels.  All zeros without solids.  Synchronous; changes no field."""
        n_bodies = self.bodies_info()[0]
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records: first = 0, count = None")
            out = np.zeros((1, n_bodies), BODY_FRICTION_DTYPE)
            capi.check(self._lib.sfl_friction(self._h, self._friction_ptr(out), out.nbytes))
            return out
        count = self.batch - first if count is None else count
        out = np.zeros((count, n_bodies), BODY_FRICTION_DTYPE)
        capi.check(self._lib.sfl_batch_friction(self._h, first, count, self._friction_ptr(out), out.nbytes))
        return out

    def _friction_nu(self, nu, first, count):
        """nu as float64 that broadcasts against ``(..., count, bodies, 2)``: a scalar, one value per member of the range,
        or None for the viscosity that is set (per member in a batch; zeros when none is set)."""
        if nu is None:
            nu = self.viscosity()[0]
            if self._loads_batch:
                nu = nu[first:first + count]
        a = np.asarray(nu, dtype=np.float64)
        if a.ndim == 0:
            return a
        if a.shape != (count,):
            raise ValueError(f"friction: nu of shape {a.shape}, want a number or {(count,)}")
        return a[:, None, None]

    def friction_xy(self, nu=None, first: int = 0, count=None, relative: bool = False) -> np.ndarray:
        """:meth:`friction` as float64 ``(count, bodies, 2)``: nu * fx * 2^exp2, nu * fy * 2^exp2 -- the force per unit
        depth and density, with NO factor dx.  `nu`: a number, one value per member, or None for the viscosity that is
        set (zeros when none is).  `relative`: the wall's share (:func:`wall_shares`, from the wall table that is set) is
        subtracted in front of nu: the friction of the fluid's velocity RELATIVE to a moving wall.  The records keep
        their definition, the wall at rest."""
        rec = self.friction(first, count)
        xy = _Loads._xy(rec)
        if relative:
            xy = xy - self._wall_shares(first, rec.shape[0])[0]
        return self._friction_nu(nu, first, rec.shape[0]) * xy

    def _wall_shares(self, first, count):
        """(friction share float64 (count, bodies, 2), torque share float64 (count, bodies)) of members [first, first +
        count) -- a context: count = 1 -- from the mask, the labels, the pivots and the wall table that are set."""
        n_bodies = self.bodies_info()[0]
        if self._loads_batch:
            masks, labels, pivots = self.solids(first, count), self.bodies(first, count), self.body_pivots(first, count)
            tables = [self.wall_velocity(first + k) for k in range(count)]
        else:
            masks, labels, pivots, tables = self.solids()[None], self.bodies()[None], self.body_pivots()[None], [self.wall_velocity()]
        shares = [wall_shares(masks[k], labels[k], n_bodies, np.round(pivots[k] * 2.0).astype(np.int64), *tables[k]) for k in range(count)]
        return np.stack([f for f, _ in shares]), np.stack([t for _, t in shares])

    def friction_start(self, every: int, capacity: int, first: int = 0, count=None):
        """Start the friction recorder, by the rules of :meth:`loads_start` and independent of it: after every
        `every`-th step of any step call one launch on the stream writes the records of members [first, first + count)
        from the velocity that step left; `capacity` samples fit.  A step call that would complete more samples than are
        free raises SflError with ERR_STATE and steps nothing.  A sample taken without solids set is zeros."""
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records per sample: first = 0, count = None")
            rc = self._lib.sfl_friction_start(self._h, every, capacity)
            rec = (0, 1)
        else:
            count = self.batch - first if count is None else count
            rc = self._lib.sfl_batch_friction_start(self._h, every, first, count, capacity)
            rec = (first, count)
        if rc == capi.OK:
            self._friction_rec = rec
        capi.check(rc)

    def friction_info(self):
        """(samples written, capacity, steps counted since friction_start, bodies).  Never waits."""
        samples, capacity, steps, n = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        capi.check(self._loads_call("friction_info")(self._h, C.byref(samples), C.byref(capacity), C.byref(steps), C.byref(n)))
        return samples.value, capacity.value, steps.value, n.value

    def friction_history(self) -> np.ndarray:
        """The samples written so far, BODY_FRICTION_DTYPE of shape ``(samples, count, bodies)`` (a context: count = 1);
        sample s belongs to step (s + 1) * every since friction_start.  Not consumed.  Synchronous."""
        samples, _, _, n_bodies = self.friction_info()
        out = np.zeros((samples, self._friction_rec[1], n_bodies), BODY_FRICTION_DTYPE)
        capi.check(self._loads_call("friction_read")(self._h, 0, samples, self._friction_ptr(out), out.nbytes))
        return out

    def friction_history_xy(self, nu=None) -> np.ndarray:
        """:meth:`friction_history` as float64 ``(samples, count, bodies, 2)``, scaled by `nu` as :meth:`friction_xy`."""
        rec = self.friction_history()
        return self._friction_nu(nu, self._friction_rec[0], rec.shape[1]) * _Loads._xy(rec)

    def friction_stop(self):
        """Stop the friction recorder and free its samples."""
        capi.check(self._loads_call("friction_stop")(self._h))


MEAN_PLANE_NAMES = ("U", "V", "UU", "VV", "UV", "P", "PP", "R", "G", "B")   # plane ids 0..9 of include/sfl.h "AVERAGES"
_MEAN_GROUP_OF = (1, 1, 2, 2, 2, 4, 4, 8, 8, 8)                           # ... and the SFL_MEAN_* group of each


class _Means:
    """Averages: per-cell sums over time of the velocity, its second moments, the pressure and the dye, added on the device
    while stepping (include/sfl.h "AVERAGES").  The library reports SUMS and the number of samples; the means and the
    central moments are formed here, in float64.  Shared by :class:`Solver` (planes of shape ``(1, dim_y, dim_x)``) and
    :class:`BatchSolver` (``(count, dim_y, dim_x)``)."""

    _mean_rec = (0, 1)   # the recorded members (first, count)

    def mean_start(self, what: int, every: int, first: int = 0, count=None):
        """Allocate and zero the planes of the groups in `what` (a mask of ``capi.MEAN_*``) for members [first, first +
        count) and, for every >= 1, add one sample behind every `every`-th step of any step call from now on -- counted
        across calls; the step calls stay asynchronous.  every = 0: only :meth:`mean_sample` adds, and the step calls keep
        their fusion.  A start while on begins anew from zero."""
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of planes: first = 0, count = None")
            capi.check(self._lib.sfl_mean_start(self._h, what, every))
        else:
            count = self.batch - first if count is None else count
            capi.check(self._lib.sfl_batch_mean_start(self._h, what, every, first, count))
            self._mean_rec = (first, count)

    def mean_stop(self):
        """Drain the stream and free the planes."""
        capi.check(self._loads_call("mean_stop")(self._h))

    def mean_sample(self):
        """Add the fields held now as one more sample, asynchronously, whatever `every` is."""
        capi.check(self._loads_call("mean_sample")(self._h))

    def mean_info(self):
        """(what, every, samples added, steps counted since mean_start); zeros without averages on.  Never waits."""
        what, every, samples, steps = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        capi.check(self._loads_call("mean_info")(self._h, C.byref(what), C.byref(every), C.byref(samples), C.byref(steps)))
        return what.value, every.value, samples.value, steps.value

    def mean_sums(self, plane: int, first=None, count=None) -> np.ndarray:
        """The raw plane `plane` (``capi.MEAN_PLANE_*``) of members [first, first + count) -- default: the recorded range;
        any other must lie inside it --: float64, uint64 for the dye planes, of
        shape ``(count, dim_y, dim_x)``, bit for bit what the rule gives on the downloaded fields.  Synchronous."""
        dtype = np.uint64 if 0 <= plane < len(_MEAN_GROUP_OF) and _MEAN_GROUP_OF[plane] == capi.MEAN_DYE else np.float64
        if not self._loads_batch:
            if first not in (None, 0) or count not in (None, 1):
                raise ValueError("a context has one set of planes: first = None, count = None")
            out = np.empty((1, self.dim_y, self.dim_x), dtype)
            capi.check(self._lib.sfl_mean_download(self._h, plane, out.ctypes.data_as(C.c_void_p), out.nbytes))
            return out
        first = self._mean_rec[0] if first is None else first
        count = self._mean_rec[0] + self._mean_rec[1] - first if count is None else count
        out = np.empty((max(count, 0), self.dim_y, self.dim_x), dtype)
        capi.check(self._lib.sfl_batch_mean_download(self._h, plane, first, count, out.ctypes.data_as(C.c_void_p), out.nbytes))
        return out

    def means(self, first=None, count=None) -> dict:
        """The means of the live groups as float64 arrays by plane name ("U", "V", "UU", ..., "B"): sum / samples; the dye
        in units of the raw UQ32 value.  NaN everywhere while no sample has been added."""
        what, _, samples, _ = self.mean_info()
        n = np.float64(samples) if samples else np.float64("nan")
        return {name: self.mean_sums(k, first, count).astype(np.float64) / n
                for k, name in enumerate(MEAN_PLANE_NAMES) if what & _MEAN_GROUP_OF[k]}

    def reynolds_stress(self, first=None, count=None) -> dict:
        """The central second moments of the velocity, float64: ``uu`` = <u'u'> = UU/n - (U/n)^2, ``vv``, ``uv`` = UV/n -
        (U/n)(V/n), and ``tke`` = (uu + vv) / 2.  Needs the groups MEAN_VELOCITY and MEAN_STRESS."""
        what = self.mean_info()[0]
        if what & 3 != 3:
            raise ValueError(f"reynolds_stress: the averages hold the groups {what}; MEAN_VELOCITY | MEAN_STRESS are needed")
        m = self.means(first, count)
        uu, vv, uv = m["UU"] - m["U"] * m["U"], m["VV"] - m["V"] * m["V"], m["UV"] - m["U"] * m["V"]
        return {"uu": uu, "vv": vv, "uv": uv, "tke": 0.5 * (uu + vv)}


class _Torque:
    """Torque: the moment about z of the pressure load and of the skin friction on solid bodies about a pivot per body, as
    figures and as curves recorded while stepping (include/sfl.h "TORQUE").  Shared by :class:`Solver` (``[1, bodies]``
    records per sample) and :class:`BatchSolver` (``[count, bodies]``)."""

    _torque_rec = (0, 1)   # the recorded members (first, count)

    def _torque_ptr(self, a):
        return a.ctypes.data_as(C.POINTER(capi.BodyTorque))

    def set_body_pivots(self, xy):
        """The pivots in cells: floats of shape ``(bodies, 2)`` (a batch: also ``(batch, bodies, 2)``), (x, y) last, every
        value a multiple of 0.5 (ValueError otherwise) -- the library takes half cells.  None goes back to (0, 0) for every
        body.  Allowed while the recorder is on: the new pivots hold from the next sample."""
        ptr = C.POINTER(C.c_int32)
        if xy is None:
            args = (None, 0, 1) if self._loads_batch else (None, 1)
            capi.check(self._loads_call("set_body_pivots")(self._h, *args))
            return
        a = np.asarray(xy, dtype=np.float64)
        n_bodies = self.bodies_info()[0]
        shapes = [(n_bodies, 2)] + ([(self.batch, n_bodies, 2)] if self._loads_batch else [])
        if a.shape not in shapes:
            raise ValueError(f"pivots: shape {a.shape}, want one of {shapes}")
        twice = a * 2.0
        if not (np.isfinite(twice).all() and (twice == np.round(twice)).all() and (np.abs(twice) < 2.0 ** 31).all()):
            raise ValueError("pivots: every coordinate must be a multiple of 0.5 cells")
        p2 = np.ascontiguousarray(twice.astype(np.int32))
        args = (int(a.ndim == 3), n_bodies) if self._loads_batch else (n_bodies,)
        capi.check(self._loads_call("set_body_pivots")(self._h, p2.ctypes.data_as(ptr), *args))

    def body_pivots(self, first: int = 0, count=None) -> np.ndarray:
        """The pivots in cells, float64 ``(bodies, 2)`` (a batch: ``(count, bodies, 2)`` of members [first, first + count));
        zeros when none are set."""
        ptr = C.POINTER(C.c_int32)
        n_bodies = self.bodies_info()[0]
        if not self._loads_batch:
            a = np.zeros((n_bodies, 2), np.int32)
            capi.check(self._lib.sfl_body_pivots_download(self._h, a.ctypes.data_as(ptr), a.nbytes))
            return a / 2.0
        count = self.batch - first if count is None else count
        a = np.zeros((count, n_bodies, 2), np.int32)
        capi.check(self._lib.sfl_batch_body_pivots_download(self._h, first, count, a.ctypes.data_as(ptr), a.nbytes))
        return a / 2.0

    def torque(self, first: int = 0, count=None) -> np.ndarray:
        """The torque on every body from the pressure and the velocity held: a BODY_TORQUE_DTYPE array of shape
        ``(count, bodies)`` -- a context: ``(1, bodies)`` --, every field bit for bit what the rule of include/sfl.h "TORQUE"
        gives on the downloaded fields, mask, labels and pivots.  Zeros but for pivot2 without solids.  Synchronous."""
        n_bodies = self.bodies_info()[0]
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records: first = 0, count = None")
            out = np.zeros((1, n_bodies), BODY_TORQUE_DTYPE)
            capi.check(self._lib.sfl_torque(self._h, self._torque_ptr(out), out.nbytes))
            return out
        count = self.batch - first if count is None else count
        out = np.zeros((count, n_bodies), BODY_TORQUE_DTYPE)
        capi.check(self._lib.sfl_batch_torque(self._h, first, count, self._torque_ptr(out), out.nbytes))
        return out

    def _torque_xy(self, rec, first, dx, rho):
        """float64 ``(..., count, bodies, 2)`` of records ``(..., count, bodies)``: the pressure torque mp * 2^(exp2_p - 1) *
        dx^2 and the friction torque rho * nu * mf * 2^(exp2_f - 1) * dx, nu the viscosity that is set (per member)."""
        nu = self._friction_nu(None, first, rec.shape[-2])
        nu = nu if nu.ndim == 0 else nu[:, :, 0]   # (count, 1) against (..., count, bodies)
        mp = rec["mp"].astype(np.float64) * np.ldexp(1.0, rec["exp2_p"].astype(np.int64) - 1) * (float(dx) * float(dx))
        mf = rec["mf"].astype(np.float64) * np.ldexp(1.0, rec["exp2_f"].astype(np.int64) - 1) * nu * (float(rho) * float(dx))
        return np.stack([mp, mf], axis=-1)

    def torque_xy(self, dx: float = 1.0, rho: float = 1.0, first: int = 0, count=None, relative: bool = False) -> np.ndarray:
        """:meth:`torque` as float64 ``(count, bodies, 2)``: [..., 0] the pressure torque in pressure x length^2, [..., 1] the
        friction torque per unit depth, with the viscosity that is set (zeros when none is).  Counter-clockwise positive.
        `relative`: the wall's share of the friction torque (:func:`wall_shares`) is subtracted, as in :meth:`friction_xy`."""
        rec = self.torque(first, count)
        out = self._torque_xy(rec, first, dx, rho)
        if relative:
            nu = self._friction_nu(None, first, rec.shape[-2])
            nu = nu if nu.ndim == 0 else nu[:, :, 0]
            out[..., 1] -= self._wall_shares(first, rec.shape[-2])[1] * nu * (float(rho) * float(dx))
        return out

    def torque_start(self, every: int, capacity: int, first: int = 0, count=None):
        """Start the torque recorder, by the rules of :meth:`loads_start` and independent of the other recorders; behind a
        step the order is history, loads, friction, torque."""
        if not self._loads_batch:
            if first != 0 or count not in (None, 1):
                raise ValueError("a context has one set of records per sample: first = 0, count = None")
            rc = self._lib.sfl_torque_start(self._h, every, capacity)
            rec = (0, 1)
        else:
            count = self.batch - first if count is None else count
            rc = self._lib.sfl_batch_torque_start(self._h, every, first, count, capacity)
            rec = (first, count)
        if rc == capi.OK:
            self._torque_rec = rec
        capi.check(rc)

    def torque_info(self):
        """(samples written, capacity, steps counted since torque_start, bodies).  Never waits."""
        samples, capacity, steps, n = C.c_int(), C.c_int(), C.c_int64(), C.c_int()
        capi.check(self._loads_call("torque_info")(self._h, C.byref(samples), C.byref(capacity), C.byref(steps), C.byref(n)))
        return samples.value, capacity.value, steps.value, n.value

    def torque_history(self) -> np.ndarray:
        """The samples written so far, BODY_TORQUE_DTYPE of shape ``(samples, count, bodies)`` (a context: count = 1); sample
        s belongs to step (s + 1) * every since torque_start.  Not consumed.  Synchronous."""
        samples, _, _, n_bodies = self.torque_info()
        out = np.zeros((samples, self._torque_rec[1], n_bodies), BODY_TORQUE_DTYPE)
        capi.check(self._loads_call("torque_read")(self._h, 0, samples, self._torque_ptr(out), out.nbytes))
        return out

    def torque_history_xy(self, dx: float = 1.0, rho: float = 1.0) -> np.ndarray:
        """:meth:`torque_history` as float64 ``(samples, count, bodies, 2)``, scaled as :meth:`torque_xy`."""
        return self._torque_xy(self.torque_history(), self._torque_rec[0], dx, rho)

    def torque_stop(self):
        """Stop the torque recorder and free its samples."""
        capi.check(self._loads_call("torque_stop")(self._h))


class Solver(_Tracers, _History, _Loads, _Friction, _Torque, _Means):
    """One solver context: rows [row_begin, row_end) of a dim_x * dim_y domain on one device."""

    def __init__(self, dim_x: int, dim_y: int, device: int = 0, rank: int = 0, nranks: int = 1):
        self._h = C.c_void_p()
        self._lib = capi.lib()
        capi.check(self._lib.sfl_create_slab(C.byref(self._h), device, dim_x, dim_y, rank, nranks))
        self.dim_x, self.dim_y, self.rank, self.nranks = dim_x, dim_y, rank, nranks
        self.row_begin, self.row_end = slab_rows(dim_y, nranks, rank)

    # -- lifetime ------------------------------------------------------------------------
    def close(self):
        if self._h:
            self._lib.sfl_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def rows(self) -> int:
        return self.row_end - self.row_begin

    # -- configuration -------------------------------------------------------------------
    def set_option(self, option: int, value: int):
        capi.check(self._lib.sfl_set_option(self._h, option, value))

    def get_option(self, option: int) -> int:
        v = C.c_int()
        capi.check(self._lib.sfl_get_option(self._h, option, C.byref(v)))
        return v.value

    def comm_attach(self, unique_id: bytes):
        capi.check(self._lib.sfl_comm_attach(self._h, unique_id, len(unique_id)))

    def comm_check_options(self):
        """Collective: every rank of the communicator must carry the same domain and options (sfl_comm_check_options)."""
        capi.check(self._lib.sfl_comm_check_options(self._h))

    def comm_loopback(self, rows: int):
        capi.check(self._lib.sfl_comm_loopback(self._h, rows))

    def comm_emulate(self):
        """This rank's program alone, halo messages as self-copies (timing only; sfl_comm_emulate)."""
        capi.check(self._lib.sfl_comm_emulate(self._h))

    def comm_emulate_rccl(self):
        """This rank's program alone with real RCCL messages to itself as the transport (timing only; sfl_comm_emulate_rccl)."""
        capi.check(self._lib.sfl_comm_emulate_rccl(self._h))

    @staticmethod
    def link_group(solvers):
        """Join slabs living on one device into an in-process group (virtual ranks)."""
        arr = (C.c_void_p * len(solvers))(*[s._h for s in solvers])
        capi.check(capi.lib().sfl_group_link(arr, len(solvers)))

    # -- field I/O (owned rows) --------------------------------------------------------------
    def _shape(self, field):
        dt, nc = _FIELD_SPEC[field]
        return (self.rows, self.dim_x, nc) if nc > 1 else (self.rows, self.dim_x)

    def upload(self, field: int, a: np.ndarray):
        dt, _ = _FIELD_SPEC[field]
        a = np.ascontiguousarray(a, dtype=dt)
        if a.shape != self._shape(field):
            raise ValueError(f"field {field}: shape {a.shape}, slab wants {self._shape(field)}")
        capi.check(self._lib.sfl_upload(self._h, field, a.ctypes.data, a.nbytes))

    def download(self, field: int) -> np.ndarray:
        dt, _ = _FIELD_SPEC[field]
        a = np.empty(self._shape(field), dt)
        capi.check(self._lib.sfl_download(self._h, field, a.ctypes.data, a.nbytes))
        return a

    def device_ptr(self, field: int) -> int:
        p = C.c_void_p()
        capi.check(self._lib.sfl_field_device_ptr(self._h, field, C.byref(p)))
        return p.value

    # -- operators (asynchronous on the context's stream) -----------------------------------
    def advect_velocity(self, dt, no_slip=True):
        capi.check(self._lib.sfl_advect_velocity(self._h, dt, int(no_slip)))

    def advect_color(self, dt, no_slip=False):
        capi.check(self._lib.sfl_advect_color(self._h, dt, int(no_slip)))

    def advect_external(self, next_p_dev: int, p_dev: int, channels: int, kind: int, dt, no_slip):
        """A field of the caller's (device pointers) advected with the resident velocity (sfl_advect_external)."""
        capi.check(self._lib.sfl_advect_external(self._h, next_p_dev, p_dev, channels, kind, dt, int(no_slip)))

    def calculate_divergence(self, dx=1.0):
        capi.check(self._lib.sfl_calculate_divergence(self._h, dx))

    def poisson_solve(self, dx=1.0, iters=10, omega=1.96):
        capi.check(self._lib.sfl_poisson_solve(self._h, dx, iters, omega))

    def residual(self, dx=1.0) -> np.float32:
        """The update norm of the pressure and divergence the context holds right now: max |p_gs - p| over all cells, a
        NaN when any cell's is one (include/sfl.h sfl_residual; the definition of BatchSolver.residual).  One pass over
        p and d; synchronous.  Whole-domain contexts only."""
        u = C.c_float()
        capi.check(self._lib.sfl_residual(self._h, dx, C.byref(u)))
        return np.float32(u.value)

    def poisson_continue(self, dx=1.0, iters=10, omega=1.96):
        """`iters` more red-black iterations on the pressure the context holds (sfl_poisson_continue): after
        poisson_solve(dx, a, omega) it leaves poisson_solve(dx, a + iters, omega), bit for bit; after an upload of the
        pressure it iterates from that field.  Whole-domain contexts only."""
        capi.check(self._lib.sfl_poisson_continue(self._h, dx, iters, omega))

    def poisson_solve_until(self, dx=1.0, max_iters=10, omega=1.96, tol=None, every=8):
        """poisson_solve stopped at a tolerance (sfl_poisson_solve_until, the rule of BatchSolver.poisson_solve_until): in
        front of every `every`-th iteration the update norm is checked, and the solve ends at the first check that finds
        it <= `tol` (or a NaN), at `max_iters` at the latest; a negative `tol` never stops.  A check is one pass over p
        and d and a round trip to the host -- at 8192 x 8192 what about six iterations cost -- so choose `every` with
        that in mind (include/sfl.h has the measurements).  Returns (iterations,
        residual): the iterations run and the update norm of the pressure they left.  Synchronous.  Whole-domain
        contexts only."""
        if tol is None:
            raise ValueError("tol: a tolerance is required (a negative one never stops the solve)")
        k, u = C.c_int32(), C.c_float()
        capi.check(self._lib.sfl_poisson_solve_until(self._h, dx, max_iters, omega, tol, every, C.byref(k), C.byref(u)))
        return k.value, np.float32(u.value)

    def subtract_gradient(self, dx=1.0):
        capi.check(self._lib.sfl_subtract_gradient(self._h, dx))

    def flow_stats(self, dx=1.0, velocity=True, dye=True):
        """What the flow the context holds looks like, without a download (sfl_flow_stats): one record of
        FLOW_STATS_DTYPE.  With `velocity`: max_abs_vx, max_abs_vy = max |v.x|, max |v.y| -- times dt the longest
        back-trace of the next advection, bit for bit -- and max_abs_div = max |calculate_divergence(v, dx)|, the figure
        of merit of the projection; a NaN anywhere makes the figure a NaN.  With `dye`: dye_sum = the exact uint64 sum
        of every channel's raw values.  Bit for bit what numpy gives on the downloaded fields; one streaming pass per
        part asked for; reads only; synchronous.  Whole-domain contexts only."""
        what, out = _stats_what(velocity, dye), np.zeros((), FLOW_STATS_DTYPE)
        capi.check(self._lib.sfl_flow_stats(self._h, what, dx, out.ctypes.data_as(C.POINTER(capi.FlowStats))))
        return out[()]

    def distance(self, other: "Solver", velocity=True, dye=True, pressure=True):
        """How far this context's fields are from `other`'s, without a download (sfl_distance): one record of
        FIELD_DISTANCE_DTYPE.  max_abs_dvx / dvy / dp = max |a - b| in float32 (a NaN anywhere makes the figure a NaN),
        max_abs_ddye / sum_abs_ddye = per channel the maximum and the exact uint64 sum of |a - b| on the raw values,
        *_cells_differ = the cells whose BITS differ: all zero <=> the fields are identical bits.  Bit for bit what numpy
        gives on the downloaded fields; one streaming pass per part asked for; reads only; synchronous.  Whole-domain
        contexts of one shape on one device; ``other`` may be ``self``."""
        what, out = _dist_what(velocity, dye, pressure), np.zeros((), FIELD_DISTANCE_DTYPE)
        capi.check(self._lib.sfl_distance(self._h, other._h, what, out.ctypes.data_as(C.POINTER(capi.FieldDistance))))
        return out[()]

    def step(self, dt, dx=1.0, iters=10, omega=1.96):
        capi.check(self._lib.sfl_step(self._h, dt, dx, iters, omega))

    def step_n(self, n, dt, dx=1.0, iters=10, omega=1.96):
        """n steps in one call (sfl_step_n): the same results as n x step(), fused across the step boundaries."""
        capi.check(self._lib.sfl_step_n(self._h, n, dt, dx, iters, omega))

    def queue_forces(self, cells_ij, vel_xy, step: int = 0):
        """Point forces for step `step` of the steps to come (0: the next one); the timeline rule of include/sfl.h."""
        cells = np.ascontiguousarray(cells_ij, np.int32).reshape(-1, 2)
        vel = np.ascontiguousarray(vel_xy, np.float32).reshape(-1, 2)
        capi.check(self._lib.sfl_queue_forces_at(
            self._h, step, cells.ctypes.data_as(C.POINTER(C.c_int)),
            vel.ctypes.data_as(C.POINTER(C.c_float)), len(cells)))

    def forces_pending(self):
        """(records, last_step) of the timeline of queued forces; last_step is -1 when it is empty."""
        records, last = C.c_int(0), C.c_int(0)
        capi.check(self._lib.sfl_forces_pending(self._h, C.byref(records), C.byref(last)))
        return records.value, last.value

    def forget_forces(self):
        """Empties the timeline of queued forces."""
        capi.check(self._lib.sfl_forget_forces(self._h))

    def queue_drags(self, drags, step: int = 0):
        """drags: iterable of (coords_x, coords_y, velocity_x, velocity_y) in the sketch's graphics coordinates
        (struct drag, ino:45-48); transformed like ino:264-269 by the library.  step: as for queue_forces."""
        drags = list(drags)
        arr = (capi.Drag * max(len(drags), 1))(*[capi.Drag(int(a), int(b), float(c), float(d)) for a, b, c, d in drags])
        capi.check(self._lib.sfl_queue_drags_at(self._h, step, C.cast(arr, C.c_void_p), len(drags)))

    def setup_sketch_fields(self):
        """Velocity = 0, dye = the sketch's blurred three-sector pattern (setup(), ino:196-241)."""
        capi.check(self._lib.sfl_setup_sketch_fields(self._h))

    def render_rgb565(self, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """Dye field -> RGB565 image, uint16[scaling*(dim_x-1), scaling*(dim_y-1)] (ino:116-176)."""
        img = np.empty((scaling * (self.dim_x - 1), scaling * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_render_rgb565(self._h, scaling, int(byteswap),
                                               img.ctypes.data_as(C.POINTER(C.c_uint16)), img.nbytes))
        return img

    # -- views ---------------------------------------------------------------------------
    def view_scalar(self, what: int, dx: float = 1.0) -> np.ndarray:
        """Speed, vorticity, pressure or divergence (capi.VIEW_*) of the fields held now, float32[dim_y, dim_x]."""
        out = np.empty((self.dim_y, self.dim_x), np.float32)
        capi.check(self._lib.sfl_view_scalar(self._h, what, dx, out.ctypes.data_as(C.POINTER(C.c_float)), out.nbytes))
        return out

    def view_texels(self, view: View) -> np.ndarray:
        """The node colours of a view, uint32[dim_y, dim_x, 3]: laid out as the dye."""
        out = np.empty((self.dim_y, self.dim_x, 3), np.uint32)
        capi.check(self._lib.sfl_view_texels(self._h, C.byref(view.struct()), out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes))
        return out

    def view_render(self, view: View, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """A view -> RGB565 image shaped as :meth:`render_rgb565`'s: the draw task's chain on the view's node colours."""
        img = np.empty((max(scaling, 0) * (self.dim_x - 1), max(scaling, 0) * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_view_render(self._h, C.byref(view.struct()), scaling, int(byteswap), _u16p(img), img.nbytes))
        return img

    # -- solid cells ---------------------------------------------------------------------
    def set_solids(self, mask):
        """Solid cells inside the grid (include/sfl.h "SOLIDS OF A CONTEXT"): `mask` a bool or uint8 array of shape
        ``(dim_y, dim_x)``, nonzero = solid; None clears the solids.  No field is touched.  Whole-domain contexts
        without a transport, at any grid size; step, step_n, calculate_divergence, poisson_solve, poisson_continue,
        poisson_solve_until, subtract_gradient, residual, flow_stats and histories then follow the solids' rule -- the
        rule of :meth:`BatchSolver.set_solids`, bit for bit -- and the divergence view is refused while set."""
        if mask is None:
            capi.check(self._lib.sfl_set_solids(self._h, None))
            return
        mask = np.asarray(mask)
        if mask.dtype != np.bool_ and mask.dtype != np.uint8:
            raise ValueError(f"solids: a bool or uint8 mask, got {mask.dtype}")
        if mask.shape != (self.dim_y, self.dim_x):
            raise ValueError(f"solids: shape {mask.shape}, want {(self.dim_y, self.dim_x)}")
        m = np.ascontiguousarray(mask != 0, dtype=np.uint8)
        capi.check(self._lib.sfl_set_solids(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8))))

    def solids_info(self):
        """(set, solid_cells) as the library reports it."""
        s, n = C.c_int(0), C.c_int64(0)
        capi.check(self._lib.sfl_solids_info(self._h, C.byref(s), C.byref(n)))
        return bool(s.value), n.value

    def solids(self) -> np.ndarray:
        """The mask, bool[dim_y, dim_x]: all False without solids.  Synchronous."""
        a = np.zeros((self.dim_y, self.dim_x), np.uint8)
        capi.check(self._lib.sfl_solids_download(self._h, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.nbytes))
        return a.astype(bool)

    # -- viscosity -----------------------------------------------------------------------
    def set_openings(self, open, inflow=(0.0, 0.0)):
        """Inflow and outflow cells on the rim of the grid (include/sfl.h "OPENINGS OF A CONTEXT"): `open` a uint8 array
        ``(dim_y, dim_x)`` of 0, OPEN_INFLOW and OPEN_OUTFLOW, nonzero only on rim cells that are no corners; `inflow` the
        ``(u, v)`` every fluid inflow cell holds after the forces; None clears the openings.  No field is touched.  step,
        step_n, the operators, the solves, residual, flow_stats and histories then follow the openings' rule, with and
        without solids; slabs, transports, the divergence view and viscosity are refused while set."""
        if open is None:
            capi.check(self._lib.sfl_set_openings(self._h, None, 0.0, 0.0))
            return
        m = np.asarray(open)
        if m.dtype != np.uint8:
            raise ValueError(f"openings: a uint8 map, got {m.dtype}")
        if m.shape != (self.dim_y, self.dim_x):
            raise ValueError(f"openings: shape {m.shape}, want {(self.dim_y, self.dim_x)}")
        u = np.asarray(inflow, dtype=np.float32)
        if u.shape != (2,):
            raise ValueError(f"openings: inflow of shape {u.shape}, want (2,)")
        m = np.ascontiguousarray(m)
        capi.check(self._lib.sfl_set_openings(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), C.c_float(u[0]), C.c_float(u[1])))

    def set_inflow(self, inflow):
        """Change the inflow velocity ``(u, v)`` of a context with openings set.  The map stays."""
        u = np.asarray(inflow, dtype=np.float32)
        if u.shape != (2,):
            raise ValueError(f"openings: inflow of shape {u.shape}, want (2,)")
        capi.check(self._lib.sfl_set_inflow(self._h, C.c_float(u[0]), C.c_float(u[1])))

    def openings_info(self):
        """(set, live inflow cells, live outflow cells) as the library reports it."""
        s, n_in, n_out = C.c_int(0), C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.sfl_openings_info(self._h, C.byref(s), None, None, C.byref(n_in), C.byref(n_out)))
        return bool(s.value), n_in.value, n_out.value

    def openings(self):
        """(the map, uint8[dim_y, dim_x]; the inflow, float32[2]): zeros without openings."""
        m = np.zeros((self.dim_y, self.dim_x), np.uint8)
        capi.check(self._lib.sfl_openings_download(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.nbytes))
        x, y = C.c_float(0), C.c_float(0)
        capi.check(self._lib.sfl_openings_info(self._h, None, C.byref(x), C.byref(y), None, None))
        return m, np.array([x.value, y.value], np.float32)

    def set_inflow_profile(self, cells, vel):
        """A per-cell inflow profile (include/sfl.h "INFLOW PROFILES AND FLUX"): `cells` integers ``(n, 2)``, (i, j) per
        record, each a cell whose map byte is OPEN_INFLOW; `vel` float32 ``(n, 2)``.  After the forces those cells hold their
        record's velocity, every other fluid inflow cell the uniform inflow.  Of two records on one cell the later wins;
        n == 0 (or None) clears the profile; a new map drops it, set_inflow keeps it."""
        c, v = _profile_records([] if cells is None else cells, [] if vel is None else vel)
        capi.check(self._lib.sfl_set_inflow_profile(self._h, c.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_float)), len(c)))

    def inflow_profile(self):
        """(cells int32[n, 2], vel float32[n, 2]): the records held, in cell-index order; empty without a profile."""
        n = C.c_int(0)
        capi.check(self._lib.sfl_inflow_profile_info(self._h, C.byref(n)))
        c, v = np.zeros((n.value, 2), np.int32), np.zeros((n.value, 2), np.float32)
        capi.check(self._lib.sfl_inflow_profile_download(self._h, c.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_float)), n.value))
        return c, v

    def set_wall_velocity(self, cells, vel):
        """Wall velocities (include/sfl.h "WALL VELOCITIES"): `cells` integers ``(n, 2)``, (i, j) per record, each a SOLID
        cell of the mask that is set; `vel` float32 ``(n, 2)``.  In step and step_n those cells hold their record's velocity
        where item 3a and the next step's advection read them; the pressure still sees a wall at rest.  Of two records on
        one cell the later wins; n == 0 (or None) clears the table; every set_solids drops it."""
        c, v = _profile_records([] if cells is None else cells, [] if vel is None else vel, "wall velocity")
        capi.check(self._lib.sfl_set_wall_velocity(self._h, c.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_float)), len(c)))

    def wall_velocity(self):
        """(cells int32[n, 2], vel float32[n, 2]): the records held, in cell-index order; empty without a table."""
        n = self.wall_velocity_info()
        c, v = np.zeros((n, 2), np.int32), np.zeros((n, 2), np.float32)
        capi.check(self._lib.sfl_wall_velocity_download(self._h, c.ctypes.data_as(C.POINTER(C.c_int)), v.ctypes.data_as(C.POINTER(C.c_float)), n))
        return c, v

    def wall_velocity_info(self) -> int:
        """The number of unique cells the wall table holds (0 without one).  Never waits."""
        n = C.c_int(0)
        capi.check(self._lib.sfl_wall_velocity_info(self._h, C.byref(n)))
        return n.value

    def openings_flux(self) -> np.ndarray:
        """The flux through the live open cells from the velocity held: one OPEN_FLUX_DTYPE record (shape ``()``); exact
        integers, see :func:`openings_flux_xy`.  All zeros without openings.  One launch over the rim, synchronous."""
        out = np.zeros((), OPEN_FLUX_DTYPE)
        capi.check(self._lib.sfl_openings_flux(self._h, out.ctypes.data_as(C.POINTER(capi.OpenFlux))))
        return out

    def set_viscosity(self, nu, sweeps: int):
        """Viscosity (include/sfl.h "VISCOSITY"): step and step_n then run `sweeps` red-black sweeps of an implicit
        diffusion of the velocity between the forces and the divergence, as one unfused sequence per step.  nu == 0 or
        sweeps == 0 clears it.  Whole-domain contexts without a transport, at any grid size; honours the solids."""
        capi.check(self._lib.sfl_set_viscosity(self._h, float(nu), int(sweeps)))

    def viscosity(self):
        """(nu, sweeps) as the library reports it: (0.0, 0) when none is set."""
        nu, s = C.c_float(0), C.c_int(0)
        capi.check(self._lib.sfl_viscosity_info(self._h, C.byref(nu), C.byref(s)))
        return np.float32(nu.value), s.value

    def diffuse_velocity(self, nu, dt, dx=1.0, sweeps: int = 1):
        """The diffusion as an operator of its own on the velocity held; needs nothing set."""
        capi.check(self._lib.sfl_diffuse_velocity(self._h, float(nu), float(dt), float(dx), int(sweeps)))

    def synchronize(self):
        capi.check(self._lib.sfl_synchronize(self._h))

    def timer_start(self):
        capi.check(self._lib.sfl_timer_start(self._h))

    def timer_stop(self) -> float:
        ms = C.c_float()
        capi.check(self._lib.sfl_timer_stop(self._h, C.byref(ms)))
        return ms.value

    def last_solve_info(self):
        a, b, c = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._lib.sfl_last_solve_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return {"launches": a.value, "exchanges": b.value, "fuse": c.value, "halo": self.get_option(capi.OPT_LAST_HALO)}


class BatchSolver(_Tracers, _History, _Loads, _Friction, _Torque, _Means):
    """A batch (sfl_batch_*): `batch` independent whole-domain simulations of one dim_x * dim_y grid on one device,
    every member stepped by the same launch.  Member m holds, bit for bit, what a :class:`Solver` of the same shape
    holds after the same calls made with member m's data and forces.  Arrays of members are shaped
    ``(count, dim_y, dim_x[, k])``.

    ``large=True`` makes a batch of large members (sfl_batch_create_large): up to ``capi.BATCH_LARGE_MAX_CELLS`` cells
    per member instead of 6144, 8 B of LDS per cell instead of 16, one member per CU.  Every method is the same."""

    def __init__(self, dim_x: int, dim_y: int, batch: int, device: int = 0, large: bool = False):
        self._h = C.c_void_p()
        self._lib = capi.lib()
        create = self._lib.sfl_batch_create_large if large else self._lib.sfl_batch_create
        capi.check(create(C.byref(self._h), device, dim_x, dim_y, batch))
        self.dim_x, self.dim_y, self.batch, self.device = dim_x, dim_y, batch, device
        self._rec = (0, 0, 1)   # (first, count, scaling) of the running recording: the shape of what frames() reads

    _tracer_prefix = "sfl_batch_tracers_"
    _history_prefix = "sfl_batch_history_"
    _loads_batch = True

    def _tracer_lead(self):
        return (self.batch,)

    def _history_range(self, first, count):
        count = self.batch - first if count is None else count
        return (first, count), (first, count)

    def close(self):
        if self._h:
            self._lib.sfl_batch_destroy(self._h)
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def large(self) -> bool:
        """True for a batch of large members (``large=True``), as the library reports it."""
        flag = C.c_int()
        capi.check(self._lib.sfl_batch_is_large(self._h, C.byref(flag)))
        return bool(flag.value)

    @property
    def shape(self):
        """(dim_x, dim_y, batch) as the library reports it."""
        x, y, b = C.c_int(), C.c_int(), C.c_int()
        capi.check(self._lib.sfl_batch_shape(self._h, C.byref(x), C.byref(y), C.byref(b)))
        return x.value, y.value, b.value

    def _shape(self, field, count):
        _, nc = _FIELD_SPEC[field]
        return (count, self.dim_y, self.dim_x, nc) if nc > 1 else (count, self.dim_y, self.dim_x)

    def upload(self, field: int, a: np.ndarray, first: int = 0):
        """Members [first, first + len(a)) of a field (synchronous)."""
        dt, _ = _FIELD_SPEC[field]
        a = np.ascontiguousarray(a, dtype=dt)
        if a.shape[1:] != self._shape(field, 0)[1:]:
            raise ValueError(f"field {field}: shape {a.shape}, a batch member wants {self._shape(field, 0)[1:]}")
        capi.check(self._lib.sfl_batch_upload(self._h, field, first, a.shape[0], a.ctypes.data, a.nbytes))

    def download(self, field: int, first: int = 0, count=None) -> np.ndarray:
        """Members [first, first + count) of a field (synchronous; count None = to the end of the batch)."""
        dt, _ = _FIELD_SPEC[field]
        count = self.batch - first if count is None else count
        a = np.empty(self._shape(field, max(count, 0)), dt)
        capi.check(self._lib.sfl_batch_download(self._h, field, first, count, a.ctypes.data, a.nbytes))
        return a

    def device_ptr(self, field: int) -> int:
        """Member 0 of the field's current buffer (valid until the next step)."""
        p = C.c_void_p()
        capi.check(self._lib.sfl_batch_field_device_ptr(self._h, field, C.byref(p)))
        return p.value

    def queue_forces(self, members, cells_ij, vel_xy, step: int = 0):
        """Point forces of step `step` of the steps to come (0: the next one; the timeline rule of include/sfl.h): record k
        sets member members[k]'s velocity at cell cells_ij[k] to vel_xy[k]."""
        members = np.ascontiguousarray(members, np.int32).reshape(-1)
        cells = np.ascontiguousarray(cells_ij, np.int32).reshape(-1, 2)
        vel = np.ascontiguousarray(vel_xy, np.float32).reshape(-1, 2)
        if not len(members) == len(cells) == len(vel):
            raise ValueError("members, cells_ij and vel_xy need one entry per force")
        capi.check(self._lib.sfl_batch_queue_forces_at(
            self._h, step, members.ctypes.data_as(C.POINTER(C.c_int)), cells.ctypes.data_as(C.POINTER(C.c_int)),
            vel.ctypes.data_as(C.POINTER(C.c_float)), len(members)))

    def forces_pending(self):
        """(records, last_step) of the timeline of queued forces; last_step is -1 when it is empty."""
        records, last = C.c_int(0), C.c_int(0)
        capi.check(self._lib.sfl_batch_forces_pending(self._h, C.byref(records), C.byref(last)))
        return records.value, last.value

    def forget_forces(self):
        """Empties the timeline of queued forces."""
        capi.check(self._lib.sfl_batch_forget_forces(self._h))

    def step_n(self, n, dt, dx=1.0, iters=10, omega=1.96):
        capi.check(self._lib.sfl_batch_step_n(self._h, n, dt, dx, iters, omega))

    def step(self, dt, dx=1.0, iters=10, omega=1.96):
        self.step_n(1, dt, dx, iters, omega)

    def poisson_solve(self, dx=1.0, iters=10, omega=1.96):
        capi.check(self._lib.sfl_batch_poisson_solve(self._h, dx, iters, omega))

    def _member_params(self, first, *rest):
        """`first` a ready-made member_params array, or the arguments of member_params after `batch`."""
        if isinstance(first, np.ndarray) and first.dtype.names:
            if first.dtype != MEMBER_PARAMS_DTYPE or first.shape != (self.batch,):
                raise ValueError(f"member parameters: want {self.batch} records of {MEMBER_PARAMS_DTYPE}, got "
                                 f"{first.shape} of {first.dtype}")
            prm = np.ascontiguousarray(first)
        else:
            prm = member_params(self.batch, first, *rest)
        return prm, prm.ctypes.data_as(C.POINTER(capi.MemberParams))

    def step_n_each(self, n, dt, dx=1.0, iters=10, omega=1.96):
        """step_n with parameters of each member's own: every argument a scalar or a sequence of `batch` values, or
        `dt` a ready-made :func:`member_params` array (the others are then ignored).  Leaves ``residual()``."""
        prm, ptr = self._member_params(dt, dx, iters, omega)
        capi.check(self._lib.sfl_batch_step_n_each(self._h, n, ptr))

    def poisson_solve_each(self, dx=1.0, iters=10, omega=1.96):
        """poisson_solve with each member's own dx, iters and omega (scalars or sequences of `batch` values), or `dx` a
        ready-made :func:`member_params` array (its dt is ignored).  Leaves ``residual()``."""
        if not (isinstance(dx, np.ndarray) and dx.dtype.names):
            dx = member_params(self.batch, 0.0, dx, iters, omega)
        prm, ptr = self._member_params(dx)
        capi.check(self._lib.sfl_batch_poisson_solve_each(self._h, ptr))

    def _member_stops(self, tol, every):
        """`tol` a ready-made member_stops array, or the arguments of member_stops after `batch`."""
        if tol is None:
            raise ValueError("tol: a scalar, a sequence of one value per member or a member_stops array is required")
        if isinstance(tol, np.ndarray) and tol.dtype.names:
            if tol.dtype != MEMBER_STOP_DTYPE or tol.shape != (self.batch,):
                raise ValueError(f"member stops: want {self.batch} records of {MEMBER_STOP_DTYPE}, got {tol.shape} of "
                                 f"{tol.dtype}")
            stops = np.ascontiguousarray(tol)
        else:
            stops = member_stops(self.batch, tol, every)
        return stops, stops.ctypes.data_as(C.POINTER(capi.MemberStop))

    def step_n_until(self, n, dt, dx=1.0, max_iters=10, omega=1.96, tol=None, every=4):
        """step_n_each with every step's pressure solve stopped by each member's own rule (include/sfl.h
        sfl_member_stop): in front of every `every`-th iteration the update norm is checked, and the solve ends at the
        first check that finds it <= `tol` (or a NaN), at `max_iters` at the latest.  Arguments: scalars or sequences of
        `batch` values; `dt` may be a ready-made :func:`member_params` array (its iters is the cap; dx, max_iters and omega
        are then ignored) and `tol` (required) a ready-made :func:`member_stops` array (every is then ignored).  Leaves ``residual()`` and
        ``iterations()``."""
        prm, ptr = self._member_params(dt, dx, max_iters, omega)
        stops, sptr = self._member_stops(tol, every)
        capi.check(self._lib.sfl_batch_step_n_until(self._h, n, ptr, sptr))

    def poisson_solve_until(self, dx=1.0, max_iters=10, omega=1.96, tol=None, every=4):
        """poisson_solve_each stopped by each member's own rule (see :meth:`step_n_until`); `dx` may be a ready-made
        :func:`member_params` array (its dt is ignored), `tol` a ready-made :func:`member_stops` array."""
        if not (isinstance(dx, np.ndarray) and dx.dtype.names):
            dx = member_params(self.batch, 0.0, dx, max_iters, omega)
        prm, ptr = self._member_params(dx)
        stops, sptr = self._member_stops(tol, every)
        capi.check(self._lib.sfl_batch_poisson_solve_until(self._h, ptr, sptr))

    def iterations(self, first: int = 0, count=None) -> np.ndarray:
        """The iterations of members [first, first + count) as the last ``*_until`` call left them, int32[count, 2]: those
        of the member's last solve, and their sum over the steps of that call.  Synchronous; SflError with ERR_STATE
        when the last call that wrote the pressure was not an ``*_until`` call."""
        count = self.batch - first if count is None else count
        a = np.empty((max(count, 0), 2), np.int32)
        capi.check(self._lib.sfl_batch_iterations(self._h, first, count, a.ctypes.data_as(C.POINTER(C.c_int32)), a.nbytes))
        return a

    def residual(self, first: int = 0, count=None) -> np.ndarray:
        """The update norm of members [first, first + count) as the last ``*_each`` or ``*_until`` call left it, float32[count]:
        max |p_gs - p| over the member's cells on its final pressure, a NaN for a member that diverged to one
        (include/sfl.h sfl_batch_residual).  Synchronous; SflError with ERR_STATE when no ``*_each`` call wrote it."""
        count = self.batch - first if count is None else count
        a = np.empty(max(count, 0), np.float32)
        capi.check(self._lib.sfl_batch_residual(self._h, first, count, _fp(a), a.nbytes))
        return a

    def flow_stats(self, dx=1.0, first: int = 0, count=None, velocity=True, dye=True) -> np.ndarray:
        """The flow statistics of members [first, first + count) (sfl_batch_flow_stats[_each]; the definitions of
        :meth:`Solver.flow_stats`): a FLOW_STATS_DTYPE array of `count` records.  `dx` a scalar, or a sequence of `batch`
        values: member m's divergence is then scaled by its own.  A member reports what a context holding the same fields
        reports.  One launch per part asked for, whatever the range; reads only (``residual()`` and ``iterations()``
        stay valid); synchronous."""
        what = _stats_what(velocity, dye)
        count = self.batch - first if count is None else count
        out = np.zeros(max(count, 0), FLOW_STATS_DTYPE)
        ptr = out.ctypes.data_as(C.POINTER(capi.FlowStats))
        if np.ndim(dx) == 0:
            capi.check(self._lib.sfl_batch_flow_stats(self._h, what, dx, first, count, ptr, out.nbytes))
        else:
            prm, pptr = self._member_params(0.0, dx, 0, 0.0)
            capi.check(self._lib.sfl_batch_flow_stats_each(self._h, what, pptr, first, count, ptr, out.nbytes))
        return out

    def distance(self, ref=None, ref_member=None, first: int = 0, count=None, velocity=True, dye=True,
                 pressure=True) -> np.ndarray:
        """The distance of members [first, first + count) from a reference (sfl_batch_distance; the definitions of
        :meth:`Solver.distance`): a FIELD_DISTANCE_DTYPE array of `count` records.  Record k is member first + k against
        member `ref_member` of `ref`, or, with ``ref_member=None``, against member first + k of `ref`: the pairwise form,
        for twins.  ``ref=None`` is this batch; `ref` may be the other kind of batch of the same shape.  One launch per
        part asked for, whatever the range; reads only (``residual()`` and ``iterations()`` stay valid); synchronous."""
        what = _dist_what(velocity, dye, pressure)
        count = self.batch - first if count is None else count
        out = np.zeros(max(count, 0), FIELD_DISTANCE_DTYPE)
        capi.check(self._lib.sfl_batch_distance(self._h, what, None if ref is None else ref._h,
                                                -1 if ref_member is None else ref_member, first, count,
                                                out.ctypes.data_as(C.POINTER(capi.FieldDistance)), out.nbytes))
        return out

    def envelope(self, first: int = 0, count=None):
        """Take the per-cell envelope of the CURRENT dye over members [first, first + count) (sfl_batch_envelope): mean
        (floor of the exact sum over count), minimum, maximum and spread = max - min of every cell and channel, exact
        integers.  A snapshot kept on the device: later steps do not change it, the next call replaces it.
        Asynchronous; count None = to the end of the batch."""
        count = self.batch - first if count is None else count
        capi.check(self._lib.sfl_batch_envelope(self._h, first, count))

    def envelope_info(self):
        """(first, count) of the snapshot held; count 0: none yet.  Never waits."""
        first, count = C.c_int(0), C.c_int(0)
        capi.check(self._lib.sfl_batch_envelope_info(self._h, C.byref(first), C.byref(count)))
        return first.value, count.value

    def envelope_field(self, which: int) -> np.ndarray:
        """Field `which` (capi.ENV_MEAN / ENV_MIN / ENV_MAX / ENV_SPREAD) of the snapshot, uint32[dim_y, dim_x, 3] laid
        out as a context's dye.  Synchronous."""
        a = np.empty((self.dim_y, self.dim_x, 3), np.uint32)
        capi.check(self._lib.sfl_batch_envelope_download(self._h, which, _up(a), a.nbytes))
        return a

    def envelope_render(self, which: int, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """Field `which` of the snapshot -> RGB565 image, bit for bit what ``Solver.render_rgb565`` draws for a context
        whose dye is that field.  Synchronous."""
        img = np.empty((max(scaling, 0) * (self.dim_x - 1), max(scaling, 0) * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_batch_envelope_render(self._h, which, scaling, int(byteswap),
                                                       img.ctypes.data_as(C.POINTER(C.c_uint16)), img.nbytes))
        return img

    def setup_sketch_fields(self):
        """Every member: velocity = 0, dye = the sketch's blurred three-sector pattern (setup(), ino:196-241)."""
        capi.check(self._lib.sfl_batch_setup_sketch_fields(self._h))

    def render_rgb565(self, member: int, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """One member's dye -> RGB565 image, uint16[scaling*(dim_x-1), scaling*(dim_y-1)] (ino:116-176)."""
        img = np.empty((scaling * (self.dim_x - 1), scaling * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_batch_render_rgb565(self._h, member, scaling, int(byteswap),
                                                     img.ctypes.data_as(C.POINTER(C.c_uint16)), img.nbytes))
        return img

    def render_members(self, first: int = 0, count=None, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """The dye of members [first, first + count) -> RGB565 images, uint16[count, H, W] with H = scaling*(dim_x-1) and
        W = scaling*(dim_y-1): image k is ``render_rgb565(first + k)`` bit for bit, all of them from one launch and one
        copy (sfl_batch_render_members).  Synchronous; count None = to the end of the batch."""
        count = self.batch - first if count is None else count
        img = np.empty((max(count, 0), max(scaling, 0) * (self.dim_x - 1), max(scaling, 0) * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_batch_render_members(self._h, first, count, scaling, int(byteswap),
                                                      img.ctypes.data_as(C.POINTER(C.c_uint16)), img.nbytes))
        return img

    def record_start(self, every: int = 1, first: int = 0, count=None, scaling: int = 4, byteswap: bool = True,
                     capacity: int = 64):
        """Start the recorder (sfl_batch_record_start): from now on every `every`-th step of ``step_n``, ``step_n_each``
        and ``step_n_until`` -- counted across calls -- leaves a frame of members [first, first + count) in device memory,
        rendered between the step launches without a wait; `capacity` frames fit (device memory: capacity * count * H * W
        * 2 bytes).  A step call that would complete more frames than are free raises SflError with ERR_STATE and steps
        nothing: read the frames (:meth:`frames`) and call record_start again.  Called while recording, it starts afresh."""
        count = self.batch - first if count is None else count
        rc = self._lib.sfl_batch_record_start(self._h, every, first, count, scaling, int(byteswap), capacity)
        if rc == capi.OK:
            self._rec = (first, count, scaling)
        elif self.record_info()[1] == 0:   # a failed allocation: the batch is not recording any more
            self._rec = (0, 0, 1)
        capi.check(rc)

    def record_stop(self):
        """Stop recording and free the frames."""
        capi.check(self._lib.sfl_batch_record_stop(self._h))
        self._rec = (0, 0, 1)

    def record_info(self):
        """(frames written, capacity, steps counted since record_start); (0, 0, 0) when not recording.  Never waits."""
        frames, capacity, steps = C.c_int(), C.c_int(), C.c_int64()
        capi.check(self._lib.sfl_batch_record_info(self._h, C.byref(frames), C.byref(capacity), C.byref(steps)))
        return frames.value, capacity.value, steps.value

    def frames(self, frame_first: int = 0, frame_count=None, first=None, count=None) -> np.ndarray:
        """Recorded frames [frame_first, frame_first + frame_count) of members [first, first + count), uint16[F, count, H, W]
        (sfl_batch_record_read; frames are not consumed).  Defaults: every frame written so far, the recorded members.
        Member numbers are the batch's.  Synchronous; an empty array when there is nothing to read."""
        written, _, _ = self.record_info()
        rec_first, rec_count, scaling = self._rec
        frame_count = written - frame_first if frame_count is None else frame_count
        first = rec_first if first is None else first
        count = rec_first + rec_count - first if count is None else count
        out = np.empty((max(frame_count, 0), max(count, 0), scaling * (self.dim_x - 1), scaling * (self.dim_y - 1)), np.uint16)
        for f in range(max(frame_count, 0)):
            capi.check(self._lib.sfl_batch_record_read(self._h, frame_first + f, first, count,
                                                       out[f].ctypes.data_as(C.POINTER(C.c_uint16)), out[f].nbytes))
        return out

    # -- views ---------------------------------------------------------------------------
    def _view_count(self, first, count):
        return self.batch - first if count is None else count

    def view_scalar(self, what: int, dx: float = 1.0, first: int = 0, count=None) -> np.ndarray:
        """Speed, vorticity, pressure or divergence (capi.VIEW_*) of members [first, first + count), float32[count, dim_y,
        dim_x], from one launch and one copy."""
        count = self._view_count(first, count)
        out = np.empty((max(count, 0), self.dim_y, self.dim_x), np.float32)
        capi.check(self._lib.sfl_batch_view_scalar(self._h, what, dx, first, count, out.ctypes.data_as(C.POINTER(C.c_float)), out.nbytes))
        return out

    def view_texels(self, view: View, first: int = 0, count=None) -> np.ndarray:
        """The node colours of a view of members [first, first + count), uint32[count, dim_y, dim_x, 3]."""
        count = self._view_count(first, count)
        out = np.empty((max(count, 0), self.dim_y, self.dim_x, 3), np.uint32)
        capi.check(self._lib.sfl_batch_view_texels(self._h, C.byref(view.struct()), first, count,
                                                   out.ctypes.data_as(C.POINTER(C.c_uint32)), out.nbytes))
        return out

    def view_render_members(self, view: View, first: int = 0, count=None, scaling: int = 4, byteswap: bool = True) -> np.ndarray:
        """A view of members [first, first + count) -> RGB565 images shaped as :meth:`render_members`'s, one launch."""
        count = self._view_count(first, count)
        img = np.empty((max(count, 0), max(scaling, 0) * (self.dim_x - 1), max(scaling, 0) * (self.dim_y - 1)), np.uint16)
        capi.check(self._lib.sfl_batch_view_render_members(self._h, C.byref(view.struct()), first, count, scaling, int(byteswap),
                                                           _u16p(img), img.nbytes))
        return img

    def record_view(self, view=None):
        """What the recorder draws from the next frame on: a :class:`View`, or the dye (None).  Only while recording;
        record_start and record_stop reset it to the dye.  The view is copied: it may be dropped after the call."""
        capi.check(self._lib.sfl_batch_record_view(self._h, None if view is None else C.byref(view.struct())))

    def set_solids(self, mask):
        """Solid cells inside the members' grids (include/sfl.h "SOLIDS"): `mask` a bool or uint8 array, nonzero = solid,
        of shape ``(dim_y, dim_x)`` -- one mask for all members -- or ``(batch, dim_y, dim_x)``; None clears the solids.
        No field is touched.  Batches of small members only; step_n, step_n_each, poisson_solve[_each] and flow_stats
        then follow the solids' rule, the ``_until`` calls, histories and the divergence view are refused while set."""
        if mask is None:
            capi.check(self._lib.sfl_batch_set_solids(self._h, None, 0))
            return
        mask = np.asarray(mask)
        if mask.dtype != np.bool_ and mask.dtype != np.uint8:
            raise ValueError(f"solids: a bool or uint8 mask, got {mask.dtype}")
        if mask.shape not in ((self.dim_y, self.dim_x), (self.batch, self.dim_y, self.dim_x)):
            raise ValueError(f"solids: shape {mask.shape}, want {(self.dim_y, self.dim_x)} or {(self.batch, self.dim_y, self.dim_x)}")
        m = np.ascontiguousarray(mask != 0, dtype=np.uint8)
        capi.check(self._lib.sfl_batch_set_solids(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), int(m.ndim == 3)))

    def solids_info(self):
        """(set, per_member) as the library reports it."""
        s, p = C.c_int(0), C.c_int(0)
        capi.check(self._lib.sfl_batch_solids_info(self._h, C.byref(s), C.byref(p)))
        return bool(s.value), bool(p.value)

    def solids(self, first: int = 0, count=None) -> np.ndarray:
        """The masks of members [first, first + count), bool[count, dim_y, dim_x]: all False without solids, a shared
        mask repeated.  Synchronous."""
        count = self.batch - first if count is None else count
        a = np.zeros((max(count, 0), self.dim_y, self.dim_x), np.uint8)
        capi.check(self._lib.sfl_batch_solids_download(self._h, first, count, a.ctypes.data_as(C.POINTER(C.c_uint8)), a.nbytes))
        return a.astype(bool)

    def set_viscosity(self, nu, sweeps: int):
        """Viscosity (include/sfl.h "VISCOSITY"): `nu` one number for all members or an array of `batch`; None clears it.
        step_n and step_n_each then run `sweeps` sweeps of an implicit diffusion of the velocity between the forces and
        the divergence, with and without solids; members with nu == 0 skip it.  Batches of small members only; the
        ``_until`` step is refused while set."""
        if nu is None:
            capi.check(self._lib.sfl_batch_set_viscosity(self._h, None, 0, int(sweeps)))
            return
        a = np.asarray(nu, dtype=np.float32)
        if a.shape not in ((), (self.batch,)):
            raise ValueError(f"viscosity: nu of shape {a.shape}, want a number or {(self.batch,)}")
        per_member = a.ndim == 1
        a = np.ascontiguousarray(a.reshape(-1))
        capi.check(self._lib.sfl_batch_set_viscosity(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), int(per_member), int(sweeps)))

    def viscosity(self):
        """(nu of every member, float32[batch] -- zeros when none is set --, sweeps)."""
        s = C.c_int(0)
        capi.check(self._lib.sfl_batch_viscosity_info(self._h, None, None, C.byref(s)))
        a = np.zeros(self.batch, np.float32)
        capi.check(self._lib.sfl_batch_viscosity_download(self._h, 0, self.batch, a.ctypes.data_as(C.POINTER(C.c_float)), a.nbytes))
        return a, s.value

    def _inflow(self, inflow):
        a = np.asarray(inflow, dtype=np.float32)
        if a.shape not in ((2,), (self.batch, 2)):
            raise ValueError(f"openings: inflow of shape {a.shape}, want (2,) or {(self.batch, 2)}")
        return np.ascontiguousarray(a.reshape(-1)), int(a.ndim == 2)

    def set_openings(self, open, inflow=(0.0, 0.0)):
        """Inflow and outflow cells on the rim of the members' grids (include/sfl.h "OPENINGS"): `open` a uint8 array of
        0, OPEN_INFLOW and OPEN_OUTFLOW of shape ``(dim_y, dim_x)`` -- one map for all members -- or ``(batch, dim_y,
        dim_x)``, nonzero only on rim cells that are no corners; `inflow` one ``(u, v)`` for all members or an array
        ``(batch, 2)``; None clears the openings.  No field is touched.  Batches of small members only; step_n,
        step_n_each, poisson_solve[_each] and flow_stats then follow the openings' rule, with and without solids; the
        ``_until`` calls, histories, the divergence view and viscosity are refused while set."""
        if open is None:
            capi.check(self._lib.sfl_batch_set_openings(self._h, None, 0, None, 0))
            return
        m = np.asarray(open)
        if m.dtype != np.uint8:
            raise ValueError(f"openings: a uint8 map, got {m.dtype}")
        if m.shape not in ((self.dim_y, self.dim_x), (self.batch, self.dim_y, self.dim_x)):
            raise ValueError(f"openings: shape {m.shape}, want {(self.dim_y, self.dim_x)} or {(self.batch, self.dim_y, self.dim_x)}")
        a, each = self._inflow(inflow)
        m = np.ascontiguousarray(m)
        capi.check(self._lib.sfl_batch_set_openings(self._h, m.ctypes.data_as(C.POINTER(C.c_uint8)), int(m.ndim == 3),
                                                    a.ctypes.data_as(C.POINTER(C.c_float)), each))

    def set_inflow(self, inflow):
        """Change the inflow velocity of a batch with openings set: one ``(u, v)`` or an array ``(batch, 2)``.  The map stays."""
        a, each = self._inflow(inflow)
        capi.check(self._lib.sfl_batch_set_inflow(self._h, a.ctypes.data_as(C.POINTER(C.c_float)), each))

    def openings_info(self):
        """(set, per_member, inflow_per_member, live inflow cells, live outflow cells) as the library reports it."""
        s, p, q, n_in, n_out = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int64(0), C.c_int64(0)
        capi.check(self._lib.sfl_batch_openings_info(self._h, C.byref(s), C.byref(p), C.byref(q), C.byref(n_in), C.byref(n_out)))
        return bool(s.value), bool(p.value), bool(q.value), n_in.value, n_out.value

    def openings(self, first: int = 0, count=None):
        """(the maps of members [first, first + count), uint8[count, dim_y, dim_x]; their inflow, float32[count, 2]): zeros
        without openings, a shared map or inflow repeated."""
        count = self.batch - first if count is None else count
        m = np.zeros((max(count, 0), self.dim_y, self.dim_x), np.uint8)
        capi.check(self._lib.sfl_batch_openings_download(self._h, first, count, m.ctypes.data_as(C.POINTER(C.c_uint8)), m.nbytes))
        a = np.zeros((max(count, 0), 2), np.float32)
        capi.check(self._lib.sfl_batch_inflow_download(self._h, first, count, a.ctypes.data_as(C.POINTER(C.c_float)), a.nbytes))
        return m, a

    def set_inflow_profile(self, cells, vel, members=None):
        """A per-cell inflow profile (include/sfl.h "INFLOW PROFILES AND FLUX"): `cells` integers ``(n, 2)``, (i, j) per
        record; `vel` float32 ``(n, 2)``; `members` None -- every record to every member -- or ``n`` member numbers, record k
        to member members[k] (one batch is then a sweep over the profile).  Each record names a cell whose map byte is
        OPEN_INFLOW in every member it applies to.  Of two records on one cell of one member the later wins; n == 0 (or
        None) clears the profile; a new map drops it, set_inflow keeps it."""
        c, v = _profile_records([] if cells is None else cells, [] if vel is None else vel)
        who = None
        if members is not None and len(c):
            w = np.asarray(members)
            if w.shape != (len(c),) or not np.issubdtype(w.dtype, np.integer):
                raise ValueError(f"inflow profile: members of shape {w.shape} and dtype {w.dtype}, want {(len(c),)} integers")
            w = np.ascontiguousarray(w, np.int32)
            who = w.ctypes.data_as(C.POINTER(C.c_int))
        capi.check(self._lib.sfl_batch_set_inflow_profile(self._h, who, c.ctypes.data_as(C.POINTER(C.c_int)),
                                                          v.ctypes.data_as(C.POINTER(C.c_float)), len(c)))

    def inflow_profile(self, member: int = 0):
        """(cells int32[n, 2], vel float32[n, 2]): the records of one member, in cell-index order; empty without a profile."""
        n = C.c_int(0)
        rc = self._lib.sfl_batch_inflow_profile_download(self._h, member, None, None, 0, C.byref(n))   # (no room: the count alone)
        if rc != capi.OK and n.value == 0:
            capi.check(rc)
        c, v = np.zeros((n.value, 2), np.int32), np.zeros((n.value, 2), np.float32)
        capi.check(self._lib.sfl_batch_inflow_profile_download(self._h, member, c.ctypes.data_as(C.POINTER(C.c_int)),
                                                               v.ctypes.data_as(C.POINTER(C.c_float)), n.value, None))
        return c, v

    def inflow_profile_info(self):
        """(set, unique cells held over all members) as the library reports it.  Never waits."""
        s, n = C.c_int(0), C.c_int64(0)
        capi.check(self._lib.sfl_batch_inflow_profile_info(self._h, C.byref(s), C.byref(n)))
        return bool(s.value), n.value

    def openings_flux(self, first: int = 0, count=None) -> np.ndarray:
        """The flux through the live open cells of members [first, first + count) from the velocity held: an
        OPEN_FLUX_DTYPE array of shape ``(count,)``; exact integers, see :func:`openings_flux_xy`.  All zeros without
        openings.  One launch, one workgroup per member over its rim; synchronous."""
        count = self.batch - first if count is None else count
        out = np.zeros((max(count, 0),), OPEN_FLUX_DTYPE)
        capi.check(self._lib.sfl_batch_openings_flux(self._h, first, count, out.ctypes.data_as(C.POINTER(capi.OpenFlux)), out.nbytes))
        return out

    def set_wall_velocity(self, cells, vel, members=None):
        """Wall velocities (include/sfl.h "WALL VELOCITIES"): `cells` integers ``(n, 2)``, (i, j) per record; `vel` float32
        ``(n, 2)``; `members` None -- every record to every member -- or ``n`` member numbers, record k to member
        members[k] (one batch is then a sweep over the wall's speed).  Each record names a cell that is SOLID in the mask
        of every member it applies to.  Of two records on one cell of one member the later wins; n == 0 (or None) clears
        the table; every set_solids drops it."""
        c, v = _profile_records([] if cells is None else cells, [] if vel is None else vel, "wall velocity")
        who = None
        if members is not None and len(c):
            w = np.asarray(members)
            if w.shape != (len(c),) or not np.issubdtype(w.dtype, np.integer):
                raise ValueError(f"wall velocity: members of shape {w.shape} and dtype {w.dtype}, want {(len(c),)} integers")
            w = np.ascontiguousarray(w, np.int32)
            who = w.ctypes.data_as(C.POINTER(C.c_int))
        capi.check(self._lib.sfl_batch_set_wall_velocity(self._h, who, c.ctypes.data_as(C.POINTER(C.c_int)),
                                                         v.ctypes.data_as(C.POINTER(C.c_float)), len(c)))

    def wall_velocity(self, member: int = 0):
        """(cells int32[n, 2], vel float32[n, 2]): the records of one member, in cell-index order; empty without a table."""
        n = C.c_int(0)
        capi.check(self._lib.sfl_batch_wall_velocity_download(self._h, member, None, None, 0, C.byref(n)))   # (no arrays: the count alone)
        c, v = np.zeros((n.value, 2), np.int32), np.zeros((n.value, 2), np.float32)
        capi.check(self._lib.sfl_batch_wall_velocity_download(self._h, member, c.ctypes.data_as(C.POINTER(C.c_int)),
                                                              v.ctypes.data_as(C.POINTER(C.c_float)), n.value, None))
        return c, v

    def wall_velocity_info(self):
        """(set, unique cells held over all members, a shared table counted once per member).  Never waits."""
        s, n = C.c_int(0), C.c_int64(0)
        capi.check(self._lib.sfl_batch_wall_velocity_info(self._h, C.byref(s), C.byref(n)))
        return bool(s.value), n.value

    def synchronize(self):
        capi.check(self._lib.sfl_batch_synchronize(self._h))


def rigid_wall_velocity(labels, body: int, u=0.0, v=0.0, omega=0.0, pivot2=(0, 0)):
    """(cells int32[n, 2], vel float32[n, 2]) for set_wall_velocity: every cell of `labels` (integers ``(dim_y, dim_x)``,
    the bodies' labels) that carries `body` moves as one rigid body -- translation (u, v) plus rotation `omega` (radians per
    unit time, counter-clockwise) about the pivot, given in HALF CELLS as the torque's pivots are.  Per cell (i, j), every
    operation one float32 rounding: rx = 0.5f * (2 i - px2), ry = 0.5f * (2 j - py2), wu = u - omega * ry, wv = v + omega * rx.
    Cells in cell-index order."""
    lab = np.asarray(labels)
    if lab.ndim != 2 or not np.issubdtype(lab.dtype, np.integer):
        raise ValueError(f"rigid wall velocity: labels of shape {lab.shape} and dtype {lab.dtype}, want integers (dim_y, dim_x)")
    F = np.float32
    j, i = np.nonzero(lab == body)
    rx = F(0.5) * (2 * i.astype(np.int64) - int(pivot2[0])).astype(F)
    ry = F(0.5) * (2 * j.astype(np.int64) - int(pivot2[1])).astype(F)
    wu = (F(u) - (F(omega) * ry).astype(F)).astype(F)
    wv = (F(v) + (F(omega) * rx).astype(F)).astype(F)
    return np.stack([i, j], axis=1).astype(np.int32), np.stack([wu, wv], axis=1).astype(F)


def wall_shares(solid, labels, bodies: int, pivot2, cells, vel):
    """The wall's share of the friction and of the friction torque of every body, in float64, from a mask (bool ``(dim_y,
    dim_x)``), the labels (integers, same shape; a label counts only where the cell is solid), the pivots in HALF cells
    (integers ``(bodies, 2)``) and a wall table (`cells` ``(n, 2)``, `vel` ``(n, 2)``, unique cells): over the wet faces of a
    body -- a solid cell of it and a fluid neighbour W, E, S or N of it -- the sum of the SOLID cell's tangential wall velocity
    (v across a W or E face, u across an S or N face; 0 for a cell no record names), for the torque times the face's arm:
    +rx * v across W and E, -ry * u across S and N, (rx, ry) = (i - px2 / 2, j - py2 / 2) of the solid cell.  Returns
    (float64 ``(bodies, 2)``: x from the S and N faces, y from the W and E faces; float64 ``(bodies,)``) -- what
    fx * 2^exp2, fy * 2^exp2 and mf * 2^(exp2_f - 1) of "FRICTION" and "TORQUE" would be if the fluid moved with the wall."""
    solid = np.asarray(solid, bool)
    lab = np.where(solid, np.asarray(labels).astype(np.int64), 0)
    wall = np.zeros(solid.shape + (2,), np.float64)
    c = np.asarray(cells, np.int64).reshape(-1, 2)
    wall[c[:, 1], c[:, 0]] = np.asarray(vel, np.float64).reshape(-1, 2)
    piv = np.asarray(pivot2, np.float64).reshape(bodies, 2)
    j, i = np.mgrid[0:solid.shape[0], 0:solid.shape[1]]
    fluid = ~solid
    # the fluid neighbour W, E, S, N of every cell is inside the domain and fluid
    wet = [np.zeros_like(solid) for _ in range(4)]
    wet[0][:, 1:], wet[1][:, :-1], wet[2][1:, :], wet[3][:-1, :] = fluid[:, :-1], fluid[:, 1:], fluid[:-1, :], fluid[1:, :]
    friction, torque = np.zeros((bodies, 2), np.float64), np.zeros(bodies, np.float64)
    for b in range(1, bodies + 1):
        mine = lab == b
        rx, ry = i - piv[b - 1, 0] / 2.0, j - piv[b - 1, 1] / 2.0
        for d in range(4):
            face = mine & wet[d]
            if d < 2:   # W, E: the fluid slides along y
                friction[b - 1, 1] += wall[face, 1].sum()
                torque[b - 1] += (rx[face] * wall[face, 1]).sum()
            else:       # S, N: along x
                friction[b - 1, 0] += wall[face, 0].sum()
                torque[b - 1] -= (ry[face] * wall[face, 0]).sum()
    return friction, torque


def _profile_records(cells, vel, what="inflow profile"):
    """(cells int32[n, 2], vel float32[n, 2]) of an inflow profile or a wall table, checked for shape before the library sees them."""
    c = np.asarray(cells)
    v = np.asarray(vel, dtype=np.float32)
    if c.size == 0 and v.size == 0:
        return np.zeros((0, 2), np.int32), np.zeros((0, 2), np.float32)
    if c.ndim != 2 or c.shape[1] != 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"{what}: cells of shape {c.shape} and dtype {c.dtype}, want integers (n, 2): (i, j) per record")
    if v.shape != c.shape:
        raise ValueError(f"{what}: vel of shape {v.shape}, want {c.shape}: (u, v) per record")
    return np.ascontiguousarray(c, np.int32), np.ascontiguousarray(v)


def openings_flux_xy(flux) -> np.ndarray:
    """OPEN_FLUX_DTYPE record(s) as float64 ``(..., 2)``: inflow * 2^exp2 and outflow * 2^exp2, in velocity times cell widths
    (multiply by dx).  Exact: an integer below 2^49 times a power of two."""
    f = np.asarray(flux)
    return np.stack([np.ldexp(f["inflow"].astype(np.float64), f["exp2"]), np.ldexp(f["outflow"].astype(np.float64), f["exp2"])], axis=-1)


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _up(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


class HostPath:
    """The reference's operators on host arrays, executed by the HIP kernels.

    Same method names / argument order / return conventions as ``oracle.loader.CpuPath`` so the
    parity tests read identically for the checker and the product.  ``sor_kernel`` / ``sor_fuse``
    select the SOR implementation (0 = auto)."""

    kind = "hip"

    def __init__(self, device: int = 0, sor_kernel: int = 0, sor_fuse: int = 0, sor_rows: int = 0,
                 sor_lane_cells: int = 0, sor_fold: int = 0):
        self._lib = capi.lib()
        self.device, self.sor_kernel, self.sor_fuse, self.sor_rows = device, sor_kernel, sor_fuse, sor_rows
        self.sor_lane_cells, self.sor_fold = sor_lane_cells, sor_fold

    @staticmethod
    def _dims(a):
        return int(a.shape[1]), int(a.shape[0])

    def _solver(self, dim_x, dim_y) -> Solver:
        s = Solver(dim_x, dim_y, self.device)
        if self.sor_kernel:
            s.set_option(capi.OPT_SOR_KERNEL, self.sor_kernel)
        if self.sor_fuse:
            s.set_option(capi.OPT_SOR_FUSE, self.sor_fuse)
        if self.sor_rows:
            s.set_option(capi.OPT_SOR_ROWS, self.sor_rows)
        if self.sor_lane_cells:
            s.set_option(capi.OPT_SOR_LANE_CELLS, self.sor_lane_cells)
        if self.sor_fold:
            s.set_option(capi.OPT_SOR_FOLD, self.sor_fold)
        return s

    def advect_vec2f(self, p, vel, dt, no_slip=True):
        dim_x, dim_y = self._dims(vel)
        p, vel = np.ascontiguousarray(p, np.float32), np.ascontiguousarray(vel, np.float32)
        out = np.empty_like(p)
        # keep the aliasing information: self-advection passes the same pointer twice (ino:253)
        pp = _fp(vel) if p is vel or (p.ctypes.data == vel.ctypes.data) else _fp(p)
        capi.check(self._lib.sfl_host_advect_vec2f(_fp(out), pp, _fp(vel), dim_x, dim_y, dt,
                                                   int(no_slip)))
        return out

    def advect_vec3uq32(self, p, vel, dt, no_slip=False):
        dim_x, dim_y = self._dims(vel)
        p, vel = np.ascontiguousarray(p, np.uint32), np.ascontiguousarray(vel, np.float32)
        out = np.empty_like(p)
        capi.check(self._lib.sfl_host_advect_vec3uq32(_up(out), _up(p), _fp(vel), dim_x, dim_y, dt,
                                                      int(no_slip)))
        return out

    def advect_channels(self, p, vel, dt, no_slip):
        """advect<T, float> for T = float / UQ32 / Vector2 / Vector3 of either (sfl_host_advect_channels): `p` is
        float32 or uint32 (UQ32 raw), shape [dim_y, dim_x] or [dim_y, dim_x, 2 | 3]."""
        dim_x, dim_y = self._dims(vel)
        if p.dtype not in (np.float32, np.uint32):
            raise TypeError("element channels are float32 or uint32 (UQ32 raw)")
        p, vel = np.ascontiguousarray(p), np.ascontiguousarray(vel, np.float32)
        channels = 1 if p.ndim == 2 else int(p.shape[2])
        out = np.empty_like(p)
        capi.check(self._lib.sfl_host_advect_channels(out.ctypes.data, p.ctypes.data, _fp(vel), dim_x, dim_y, dt,
                                                      int(no_slip), channels,
                                                      capi.CHANNEL_UQ32 if p.dtype == np.uint32 else capi.CHANNEL_F32))
        return out

    def divergence(self, v, dx=1.0):
        dim_x, dim_y = self._dims(v)
        v = np.ascontiguousarray(v, np.float32)
        out = np.empty((dim_y, dim_x), np.float32)
        capi.check(self._lib.sfl_host_calculate_divergence(_fp(out), _fp(v), dim_x, dim_y, dx))
        return out

    def subtract_gradient(self, v, p, dx=1.0):
        dim_x, dim_y = self._dims(v)
        out = np.array(v, np.float32, order="C", copy=True)
        p = np.ascontiguousarray(p, np.float32)
        capi.check(self._lib.sfl_host_subtract_gradient(_fp(out), _fp(p), dim_x, dim_y, dx))
        return out

    def poisson_solve(self, div, dx=1.0, iters=10, omega=1.96):
        dim_x, dim_y = self._dims(div)
        with self._solver(dim_x, dim_y) as s:
            s.upload(capi.FIELD_DIVERGENCE, div)
            s.poisson_solve(dx, iters, omega)
            s.synchronize()
            return s.download(capi.FIELD_PRESSURE)

    def step(self, v, colour, dt, dx=1.0, iters=10, omega=1.96):
        """One sim step (ino:252-287 order).  Returns (v, div, p, colour)."""
        dim_x, dim_y = self._dims(v)
        with self._solver(dim_x, dim_y) as s:
            s.upload(capi.FIELD_VELOCITY, v)
            s.upload(capi.FIELD_COLOR, colour)
            s.step(dt, dx, iters, omega)
            s.synchronize()
            return (s.download(capi.FIELD_VELOCITY), s.download(capi.FIELD_DIVERGENCE),
                    s.download(capi.FIELD_PRESSURE), s.download(capi.FIELD_COLOR))
