"""ctypes binding of the C ABI (include/sfl.h).  Mirrors the header one to one; no logic."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

_PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_PKG, "lib", "libsfl_hip.so")   # the one product library (A/B builds: tools/with_lib.py)

OK, ERR_INVALID, ERR_HIP, ERR_RCCL, ERR_NOMEM, ERR_STATE, ERR_HALO = 0, -1, -2, -3, -4, -5, -6
FIELD_VELOCITY, FIELD_COLOR, FIELD_DIVERGENCE, FIELD_PRESSURE = 0, 1, 2, 3
OPT_SOR_KERNEL, OPT_SOR_FUSE, OPT_ADVECT_HALO, OPT_SOR_ROWS, OPT_TRANSPORT = 0, 1, 2, 3, 4
OPT_SOR_LANE_CELLS = 5
OPT_SOR_HALO = 6
OPT_FUSE_PROJECTION = 7
OPT_ADVECT_KERNEL = 9
OPT_FUSE_DIVERGENCE = 10
OPT_SMALL_GRID = 11
OPT_EMULATE_WIRE_US = 12
OPT_STEP_SEAMS = 14
OPT_LAST_EARLY_ROWS = 17
OPT_HALO_TIMEOUT_MS = 18
OPT_EXCHANGE_SCHEDULE = 19
SCHEDULE_AUTO, SCHEDULE_IN_LINE, SCHEDULE_BY_EVENT, SCHEDULE_IN_TIME = 0, 1, 2, 3   # values of OPT_EXCHANGE_SCHEDULE
OPT_MEASURED_WIRE_US = 20
OPT_LAST_HALO = 21
OPT_SOR_FOLD = 22
CHANNEL_F32, CHANNEL_UQ32 = 0, 1
STEP_EXCHANGE, STEP_SOR, STEP_ZERO = 1, 2, 3
STATS_VELOCITY, STATS_DYE = 1, 2
DIST_VELOCITY, DIST_DYE, DIST_PRESSURE = 1, 2, 4
ENV_MEAN, ENV_MIN, ENV_MAX, ENV_SPREAD = 0, 1, 2, 3
VIEW_SPEED, VIEW_VORTICITY, VIEW_PRESSURE, VIEW_DIVERGENCE = 0, 1, 2, 3
VIEW_MAX_STOPS = 256
VIEW_MAX_COLOUR = 0xFC000000
MAX_BODIES = 16   # SFL_MAX_BODIES
OPEN_INFLOW, OPEN_OUTFLOW = 1, 2   # SFL_OPEN_*: the bytes of an openings map
MEAN_VELOCITY, MEAN_STRESS, MEAN_PRESSURE, MEAN_DYE, MEAN_ALL = 1, 2, 4, 8, 15   # SFL_MEAN_*: the groups of the averages
(MEAN_PLANE_U, MEAN_PLANE_V, MEAN_PLANE_UU, MEAN_PLANE_VV, MEAN_PLANE_UV, MEAN_PLANE_P, MEAN_PLANE_PP, MEAN_PLANE_R, MEAN_PLANE_G,
 MEAN_PLANE_B) = range(10)   # SFL_MEAN_PLANE_*
MEAN_PLANES = 10
UNIQUE_ID_BYTES = 128
TRACER_THREADS = 256   # kTracerThreads of csrc/tracer_kernels.h: tracers per workgroup (stated for the tests)
BATCH_LARGE_MAX_CELLS = 20224   # SFL_BATCH_LARGE_MAX_CELLS: cells of one member of sfl_batch_create_large


class PlanStep(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("kind", "field", "rows", "g_begin", "g_end", "nsweeps",
                                         "first_colour", "from_zero")]


class Drag(C.Structure):
    """struct drag of the sketch (ino:45-48): graphics coordinates."""
    _fields_ = [("coord_x", C.c_uint16), ("coord_y", C.c_uint16), ("vel_x", C.c_float), ("vel_y", C.c_float)]


class MemberParams(C.Structure):
    """sfl_member_params: the parameters of ONE batch member (sfl_batch_*_each), 16 bytes."""
    _fields_ = [("dt", C.c_float), ("dx", C.c_float), ("omega", C.c_float), ("iters", C.c_int32)]


class MemberStop(C.Structure):
    """sfl_member_stop: when ONE batch member's pressure solve stops (sfl_batch_*_until), 8 bytes."""
    _fields_ = [("tol", C.c_float), ("every", C.c_int32)]


class FlowStats(C.Structure):
    """struct sfl_flow_stats: what sfl_flow_stats and sfl_batch_flow_stats[_each] report, 40 bytes."""
    _fields_ = [("max_abs_vx", C.c_float), ("max_abs_vy", C.c_float), ("max_abs_div", C.c_float), ("what", C.c_uint32),
                ("dye_sum", C.c_uint64 * 3)]


class HistoryRecord(C.Structure):
    """struct sfl_history_record: one sample of a history, 64 bytes; the first 40 are a struct sfl_flow_stats."""
    _fields_ = [("max_abs_vx", C.c_float), ("max_abs_vy", C.c_float), ("max_abs_div", C.c_float), ("what", C.c_uint32),
                ("dye_sum", C.c_uint64 * 3), ("update_norm", C.c_float), ("iterations", C.c_int32), ("step", C.c_int64),
                ("dt", C.c_float), ("dx", C.c_float)]


class OpenFlux(C.Structure):
    """struct sfl_open_flux: the flux through the live open cells of one grid, 40 bytes."""
    _fields_ = [("inflow", C.c_int64), ("outflow", C.c_int64), ("exp2", C.c_int32), ("max_abs_n", C.c_float), ("inflow_cells", C.c_uint32),
                ("outflow_cells", C.c_uint32), ("nonfinite", C.c_uint32), ("reserved", C.c_uint32)]


class BodyLoad(C.Structure):
    """struct sfl_body_load: the pressure load on one solid body, 48 bytes."""
    _fields_ = [("fx", C.c_int64), ("fy", C.c_int64), ("exp2", C.c_int32), ("max_abs_p", C.c_float), ("faces", C.c_uint32 * 4),
                ("nonfinite", C.c_uint32), ("reserved", C.c_uint32)]


class BodyFriction(C.Structure):
    """struct sfl_body_friction: the skin friction on one solid body, 48 bytes with the offsets of BodyLoad."""
    _fields_ = [("fx", C.c_int64), ("fy", C.c_int64), ("exp2", C.c_int32), ("max_abs_t", C.c_float), ("faces", C.c_uint32 * 4),
                ("nonfinite", C.c_uint32), ("reserved", C.c_uint32)]


class BodyTorque(C.Structure):
    """struct sfl_body_torque: the moment of pressure and friction on one solid body about its pivot, 64 bytes."""
    _fields_ = [("mp", C.c_int64), ("mf", C.c_int64), ("exp2_p", C.c_int32), ("exp2_f", C.c_int32), ("max_abs_p", C.c_float),
                ("max_abs_t", C.c_float), ("faces", C.c_uint32), ("max_arm2", C.c_uint32), ("nonfinite_p", C.c_uint32),
                ("nonfinite_t", C.c_uint32), ("pivot2", C.c_int32 * 2), ("reserved", C.c_uint32 * 2)]


class FieldDistance(C.Structure):
    """struct sfl_field_distance: what sfl_distance and sfl_batch_distance report, 64 bytes."""
    _fields_ = [("max_abs_dvx", C.c_float), ("max_abs_dvy", C.c_float), ("max_abs_dp", C.c_float), ("what", C.c_uint32),
                ("velocity_cells_differ", C.c_uint32), ("dye_cells_differ", C.c_uint32), ("pressure_cells_differ", C.c_uint32),
                ("max_abs_ddye", C.c_uint32 * 3), ("sum_abs_ddye", C.c_uint64 * 3)]


class View(C.Structure):
    """struct sfl_view: a scalar of the flow and the palette it is drawn with, 40 bytes."""
    _fields_ = [("what", C.c_int32), ("dx", C.c_float), ("lo", C.c_float), ("hi", C.c_float), ("stops", C.c_int32),
                ("nan_colour", C.c_uint32 * 3), ("colours", C.POINTER(C.c_uint32))]


class SflError(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"sfl error {code}: {message}")
        self.code = code


def build_library(verbose: bool = False) -> str:
    """Compile the HIP extension for gfx950 in-tree (csrc/Makefile); returns the .so path."""
    subprocess.run(["make", "-C", os.path.join(_PKG, "csrc"), "-j4"], check=True,
                   stdout=None if verbose else subprocess.DEVNULL)
    return LIB_PATH


_lib = None


def lib() -> C.CDLL:
    """The loaded product library.  Fails loudly when it has not been built: there is no
    Python or CPU substitute for it."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build the HIP extension first "
                f"(python -c 'import __graft_entry__ as g; g.build()' or make -C "
                f"{os.path.join(_PKG, 'csrc')}).  There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def check(rc: int) -> None:
    if rc != OK:
        raise SflError(rc, lib().sfl_last_error().decode())


_ctx = C.c_void_p
_i, _f, _sz = C.c_int, C.c_float, C.c_size_t
_pi, _pf, _pu = C.POINTER(C.c_int), C.POINTER(C.c_float), C.POINTER(C.c_uint32)

# name -> (restype, argtypes); every symbol include/sfl.h declares is listed here and checked
# against the built library by tests/test_capi_symbols.py
SIGNATURES = {
    "sfl_abi_version": (_i, []),
    "sfl_last_error": (C.c_char_p, []),
    "sfl_device_count": (_i, [_pi]),
    "sfl_device_info": (_i, [_i, C.c_char_p, _sz, _pi, C.POINTER(_sz)]),
    "sfl_slab_rows": (_i, [_i, _i, _i, _pi, _pi]),
    "sfl_plan_poisson": (_i, [_i, _i, _i, _i, _i, _i, _i, C.POINTER(PlanStep), _i, _pi]),
    "sfl_plan_poisson_tail": (_i, [_i, _i, _i, _i, _i, _i, _i, _i, C.POINTER(PlanStep), _i, _pi]),
    "sfl_sor_pass_plan": (_i, [_i, _i, _pi, _pi, _i]),
    "sfl_host_advect_vec2f": (_i, [_pf, _pf, _pf, _i, _i, _f, _i]),
    "sfl_host_advect_vec3uq32": (_i, [_pu, _pu, _pf, _i, _i, _f, _i]),
    "sfl_host_advect_channels": (_i, [C.c_void_p, C.c_void_p, _pf, _i, _i, _f, _i, _i, _i]),
    "sfl_host_calculate_divergence": (_i, [_pf, _pf, _i, _i, _f]),
    "sfl_host_subtract_gradient": (_i, [_pf, _pf, _i, _i, _f]),
    "sfl_host_poisson_solve": (_i, [_pf, _pf, _i, _i, _f, _i, _f]),
    "sfl_host_release": (_i, []),
    "sfl_create": (_i, [C.POINTER(_ctx), _i, _i, _i]),
    "sfl_create_slab": (_i, [C.POINTER(_ctx), _i, _i, _i, _i, _i]),
    "sfl_destroy": (_i, [_ctx]),
    "sfl_set_option": (_i, [_ctx, _i, _i]),
    "sfl_get_option": (_i, [_ctx, _i, _pi]),
    "sfl_slab_of": (_i, [_ctx, _pi, _pi, _pi, _pi]),
    "sfl_comm_unique_id": (_i, [C.c_void_p, _sz]),
    "sfl_comm_attach": (_i, [_ctx, C.c_void_p, _sz]),
    "sfl_comm_check_options": (_i, [_ctx]),
    "sfl_comm_loopback": (_i, [_ctx, _i]),
    "sfl_comm_emulate": (_i, [_ctx]),
    "sfl_comm_emulate_rccl": (_i, [_ctx]),
    "sfl_group_link": (_i, [C.POINTER(_ctx), _i]),
    "sfl_upload": (_i, [_ctx, _i, C.c_void_p, _sz]),
    "sfl_download": (_i, [_ctx, _i, C.c_void_p, _sz]),
    "sfl_field_device_ptr": (_i, [_ctx, _i, C.POINTER(C.c_void_p)]),
    "sfl_advect_velocity": (_i, [_ctx, _f, _i]),
    "sfl_advect_color": (_i, [_ctx, _f, _i]),
    "sfl_advect_external": (_i, [_ctx, C.c_void_p, C.c_void_p, _i, _i, _f, _i]),
    "sfl_calculate_divergence": (_i, [_ctx, _f]),
    "sfl_poisson_solve": (_i, [_ctx, _f, _i, _f]),
    "sfl_subtract_gradient": (_i, [_ctx, _f]),
    "sfl_residual": (_i, [_ctx, _f, _pf]),
    "sfl_poisson_continue": (_i, [_ctx, _f, _i, _f]),
    "sfl_poisson_solve_until": (_i, [_ctx, _f, _i, _f, _f, _i, C.POINTER(C.c_int32), _pf]),
    "sfl_flow_stats": (_i, [_ctx, _i, _f, C.POINTER(FlowStats)]),
    "sfl_distance": (_i, [_ctx, _ctx, _i, C.POINTER(FieldDistance)]),
    "sfl_step": (_i, [_ctx, _f, _f, _i, _f]),
    "sfl_step_n": (_i, [_ctx, _i, _f, _f, _i, _f]),
    "sfl_queue_forces": (_i, [_ctx, _pi, _pf, _i]),
    "sfl_queue_drags": (_i, [_ctx, C.c_void_p, _i]),
    "sfl_queue_forces_at": (_i, [_ctx, _i, _pi, _pf, _i]),
    "sfl_queue_drags_at": (_i, [_ctx, _i, C.c_void_p, _i]),
    "sfl_forces_pending": (_i, [_ctx, _pi, _pi]),
    "sfl_forget_forces": (_i, [_ctx]),
    "sfl_setup_sketch_fields": (_i, [_ctx]),
    "sfl_render_rgb565": (_i, [_ctx, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_synchronize": (_i, [_ctx]),
    "sfl_timer_start": (_i, [_ctx]),
    "sfl_timer_stop": (_i, [_ctx, _pf]),
    "sfl_last_solve_info": (_i, [_ctx, _pi, _pi, _pi]),
    "sfl_batch_create": (_i, [C.POINTER(_ctx), _i, _i, _i, _i]),
    "sfl_batch_create_large": (_i, [C.POINTER(_ctx), _i, _i, _i, _i]),
    "sfl_batch_is_large": (_i, [_ctx, _pi]),
    "sfl_batch_destroy": (_i, [_ctx]),
    "sfl_batch_shape": (_i, [_ctx, _pi, _pi, _pi]),
    "sfl_batch_upload": (_i, [_ctx, _i, _i, _i, C.c_void_p, _sz]),
    "sfl_batch_download": (_i, [_ctx, _i, _i, _i, C.c_void_p, _sz]),
    "sfl_batch_field_device_ptr": (_i, [_ctx, _i, C.POINTER(C.c_void_p)]),
    "sfl_batch_queue_forces": (_i, [_ctx, _pi, _pi, _pf, _i]),
    "sfl_batch_queue_forces_at": (_i, [_ctx, _i, _pi, _pi, _pf, _i]),
    "sfl_batch_forces_pending": (_i, [_ctx, _pi, _pi]),
    "sfl_batch_forget_forces": (_i, [_ctx]),
    "sfl_batch_step_n": (_i, [_ctx, _i, _f, _f, _i, _f]),
    "sfl_batch_poisson_solve": (_i, [_ctx, _f, _i, _f]),
    "sfl_batch_step_n_each": (_i, [_ctx, _i, C.POINTER(MemberParams)]),
    "sfl_batch_poisson_solve_each": (_i, [_ctx, C.POINTER(MemberParams)]),
    "sfl_batch_residual": (_i, [_ctx, _i, _i, _pf, _sz]),
    "sfl_batch_step_n_until": (_i, [_ctx, _i, C.POINTER(MemberParams), C.POINTER(MemberStop)]),
    "sfl_batch_poisson_solve_until": (_i, [_ctx, C.POINTER(MemberParams), C.POINTER(MemberStop)]),
    "sfl_batch_iterations": (_i, [_ctx, _i, _i, C.POINTER(C.c_int32), _sz]),
    "sfl_batch_flow_stats": (_i, [_ctx, _i, _f, _i, _i, C.POINTER(FlowStats), _sz]),
    "sfl_batch_flow_stats_each": (_i, [_ctx, _i, C.POINTER(MemberParams), _i, _i, C.POINTER(FlowStats), _sz]),
    "sfl_batch_distance": (_i, [_ctx, _i, _ctx, _i, _i, _i, C.POINTER(FieldDistance), _sz]),
    "sfl_batch_envelope": (_i, [_ctx, _i, _i]),
    "sfl_batch_envelope_info": (_i, [_ctx, _pi, _pi]),
    "sfl_batch_envelope_download": (_i, [_ctx, _i, _pu, _sz]),
    "sfl_batch_envelope_render": (_i, [_ctx, _i, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_batch_setup_sketch_fields": (_i, [_ctx]),
    "sfl_batch_render_rgb565": (_i, [_ctx, _i, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_batch_render_members": (_i, [_ctx, _i, _i, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_batch_record_start": (_i, [_ctx, _i, _i, _i, _i, _i, _i]),
    "sfl_batch_record_stop": (_i, [_ctx]),
    "sfl_batch_record_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64)]),
    "sfl_batch_record_read": (_i, [_ctx, _i, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_tracers_set": (_i, [_ctx, _pf, _sz, _i]),
    "sfl_tracers_count": (_i, [_ctx, C.POINTER(_sz)]),
    "sfl_tracers_download": (_i, [_ctx, _pf, _sz]),
    "sfl_tracers_advance": (_i, [_ctx, _f]),
    "sfl_tracers_sample": (_i, [_ctx, _i, _i, C.c_void_p, _sz]),
    "sfl_tracers_trail_start": (_i, [_ctx, _i, _i]),
    "sfl_tracers_trail_stop": (_i, [_ctx]),
    "sfl_tracers_trail_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64)]),
    "sfl_tracers_trail_read": (_i, [_ctx, _i, _i, _pf, _sz]),
    "sfl_batch_tracers_set": (_i, [_ctx, _pf, _sz, _i]),
    "sfl_batch_tracers_count": (_i, [_ctx, C.POINTER(_sz)]),
    "sfl_batch_tracers_download": (_i, [_ctx, _pf, _sz]),
    "sfl_batch_tracers_advance": (_i, [_ctx, _f]),
    "sfl_batch_tracers_sample": (_i, [_ctx, _i, _i, C.c_void_p, _sz]),
    "sfl_batch_tracers_trail_start": (_i, [_ctx, _i, _i]),
    "sfl_batch_tracers_trail_stop": (_i, [_ctx]),
    "sfl_batch_tracers_trail_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64)]),
    "sfl_batch_tracers_trail_read": (_i, [_ctx, _i, _i, _pf, _sz]),
    "sfl_view_scalar": (_i, [_ctx, _i, _f, _pf, _sz]),
    "sfl_batch_view_scalar": (_i, [_ctx, _i, _f, _i, _i, _pf, _sz]),
    "sfl_view_texels": (_i, [_ctx, C.POINTER(View), _pu, _sz]),
    "sfl_batch_view_texels": (_i, [_ctx, C.POINTER(View), _i, _i, _pu, _sz]),
    "sfl_view_render": (_i, [_ctx, C.POINTER(View), _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_batch_view_render_members": (_i, [_ctx, C.POINTER(View), _i, _i, _i, _i, C.POINTER(C.c_uint16), _sz]),
    "sfl_batch_record_view": (_i, [_ctx, C.POINTER(View)]),
    "sfl_batch_history_start": (_i, [_ctx, _i, _i, _i, _i]),
    "sfl_batch_history_stop": (_i, [_ctx]),
    "sfl_batch_history_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64)]),
    "sfl_batch_history_read": (_i, [_ctx, _i, _i, _i, _i, C.POINTER(HistoryRecord), _sz]),
    "sfl_history_start": (_i, [_ctx, _i, _i]),
    "sfl_history_stop": (_i, [_ctx]),
    "sfl_history_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64)]),
    "sfl_history_read": (_i, [_ctx, _i, _i, C.POINTER(HistoryRecord), _sz]),
    "sfl_batch_set_solids": (_i, [_ctx, C.POINTER(C.c_uint8), _i]),
    "sfl_batch_solids_info": (_i, [_ctx, _pi, _pi]),
    "sfl_batch_solids_download": (_i, [_ctx, _i, _i, C.POINTER(C.c_uint8), _sz]),
    "sfl_set_solids": (_i, [_ctx, C.POINTER(C.c_uint8)]),
    "sfl_solids_info": (_i, [_ctx, _pi, C.POINTER(C.c_int64)]),
    "sfl_solids_download": (_i, [_ctx, C.POINTER(C.c_uint8), _sz]),
    "sfl_batch_set_bodies": (_i, [_ctx, C.POINTER(C.c_uint8), _i, _i]),
    "sfl_batch_bodies_info": (_i, [_ctx, _pi, _pi, _pi]),
    "sfl_batch_bodies_download": (_i, [_ctx, _i, _i, C.POINTER(C.c_uint8), _sz]),
    "sfl_batch_loads": (_i, [_ctx, _i, _i, C.POINTER(BodyLoad), _sz]),
    "sfl_batch_loads_start": (_i, [_ctx, _i, _i, _i, _i]),
    "sfl_batch_loads_stop": (_i, [_ctx]),
    "sfl_batch_loads_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_batch_loads_read": (_i, [_ctx, _i, _i, C.POINTER(BodyLoad), _sz]),
    "sfl_set_bodies": (_i, [_ctx, C.POINTER(C.c_uint8), _i]),
    "sfl_bodies_info": (_i, [_ctx, _pi, _pi]),
    "sfl_bodies_download": (_i, [_ctx, C.POINTER(C.c_uint8), _sz]),
    "sfl_loads": (_i, [_ctx, C.POINTER(BodyLoad), _sz]),
    "sfl_loads_start": (_i, [_ctx, _i, _i]),
    "sfl_loads_stop": (_i, [_ctx]),
    "sfl_loads_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_loads_read": (_i, [_ctx, _i, _i, C.POINTER(BodyLoad), _sz]),
    "sfl_set_viscosity": (_i, [_ctx, _f, _i]),
    "sfl_viscosity_info": (_i, [_ctx, _pf, _pi]),
    "sfl_diffuse_velocity": (_i, [_ctx, _f, _f, _f, _i]),
    "sfl_batch_set_viscosity": (_i, [_ctx, _pf, _i, _i]),
    "sfl_batch_viscosity_info": (_i, [_ctx, _pi, _pi, _pi]),
    "sfl_batch_viscosity_download": (_i, [_ctx, _i, _i, _pf, _sz]),
    "sfl_batch_set_openings": (_i, [_ctx, C.POINTER(C.c_uint8), _i, _pf, _i]),
    "sfl_batch_set_inflow": (_i, [_ctx, _pf, _i]),
    "sfl_batch_openings_info": (_i, [_ctx, _pi, _pi, _pi, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sfl_batch_openings_download": (_i, [_ctx, _i, _i, C.POINTER(C.c_uint8), _sz]),
    "sfl_batch_inflow_download": (_i, [_ctx, _i, _i, _pf, _sz]),
    "sfl_set_openings": (_i, [_ctx, C.POINTER(C.c_uint8), _f, _f]),
    "sfl_set_inflow": (_i, [_ctx, _f, _f]),
    "sfl_openings_info": (_i, [_ctx, _pi, _pf, _pf, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sfl_openings_download": (_i, [_ctx, C.POINTER(C.c_uint8), _sz]),
    "sfl_set_inflow_profile": (_i, [_ctx, _pi, _pf, _i]),
    "sfl_inflow_profile_info": (_i, [_ctx, _pi]),
    "sfl_inflow_profile_download": (_i, [_ctx, _pi, _pf, _i]),
    "sfl_openings_flux": (_i, [_ctx, C.POINTER(OpenFlux)]),
    "sfl_batch_set_inflow_profile": (_i, [_ctx, _pi, _pi, _pf, _i]),
    "sfl_batch_inflow_profile_info": (_i, [_ctx, _pi, C.POINTER(C.c_int64)]),
    "sfl_batch_inflow_profile_download": (_i, [_ctx, _i, _pi, _pf, _i, _pi]),
    "sfl_batch_openings_flux": (_i, [_ctx, _i, _i, C.POINTER(OpenFlux), _sz]),
    "sfl_batch_friction": (_i, [_ctx, _i, _i, C.POINTER(BodyFriction), _sz]),
    "sfl_batch_friction_start": (_i, [_ctx, _i, _i, _i, _i]),
    "sfl_batch_friction_stop": (_i, [_ctx]),
    "sfl_batch_friction_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_batch_friction_read": (_i, [_ctx, _i, _i, C.POINTER(BodyFriction), _sz]),
    "sfl_friction": (_i, [_ctx, C.POINTER(BodyFriction), _sz]),
    "sfl_friction_start": (_i, [_ctx, _i, _i]),
    "sfl_friction_stop": (_i, [_ctx]),
    "sfl_friction_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_friction_read": (_i, [_ctx, _i, _i, C.POINTER(BodyFriction), _sz]),
    "sfl_batch_set_body_pivots": (_i, [_ctx, C.POINTER(C.c_int32), _i, _i]),
    "sfl_batch_body_pivots_download": (_i, [_ctx, _i, _i, C.POINTER(C.c_int32), _sz]),
    "sfl_batch_torque": (_i, [_ctx, _i, _i, C.POINTER(BodyTorque), _sz]),
    "sfl_batch_torque_start": (_i, [_ctx, _i, _i, _i, _i]),
    "sfl_batch_torque_stop": (_i, [_ctx]),
    "sfl_batch_torque_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_batch_torque_read": (_i, [_ctx, _i, _i, C.POINTER(BodyTorque), _sz]),
    "sfl_set_body_pivots": (_i, [_ctx, C.POINTER(C.c_int32), _i]),
    "sfl_body_pivots_download": (_i, [_ctx, C.POINTER(C.c_int32), _sz]),
    "sfl_torque": (_i, [_ctx, C.POINTER(BodyTorque), _sz]),
    "sfl_torque_start": (_i, [_ctx, _i, _i]),
    "sfl_torque_stop": (_i, [_ctx]),
    "sfl_torque_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), _pi]),
    "sfl_torque_read": (_i, [_ctx, _i, _i, C.POINTER(BodyTorque), _sz]),
    "sfl_mean_start": (_i, [_ctx, _i, _i]),
    "sfl_mean_stop": (_i, [_ctx]),
    "sfl_mean_sample": (_i, [_ctx]),
    "sfl_mean_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sfl_mean_download": (_i, [_ctx, _i, C.c_void_p, _sz]),
    "sfl_batch_mean_start": (_i, [_ctx, _i, _i, _i, _i]),
    "sfl_batch_mean_stop": (_i, [_ctx]),
    "sfl_batch_mean_sample": (_i, [_ctx]),
    "sfl_batch_mean_info": (_i, [_ctx, _pi, _pi, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "sfl_batch_mean_download": (_i, [_ctx, _i, _i, _i, C.c_void_p, _sz]),
    "sfl_set_wall_velocity": (_i, [_ctx, _pi, _pf, _i]),
    "sfl_wall_velocity_info": (_i, [_ctx, _pi]),
    "sfl_wall_velocity_download": (_i, [_ctx, _pi, _pf, _i]),
    "sfl_batch_set_wall_velocity": (_i, [_ctx, _pi, _pi, _pf, _i]),
    "sfl_batch_wall_velocity_info": (_i, [_ctx, _pi, C.POINTER(C.c_int64)]),
    "sfl_batch_wall_velocity_download": (_i, [_ctx, _i, _pi, _pf, _i, _pi]),
    "sfl_batch_synchronize": (_i, [_ctx]),
}


def _declare(l: C.CDLL) -> None:
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args
