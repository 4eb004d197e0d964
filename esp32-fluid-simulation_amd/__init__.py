"""MI355X-native stable-fluids hot path (the sim task of colonelwatch/ESP32-fluid-simulation).

The product is ``lib/libsfl_hip.so`` -- hand-written HIP kernels for gfx950 behind the C ABI of
``include/sfl.h`` -- plus the C++ drop-in headers in ``include/sfl/``.  This Python package is
only the binding used by the tests and by ``bench.py``:

* :mod:`._capi`   ctypes declarations, 1:1 with include/sfl.h
* :mod:`.solver`  ``Solver`` (a context), ``BatchSolver`` (many small grids stepped by one launch) and ``HostPath`` (reference-style operators on host
  arrays, executed on the GPU)

Import it with ``importlib.import_module("esp32-fluid-simulation_amd")`` (the directory name is
not a Python identifier).  Importing never touches the GPU and never builds anything; the first
call that needs the library fails loudly if it is missing -- there is no CPU fallback.
"""
from . import _capi as capi
from ._capi import (LIB_PATH, OPEN_INFLOW, OPEN_OUTFLOW, MEAN_VELOCITY, MEAN_STRESS, MEAN_PRESSURE, MEAN_DYE, MEAN_ALL, SflError,
                    build_library)
from .solver import (BatchSolver, HostPath, Solver, comm_unique_id, device_count, device_info, plan_poisson,
                     member_params, member_stops, slab_rows, sor_pass_plan, stdout_to_stderr, FLOW_STATS_DTYPE,
                     FLOW_STATS_STRIP_COLS, FLOW_STATS_CHUNK_ROWS, FIELD_DISTANCE_DTYPE, HISTORY_DTYPE, HISTORY_THREADS, BODY_LOAD_DTYPE, BODY_FRICTION_DTYPE, BODY_TORQUE_DTYPE, OPEN_FLUX_DTYPE, openings_flux_xy, rigid_wall_velocity, wall_shares, MEAN_PLANE_NAMES, DIST_THREADS, DIST_ITEM_LOADS,
                     DIST_VELOCITY_LANE_CELLS, DIST_PRESSURE_LANE_CELLS, DIST_DYE_LANE_CELLS, ENV_BLOCK_WORDS,
                     ENV_GROUP_MEMBERS, View, PALETTE_GREY, PALETTE_HEAT, PALETTE_BLUE_WHITE_RED)

__all__ = ["capi", "LIB_PATH", "SflError", "build_library", "BatchSolver", "HostPath", "Solver",
           "comm_unique_id", "device_count", "device_info", "member_params", "member_stops", "plan_poisson", "slab_rows",
           "sor_pass_plan", "stdout_to_stderr", "FLOW_STATS_DTYPE", "FLOW_STATS_STRIP_COLS", "FLOW_STATS_CHUNK_ROWS",
           "FIELD_DISTANCE_DTYPE", "HISTORY_DTYPE", "HISTORY_THREADS", "BODY_LOAD_DTYPE", "BODY_FRICTION_DTYPE", "BODY_TORQUE_DTYPE", "OPEN_FLUX_DTYPE", "openings_flux_xy", "rigid_wall_velocity", "wall_shares", "DIST_THREADS", "DIST_ITEM_LOADS", "DIST_VELOCITY_LANE_CELLS", "DIST_PRESSURE_LANE_CELLS",
           "DIST_DYE_LANE_CELLS", "ENV_BLOCK_WORDS", "ENV_GROUP_MEMBERS", "View", "PALETTE_GREY", "PALETTE_HEAT",
           "PALETTE_BLUE_WHITE_RED", "OPEN_INFLOW", "OPEN_OUTFLOW", "MEAN_VELOCITY", "MEAN_STRESS", "MEAN_PRESSURE", "MEAN_DYE",
           "MEAN_ALL", "MEAN_PLANE_NAMES"]
