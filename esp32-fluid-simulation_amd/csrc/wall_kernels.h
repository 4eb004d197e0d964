// wall_kernels.h -- launch interface of the kernels behind the wall velocities of a whole-domain context (internal, as
// kernels.h, whose types it uses; include/sfl.h "WALL VELOCITIES"): context_walls.hip.  Called from context_walls.cpp
// alone.  WHOLE-DOMAIN arrays of any size; the wall table is a compact list of `n` records, n >= 1: cells[k] the index of
// a SOLID cell, unique and ascending, vel the (u, v) of record k at 2 * k.  Every launcher is asynchronous on the given
// stream and returns the hipError_t of its launch.
#pragma once
#include "kernels.h"

namespace sfl {

// Item 8: v[cells[k]] = record k's velocity, bits as given.  One thread per record, one 8-byte store each.
hipError_t launch_wall_scatter(hipStream_t s, float *v, const uint32_t *cells, const float *vel, int n);

// The extended item 3, in front of item 3a: every solid cell of v (codes: one byte per cell, solids.cpp solid_codes; bit 4
// clear) holds (0, 0), except one the list names, which holds its record's velocity.  Streams over the code bytes and
// stores only at solid cells; a solid cell looks itself up in the ascending list, so no cell is stored to twice.
hipError_t launch_wall_impose(hipStream_t s, float *v, const uint8_t *codes, size_t total_cells, const uint32_t *cells, const float *vel, int n);

}  // namespace sfl
