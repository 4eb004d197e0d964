// context_walls.hip -- a whole-domain context whose solid cells hold a prescribed velocity (gfx950 / MI355X; include/sfl.h
// "WALL VELOCITIES"): the two launches that extend the solids' step, on a grid of ANY size.  Kernels of their own: a context
// without a wall table launches exactly what it launched before, and the tile of diffuse_tile.h reads what they leave as
// it reads any solid neighbour -- as it is.
//
//   * wall_scatter_kernel (item 8, behind the dye advection): one thread per record of the compact list, one 8-byte vector
//     store each; the list is unique, so no two threads store to one cell.
//   * wall_impose_kernel (the extended item 3, in front of item 3a): one thread per FOUR code bytes, read as one word; only
//     a solid cell -- a byte whose bit 4 is clear -- is stored to: (0, 0), or its record's velocity where the ascending list
//     names it (a binary search of the few solid cells among the records: both reads of a step stay in L2).  One store per
//     solid cell, so the zeroes and the records need no order between them.
//
// Bounds: a thread's word lies wholly below `cells` or its bytes are read one by one; the list's indices were checked
// against the grid by the host (wall_table.h).
#include "advect_math.h"
#include "wall_kernels.h"

namespace sfl {
namespace {

using namespace advect_math;

constexpr int kThreads = 256;

__global__ void __launch_bounds__(kThreads)
wall_scatter_kernel(float2 *__restrict__ v, const uint32_t *__restrict__ cells, const float2 *__restrict__ vel, int n)
{
    const int k = blockIdx.x * kThreads + threadIdx.x;
    if (k < n) v[cells[k]] = vel[k];
}

// the record of cell c in the ascending list, or (0, 0)
__device__ __forceinline__ float2 wall_of(uint32_t c, const uint32_t *__restrict__ cells, const float2 *__restrict__ vel, int n)
{
    int lo = 0, hi = n;   // the first k with cells[k] >= c
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cells[mid] < c) lo = mid + 1;
        else hi = mid;
    }
    if (lo < n && cells[lo] == c) return vel[lo];
    return make_float2(0.0f, 0.0f);
}

__global__ void __launch_bounds__(kThreads)
wall_impose_kernel(float2 *__restrict__ v, const uint8_t *__restrict__ codes, size_t total, const uint32_t *__restrict__ cells,
                   const float2 *__restrict__ vel, int n)
{
    const size_t c0 = 4 * ((size_t)blockIdx.x * kThreads + threadIdx.x);
    if (c0 >= total) return;
    uint32_t word = 0xffffffffu;   // (a byte past the end counts as fluid: never stored to)
    if (c0 + 4 <= total) {
        word = *reinterpret_cast<const uint32_t *>(codes + c0);   // (hipMalloc's alignment, c0 a multiple of 4)
    } else {
        for (size_t k = 0; c0 + k < total; ++k) word = (word & ~(0xffu << (8 * k))) | ((uint32_t)codes[c0 + k] << (8 * k));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (!((word >> (8 * k)) & kSolidFluid)) v[c0 + k] = wall_of((uint32_t)(c0 + k), cells, vel, n);
}

}  // namespace

hipError_t launch_wall_scatter(hipStream_t s, float *v, const uint32_t *cells, const float *vel, int n)
{
    if (n < 1) return hipErrorInvalidValue;
    wall_scatter_kernel<<<(n + kThreads - 1) / kThreads, kThreads, 0, s>>>(reinterpret_cast<float2 *>(v), cells, reinterpret_cast<const float2 *>(vel), n);
    return hipGetLastError();
}

hipError_t launch_wall_impose(hipStream_t s, float *v, const uint8_t *codes, size_t total_cells, const uint32_t *cells, const float *vel, int n)
{
    if (n < 1 || total_cells < 1) return hipErrorInvalidValue;
    const size_t words = (total_cells + 3) / 4;
    wall_impose_kernel<<<(unsigned)((words + kThreads - 1) / kThreads), kThreads, 0, s>>>(reinterpret_cast<float2 *>(v), codes, total_cells, cells,
                                                                                         reinterpret_cast<const float2 *>(vel), n);
    return hipGetLastError();
}

}  // namespace sfl
