// update_norm.hip -- the update norm of a pressure field of ANY size in one streaming pass (gfx950 / MI355X):
// max over the cells of rows [g_begin, g_end) of |p_gs(c) - p(c)|, where p_gs is the value a plain Gauss-Seidel update
// would put into the cell.  What sfl_residual reports and what sfl_poisson_solve_until decides on (include/sfl.h).
//
// The arithmetic is batch_grid.hip's update_norm_in_lds, term for term: (((z + W) + E) + S) + N with -0.0f for an absent
// neighbour, z = -0.0f inside and +0.0f on the perimeter, k = -1/2, -1/3, -1/4 narrowed from double (poisson.cpp:67-89,
// :107-109), both colours read from the same p, the maximum taken over the bit patterns of |p_gs - p| as unsigned
// integers -- which orders finite values and +inf as floats do and lets any NaN win.  A maximum does not depend on the
// order of reduction: the result is bit-reproducible whatever the tiling.
//
// The pass is bound by memory: 8 B per cell (p and d once each), a few operations per cell.  So it is laid out as the
// fused SOR kernel streams (sor_lane.h), not as one thread per cell with five loads:
//   * a wave owns a TILE: a strip of 256 columns (64 lanes x one 16-byte load) and a chunk of rows it walks down with
//     the rows above and below in registers -- every row of p is loaded once per tile (plus the two rows around the
//     chunk), every row of d once;
//   * W and E come from the lane's own four cells and from the neighbour lanes by DPP wave shifts; only lane 0 and
//     lane 63 load one more cell each per row, the strip's outer neighbours;
//   * the loads of row r + 1 are issued in front of the arithmetic of row r;
//   * tiles are dealt to the waves of at most kMaxBlocks workgroups, which stride over the rest;
//   * the wave's maximum by __shfl_xor, the workgroup's through LDS, then ONE atomicMax per workgroup on a device word
//     that the launcher zeroes on the stream in front of the kernel.
// VEC = rows of 16-byte aligned float4s (dim_x a multiple of 4, aligned arrays): one global_load_dwordx4 per lane and
// row.  Everything else takes four clamped 4-byte loads per lane: correct at any width and alignment, not as fast.
// Loads are unconditional and clamped into the row: what a clamped load returns never reaches the maximum.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#include <algorithm>

#include "until_kernels.h"

namespace sfl {
namespace {

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kStripCols = 256;    // 64 lanes x 4 cells
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: every wave slot of the chip once

// DPP full-wave shifts (wave_shr:1 / wave_shl:1, as sor_lane.h): lane 0 / lane 63 receive 0 and take the strip's
// outer neighbour instead
__device__ __forceinline__ float lane_below(float x)  // value of lane - 1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x138, 0xf, 0xf, false));
}
__device__ __forceinline__ float lane_above(float x)  // value of lane + 1
{
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x130, 0xf, 0xf, false));
}

__device__ __forceinline__ v4f splat(float x) { return v4f{x, x, x, x}; }

// the lane's four cells x .. x + 3 of the row at `row`, columns clamped into the row
template <bool VEC>
__device__ __forceinline__ v4f load_cells(const float *row, int x, int dim_x)
{
    if (VEC) return *reinterpret_cast<const v4f *>(row + min(x, dim_x - 4));   // (dim_x is a multiple of 4: all in or all out)
    v4f r;
    r.x = row[min(x, dim_x - 1)];
    r.y = row[min(x + 1, dim_x - 1)];
    r.z = row[min(x + 2, dim_x - 1)];
    r.w = row[min(x + 3, dim_x - 1)];
    return r;
}

// the strip's outer neighbours of one row: lane 0 gets cell x0 - 1, lane 63 cell x0 + 256 (where the domain has them)
__device__ __forceinline__ float load_edge(const float *row, int lane, int x0, int dim_x)
{
    const int ex = lane == 0 ? x0 - 1 : x0 + kStripCols;
    const bool has = (lane == 0 && x0 > 0) || (lane == 63 && ex < dim_x);
    return has ? row[ex] : -0.0f;
}

// max |p_gs - p| over the lane's four cells of row r, as bits.  s / n: the rows below / above (-0.0f where the domain
// has none), nv = vertical neighbours present (row-uniform), edge = load_edge of this row.
__device__ __forceinline__ unsigned row_norm(unsigned m, v4f s, v4f c, v4f n, v4f dd, float edge, int lane, int x,
                                             int dim_x, int nv, float dx)
{
    const int i_max = dim_x - 1;
    float below = lane_below(c.w), above = lane_above(c.x);
    below = lane == 0 ? edge : below;
    above = lane == 63 ? edge : above;
    const float w[4] = {below, c.x, c.y, c.z}, e[4] = {c.y, c.z, c.w, above};
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int i = x + q;
        const int present = (i > 0) + (i < i_max) + nv;
        const float ww = (i > 0) ? w[q] : -0.0f;
        const float ee = (i < i_max) ? e[q] : -0.0f;
        const float z = (present == 4) ? -0.0f : 0.0f;
        const float kf = (present == 2) ? (float)(-1.0 / 2.0) : (present == 3) ? (float)(-1.0 / 3.0) : -0.25f;
        const float sum = (((z + ww) + ee) + s[q]) + n[q];
        const float p_gs = kf * (dx * dd[q] - sum);
        const unsigned bits = __float_as_uint(p_gs - c[q]) & 0x7fffffffu;   // |p_gs - p|
        if (i < dim_x) m = bits > m ? bits : m;   // (a clamped column has no say)
    }
    return m;
}

template <bool VEC>
__global__ void __launch_bounds__(kThreads)
update_norm_kernel(const float *__restrict__ p, const float *__restrict__ d, Slab g, int g_begin, int g_end,
                   int rows_per_tile, int strips, int tiles, float dx, unsigned *__restrict__ worst)
{
    __shared__ unsigned wave_worst[kWaves];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int dim_x = g.dim_x, j_max = g.gdim_y - 1;
    const size_t pitch = (size_t)dim_x;
    unsigned m = 0u;
    for (int tile = blockIdx.x * kWaves + wave; tile < tiles; tile += gridDim.x * kWaves) {   // wave-uniform
        const int chunk = tile / strips, strip = tile - chunk * strips;   // strips run fastest: neighbours in time share rows
        const int x0 = strip * kStripCols, x = x0 + 4 * lane;
        const int r0 = g_begin + chunk * rows_per_tile, r1 = min(r0 + rows_per_tile, g_end);
        const float *prow = p + (size_t)(r0 - g.grow0) * pitch, *drow = d + (size_t)(r0 - g.grow0) * pitch;
        // (loads are unconditional: a row the domain does not have is loaded from the row beside it and replaced)
        v4f below = load_cells<VEC>(r0 > 0 ? prow - pitch : prow, x, dim_x);
        if (r0 <= 0) below = splat(-0.0f);
        v4f cur = load_cells<VEC>(prow, x, dim_x), dd = load_cells<VEC>(drow, x, dim_x);
        float edge = load_edge(prow, lane, x0, dim_x);
        for (int r = r0; r < r1; ++r) {
            // row r + 1 first: its loads are in flight while row r is evaluated (the chunk's last row loads itself again)
            v4f above = load_cells<VEC>(r < j_max ? prow + pitch : prow, x, dim_x);
            if (r >= j_max) above = splat(-0.0f);
            const size_t step = r + 1 < r1 ? pitch : 0;
            const v4f dd_next = load_cells<VEC>(drow + step, x, dim_x);
            const float edge_next = load_edge(prow + step, lane, x0, dim_x);
            m = row_norm(m, below, cur, above, dd, edge, lane, x, dim_x, (r > 0) + (r < j_max), dx);
            below = cur;
            cur = above;
            dd = dd_next;
            edge = edge_next;
            prow += pitch;
            drow += pitch;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    if (lane == 0) wave_worst[wave] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kWaves; ++k) m = wave_worst[k] > m ? wave_worst[k] : m;
        atomicMax(worst, m);
    }
}

}  // namespace

hipError_t launch_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, Slab g, int g_begin,
                              int g_end, float dx)
{
    hipError_t e = hipMemsetAsync(worst, 0, sizeof(unsigned), s);
    if (e != hipSuccess || g_end <= g_begin) return e;
    const int rows = g_end - g_begin, strips = (g.dim_x + kStripCols - 1) / kStripCols;
    // the tallest tile that still leaves every wave of the capped grid one: a taller tile re-reads fewer rows (the two
    // around its chunk), but tiles that do not fill the chip leave bandwidth idle
    int rows_per_tile = 8;
    for (int r : {32, 16})
        if ((int64_t)strips * ((rows + r - 1) / r) >= (int64_t)kMaxBlocks * kWaves) {
            rows_per_tile = r;
            break;
        }
    const int tiles = strips * ((rows + rows_per_tile - 1) / rows_per_tile);
    const int blocks = std::min((tiles + kWaves - 1) / kWaves, kMaxBlocks);
    const bool vec = g.dim_x % 4 == 0 && (reinterpret_cast<uintptr_t>(p) | reinterpret_cast<uintptr_t>(d)) % 16 == 0;
    if (vec)
        update_norm_kernel<true><<<blocks, kThreads, 0, s>>>(p, d, g, g_begin, g_end, rows_per_tile, strips, tiles, dx, worst);
    else
        update_norm_kernel<false><<<blocks, kThreads, 0, s>>>(p, d, g, g_begin, g_end, rows_per_tile, strips, tiles, dx, worst);
    return hipGetLastError();
}

}  // namespace sfl
