// context_openings.hip -- a whole-domain context with openings on the rim of its grid (gfx950 / MI355X; include/sfl.h "OPENINGS
// OF A CONTEXT"): the divergence, the pressure solve, the gradient and the two maxima of context_solids.hip by the openings'
// rule, and the imposition of the inflow (item 2a) over the compact list of inflow cells that the host builds.  Kernels of
// their own: those of context_solids.hip keep their text and their instructions.
//
// Two bytes per cell, formed on the host (context_openings.cpp) and read from memory: the CODE BYTE of the solids (all fluid
// where no mask is set; a copy -- the solids' own bytes are not touched) and the OPEN BYTE (sor_open_tile.h: which neighbour is
// open, bit 4 = outflow).  Together they are the open code of advect_math.h, whose stencils the streaming kernels call
// (divergence_sum_open, project_cell_open).
//
// THE SOLVE is the tile of sor_solid_tile.h: its load, its half-sweeps and its store as they stand; behind the load
// open_tile::set_up_k sets the k of the outflow cells from n = present + 1.  The loop is the same loop.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the rule's order.
#include <algorithm>

#include "advect_math.h"
#include "open_kernels.h"
#include "sor_open_tile.h"

namespace sfl {
namespace {

using namespace advect_math;

constexpr int kStreamThreads = 256, kStreamWaves = kStreamThreads / 64;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 workgroups: what a reduction's grid is capped at (update_norm.hip)

// the open code of advect_math.h from the two bytes of a cell
__device__ __forceinline__ int open_code(const uint8_t *codes, const uint8_t *open, size_t c)
{
    return (int)codes[c] | ((int)open[c] << kOpenShift);
}

// item 2a: every fluid inflow cell holds the inflow velocity; the host's compact list names them
__global__ void __launch_bounds__(kStreamThreads)
open_inflow_kernel(float *__restrict__ v, const uint32_t *__restrict__ cells, int n, float2 inflow)
{
    const int k = blockIdx.x * kStreamThreads + threadIdx.x;
    if (k < n) reinterpret_cast<float2 *>(v)[cells[k]] = inflow;
}

// ---- the solve ---------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(solid_tile::kThreads)
open_sor_kernel(float *__restrict__ p_out, const float *__restrict__ p_in, const float *__restrict__ d,
                 const uint8_t *__restrict__ codes, const uint8_t *__restrict__ open, int dim_x, int dim_y, int k, SorParams prm)
{
    __shared__ float lds[solid_tile::kLdsFloats];
    solid_tile::Tile t;
    t.p_in = p_in;
    t.p_out = p_out;
    t.d = d;
    t.codes = codes;
    t.dim_x = dim_x;
    t.dim_y = dim_y;
    const int tiles_x = (dim_x + solid_tile::kTX - 1) / solid_tile::kTX, tile_y = blockIdx.x / tiles_x;   // (tiles of a row run fastest)
    t.x0 = (blockIdx.x - tile_y * tiles_x) * solid_tile::kTX;
    t.y0 = tile_y * solid_tile::kTY;
    t.k = k;
    t.dx = prm.dx;
    t.omega = prm.omega;
    t.one_minus_omega = prm.one_minus_omega;
    solid_tile::Cells c;
    solid_tile::load(c, lds, t, threadIdx.x);
    open_tile::set_up_k(c, t, open, threadIdx.x);   // (registers only: the barrier below is the load's)
    __syncthreads();
    for (int it = 0; it < k; ++it) {   // colour 0 = even (i + j) first
        solid_tile::half_sweep(c, lds, 0, t, threadIdx.x);
        __syncthreads();
        solid_tile::half_sweep(c, lds, 1, t, threadIdx.x);
        __syncthreads();
    }
    solid_tile::store(c, t, threadIdx.x);
}

// ---- one thread per cell -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kStreamThreads)
open_divergence_kernel(float *__restrict__ div, float *v, const uint8_t *__restrict__ codes, const uint8_t *__restrict__ open, int dim_x, size_t cells,
                        float two_dx_inv, bool zero_solids)
{
    const size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (c >= cells) return;
    const int code = open_code(codes, open, c);
    float2 *q = reinterpret_cast<float2 *>(v) + c;
    if (code & kSolidFluid) {
        div[c] = divergence_sum_open(q, dim_x, code) * two_dx_inv;
    } else {   // (no fluid cell reads a solid cell's velocity: the store races with nothing)
        div[c] = 0.0f;
        if (zero_solids) *q = make_float2(0.0f, 0.0f);
    }
}

__global__ void __launch_bounds__(kStreamThreads)
open_gradient_kernel(float *__restrict__ v, const float *__restrict__ p, const uint8_t *__restrict__ codes, const uint8_t *__restrict__ open, int dim_x,
                      size_t cells, float two_dx_inv)
{
    const size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x;
    if (c >= cells) return;
    float2 *q = reinterpret_cast<float2 *>(v) + c;
    *q = project_cell_open(*q, p + c, dim_x, open_code(codes, open, c), two_dx_inv);
}

// the workgroup's maximum of m into *worst (update_norm.hip's reduction)
__device__ __forceinline__ void reduce_max(unsigned m, unsigned *worst)
{
    __shared__ unsigned wave_worst[kStreamWaves];
    for (int o = 32; o > 0; o >>= 1) {   // the wave's maximum
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) wave_worst[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < kStreamWaves; ++k) m = wave_worst[k] > m ? wave_worst[k] : m;
        atomicMax(worst, m);
    }
}

__global__ void __launch_bounds__(kStreamThreads)
open_update_norm_kernel(const float *__restrict__ p, const float *__restrict__ d, const uint8_t *__restrict__ codes, const uint8_t *__restrict__ open, int dim_x,
                         size_t cells, float dx, unsigned *__restrict__ worst)
{
    unsigned m = 0u;
    for (size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kStreamThreads) {
        const int code = open_code(codes, open, c);
        const int present = open_tile::neighbours_of(code & 0xff, code >> kOpenShift);   // n of item 5
        const float w = (code & kSolidW) ? p[c - 1] : -0.0f;
        const float e = (code & kSolidE) ? p[c + 1] : -0.0f;
        const float s = (code & kSolidS) ? p[c - dim_x] : -0.0f;
        const float n = (code & kSolidN) ? p[c + dim_x] : -0.0f;
        const float p_gs = solid_tile::gauss_seidel(dx * d[c], solid_tile::k_factor(present), solid_tile::z_term(solid_tile::present_of(code & 0xff)), w, e, s, n);
        const unsigned bits = __float_as_uint(p_gs - p[c]) & 0x7fffffffu;   // |p_gs - p|
        if (code & kSolidFluid) m = bits > m ? bits : m;   // (a solid cell has no say)
    }
    reduce_max(m, worst);
}

__global__ void __launch_bounds__(kStreamThreads)
open_max_divergence_kernel(const float *__restrict__ v, const uint8_t *__restrict__ codes, const uint8_t *__restrict__ open, int dim_x, size_t cells, float two_dx_inv,
                            unsigned *__restrict__ worst)
{
    unsigned m = 0u;
    const float2 *q = reinterpret_cast<const float2 *>(v);
    for (size_t c = (size_t)blockIdx.x * kStreamThreads + threadIdx.x; c < cells; c += (size_t)gridDim.x * kStreamThreads) {
        const int code = open_code(codes, open, c);
        const float sum = divergence_sum_open(q + c, dim_x, code);
        const float dv = (code & kSolidFluid) ? sum * two_dx_inv : 0.0f;
        const unsigned bits = __float_as_uint(dv) & 0x7fffffffu;
        m = bits > m ? bits : m;
    }
    reduce_max(m, worst);
}

inline unsigned blocks_of(size_t cells) { return (unsigned)((cells + kStreamThreads - 1) / kStreamThreads); }
inline unsigned capped_blocks_of(size_t cells) { return std::min<unsigned>(blocks_of(cells), kMaxBlocks); }

}  // namespace

hipError_t launch_open_inflow(hipStream_t s, float *v, const uint32_t *cells, int n, float inflow_x, float inflow_y)
{
    if (n <= 0) return hipSuccess;
    open_inflow_kernel<<<blocks_of((size_t)n), kStreamThreads, 0, s>>>(v, cells, n, make_float2(inflow_x, inflow_y));
    return hipGetLastError();
}

hipError_t launch_open_divergence(hipStream_t s, float *div, float *v, const uint8_t *codes, const uint8_t *open, int dim_x, int dim_y,
                                   float two_dx_inv, bool zero_solids)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    if (cells == 0) return hipSuccess;
    open_divergence_kernel<<<blocks_of(cells), kStreamThreads, 0, s>>>(div, v, codes, open, dim_x, cells, two_dx_inv, zero_solids);
    return hipGetLastError();
}

hipError_t launch_open_gradient(hipStream_t s, float *v, const float *p, const uint8_t *codes, const uint8_t *open, int dim_x, int dim_y,
                                 float two_dx_inv)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    if (cells == 0) return hipSuccess;
    open_gradient_kernel<<<blocks_of(cells), kStreamThreads, 0, s>>>(v, p, codes, open, dim_x, cells, two_dx_inv);
    return hipGetLastError();
}

hipError_t launch_open_sor(hipStream_t s, float *p_out, const float *p_in, const float *d, const uint8_t *codes, const uint8_t *open, int dim_x,
                            int dim_y, int k, SorParams prm)
{
    if (k < 1 || k > solid_tile::kD || p_out == p_in || dim_x < 1 || dim_y < 1) return hipErrorInvalidValue;
    const int64_t tiles = (int64_t)solid_tile::tiles_x(dim_x) * solid_tile::tiles_y(dim_y);   // one workgroup each, in one dimension
    if (tiles > INT32_MAX) return hipErrorInvalidValue;   // (a context holds 2^28 cells at most: 2^22 tiles and a ragged rim)
    open_sor_kernel<<<(unsigned)tiles, solid_tile::kThreads, 0, s>>>(p_out, p_in, d, codes, open, dim_x, dim_y, k, prm);
    return hipGetLastError();
}

hipError_t launch_open_update_norm(hipStream_t s, unsigned *worst, const float *p, const float *d, const uint8_t *codes, const uint8_t *open,
                                    int dim_x, int dim_y, float dx)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    hipError_t e = hipMemsetAsync(worst, 0, sizeof(unsigned), s);
    if (e != hipSuccess || cells == 0) return e;
    open_update_norm_kernel<<<capped_blocks_of(cells), kStreamThreads, 0, s>>>(p, d, codes, open, dim_x, cells, dx, worst);
    return hipGetLastError();
}

hipError_t launch_open_max_divergence(hipStream_t s, unsigned *worst, const float *v, const uint8_t *codes, const uint8_t *open, int dim_x,
                                       int dim_y, float two_dx_inv)
{
    const size_t cells = (size_t)dim_x * (size_t)dim_y;
    hipError_t e = hipMemsetAsync(worst, 0, sizeof(unsigned), s);
    if (e != hipSuccess || cells == 0) return e;
    open_max_divergence_kernel<<<capped_blocks_of(cells), kStreamThreads, 0, s>>>(v, codes, open, dim_x, cells, two_dx_inv, worst);
    return hipGetLastError();
}

}  // namespace sfl
