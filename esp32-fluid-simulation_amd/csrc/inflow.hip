// inflow.hip -- inflow profiles and the flux through the openings (gfx950 / MI355X; include/sfl.h "INFLOW PROFILES AND
// FLUX"): item 2a of a context with a profile, and the flux record of a batch member and of a context.  New kernels;
// every other unit keeps its text.  (The step of a batch with a profile is the kProfile instantiation of
// batch_member.h's step_in_lds, in batch_openings.hip.)
//
//   open_inflow_profile_kernel   v[cells[k]] = values[k] over the compact list of the fluid inflow cells: the host
//                                (context_openings.cpp) forms `values` beside the list -- a record's velocity where the
//                                profile has one, the uniform inflow elsewhere.
//   open_flux_kernel             ONE workgroup per grid that walks only the 2 (dim_x + dim_y) - 4 rim cells
//                                (open_flux.h): pass 1 the counts and the maximum of the bit patterns of |n|, reduced by
//                                __shfl_xor in the wave and through LDS between the waves; barrier; pass 2 the terms by the
//                                finished maximum into two 64-bit sums per lane, reduced the same way; thread 0 stores
//                                the record with ordinary stores.  No atomics, no memset in front, no float is added.  A
//                                batch runs it with 256 threads per member (a member's rim has at most a few hundred
//                                cells), a context with one workgroup of 1024 (8192 x 8192: 32 764 cells, 32 per lane, the
//                                W and E cells at a stride of a row -- a latency-bound kernel of some microseconds whose
//                                second pass hits the cache, instead of two launches with atomics on a zeroed record).
// Integer sums, counts and maxima of bit patterns: the record does not depend on the order of reduction, and a batch
// member and a context of the same shape write the same bytes.
#include "batch.h"
#include "open_flux.h"
#include "open_kernels.h"

namespace sfl {
namespace {

using namespace open_flux;

constexpr int kStreamThreads = 256;
constexpr int kBatchFluxThreads = 256, kContextFluxThreads = 1024;

__global__ void __launch_bounds__(kStreamThreads)
open_inflow_profile_kernel(float *__restrict__ v, const uint32_t *__restrict__ cells, const float *__restrict__ values, int n)
{
    const int k = blockIdx.x * kStreamThreads + threadIdx.x;
    if (k < n) reinterpret_cast<float2 *>(v)[cells[k]] = reinterpret_cast<const float2 *>(values)[k];
}

// the open bits of a cell: bits 8..12 of a batch's open code, the open byte of a context
struct CodeBits {
    const uint16_t *codes;
    __device__ __forceinline__ unsigned operator()(int c) const { return (unsigned)codes[c] >> 8 & 31u; }
};
struct ByteBits {
    const uint8_t *open;
    __device__ __forceinline__ unsigned operator()(int c) const { return (unsigned)open[c] & 31u; }
};

template <class T>
__device__ __forceinline__ T wave_sum(T x)
{
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    return x;
}

// the record of the grid at v with the open bits `open`, by the workgroup
template <int kThreads, class Open>
__device__ __forceinline__ void flux_of_grid(struct sfl_open_flux *out, const float2 *__restrict__ v, Open open, int dim_x, int dim_y)
{
    constexpr int kWaves = kThreads / 64;
    __shared__ unsigned s_max[kWaves], s_count[kWaves][3];
    __shared__ long long s_sum[kWaves][2];
    const int rim = rim_cells(dim_x, dim_y), wave = threadIdx.x >> 6;
    Partial part = {0u, 0u, 0u, 0u, 0, 0};
    // ---- pass 1: the counts and the maximum
    for (int r = threadIdx.x; r < rim; r += kThreads) {
        const int c = rim_cell(r, dim_x, dim_y);
        const unsigned o = open(c);
        if (!(o & kSides)) continue;
        const float2 u = v[c];
        gather_max(part, o, normal_bits(o, __float_as_uint(u.x), __float_as_uint(u.y)));
    }
    unsigned m = part.max_bits;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned t = __shfl_xor(m, o);
        m = t > m ? t : m;
    }
    if ((threadIdx.x & 63) == 0) s_max[wave] = m;
    __syncthreads();
    m = s_max[0];
#pragma unroll
    for (int k = 1; k < kWaves; ++k) m = s_max[k] > m ? s_max[k] : m;
    part.max_bits = m;
    const int q = exp2_of(m);
    // ---- pass 2: the terms
    for (int r = threadIdx.x; r < rim; r += kThreads) {
        const int c = rim_cell(r, dim_x, dim_y);
        const unsigned o = open(c);
        if (!(o & kSides)) continue;
        const float2 u = v[c];
        gather_term(part, o, normal_bits(o, __float_as_uint(u.x), __float_as_uint(u.y)), q);
    }
    part.in = wave_sum(part.in);
    part.out = wave_sum(part.out);
    part.in_cells = wave_sum(part.in_cells);
    part.out_cells = wave_sum(part.out_cells);
    part.nonfinite = wave_sum(part.nonfinite);
    if ((threadIdx.x & 63) == 0) {
        s_sum[wave][0] = part.in;
        s_sum[wave][1] = part.out;
        s_count[wave][0] = part.in_cells;
        s_count[wave][1] = part.out_cells;
        s_count[wave][2] = part.nonfinite;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 1; k < kWaves; ++k) {
            part.in += s_sum[k][0];
            part.out += s_sum[k][1];
            part.in_cells += s_count[k][0];
            part.out_cells += s_count[k][1];
            part.nonfinite += s_count[k][2];
        }
        finish(out, part);
    }
}

__global__ void __launch_bounds__(kBatchFluxThreads)
batch_open_flux_kernel(struct sfl_open_flux *__restrict__ out, const float *__restrict__ v, const uint16_t *__restrict__ codes, size_t member_stride,
                       int dim_x, int dim_y)
{
    const size_t member = blockIdx.x;   // (of the range: every pointer is at its first member)
    const float2 *q = reinterpret_cast<const float2 *>(v) + member * (size_t)dim_x * (size_t)dim_y;
    flux_of_grid<kBatchFluxThreads>(out + member, q, CodeBits{codes + member * member_stride}, dim_x, dim_y);
}

__global__ void __launch_bounds__(kContextFluxThreads)
open_flux_kernel(struct sfl_open_flux *__restrict__ out, const float *__restrict__ v, const uint8_t *__restrict__ open, int dim_x, int dim_y)
{
    flux_of_grid<kContextFluxThreads>(out, reinterpret_cast<const float2 *>(v), ByteBits{open}, dim_x, dim_y);
}

}  // namespace

hipError_t launch_open_inflow_profile(hipStream_t s, float *v, const uint32_t *cells, const float *values, int n)
{
    if (n <= 0) return hipSuccess;
    open_inflow_profile_kernel<<<(unsigned)((n + kStreamThreads - 1) / kStreamThreads), kStreamThreads, 0, s>>>(v, cells, values, n);
    return hipGetLastError();
}

hipError_t launch_open_flux(hipStream_t s, struct sfl_open_flux *out, const float *v, const uint8_t *open, int dim_x, int dim_y)
{
    if (dim_x < 2 || dim_y < 2) return hipErrorInvalidValue;
    open_flux_kernel<<<1, kContextFluxThreads, 0, s>>>(out, v, open, dim_x, dim_y);
    return hipGetLastError();
}

hipError_t launch_batch_open_flux(hipStream_t s, struct sfl_open_flux *out, const float *v, const BatchOpenings &open, int dim_x, int dim_y,
                                  int first, int count)
{
    if (count <= 0) return hipSuccess;
    if (dim_x < 2 || dim_y < 2 || first < 0) return hipErrorInvalidValue;
    batch_open_flux_kernel<<<(unsigned)count, kBatchFluxThreads, 0, s>>>(out, v + 2 * (size_t)first * dim_x * dim_y,
                                                                          open.codes + (size_t)first * open.member_stride, open.member_stride, dim_x, dim_y);
    return hipGetLastError();
}

}  // namespace sfl
