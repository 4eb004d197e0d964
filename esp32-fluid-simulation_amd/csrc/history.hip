// history.hip -- the sampler of a batch's history (gfx950 / MI355X; include/sfl.h "HISTORIES"): one struct
// sfl_history_record per recorded member in ONE launch, one workgroup per member, launched on the batch's stream behind
// the step whose fields it reads.
//
// A member is at most kLargeMemberMaxCells = 20224 cells, so one workgroup walks all of it and nothing has to be
// combined across workgroups: no global atomics and no memset in front (the passes of flow_stats.hip and
// update_norm.hip spread a field over many workgroups and need both).  Three passes, each thread striding over the
// member by the workgroup's size:
//   velocity  the maxima of |v.x|, |v.y| and |calculate_divergence(v, dx)| as bit patterns (flow_stats.hip's
//             definition): advect_math.h's divergence_sum on a 3 x 3 window in registers, times 1 / (2 dx).  Four cells
//             per trip, the 20 loads of all four issued in front of their arithmetic, every load unconditional and
//             inside the member.  8 B per cell from memory; the four neighbours' words come from the cache lines the
//             neighbouring lanes and rows fetch;
//   p and d   the update norm: small_grid_core.h's update_norm_in_lds, whose pointers are generic, on the arrays in
//             memory.  8 B per cell;
//   dye       three exact 64-bit sums over the member's 3 * cells raw words taken as ONE stream of 4-byte loads,
//             consecutive lanes on consecutive words: right at any base (member m starts at word 3 * cells * m, which is
//             16-byte aligned only when cells is a multiple of 4).  A thread's k-th word is word t + k * kT, so its
//             channel is (t + k * kT) mod 3: three sums by k mod 3 -- a compile-time index, six loads per trip -- rotated
//             into channels once, at the end (kT is no multiple of 3).  12 B per cell.
// 28 B per cell and sample.  Reductions: __shfl_xor in the wave, LDS across the waves, thread 0 stores the 64 bytes with
// ordinary stores.  Maxima over bit patterns and integer sums do not depend on the order of reduction.
// The workgroup: 1024 threads for members of more than kSmallGridMaxCells cells -- a batch of them runs one member per
// CU, and sixteen waves keep more loads in flight than eight (27 us against 34 at 128 x 128 x 256) -- and 256 for smaller
// ones, where a thread of 1024 would own five cells (31 us against 42 at 61 x 81 x 1024): profiles/history.txt.
// Compiler's figures (-Rpass-analysis=kernel-resource-usage): no scratch at any of the three sizes.
//
// Numerics contract: -ffp-contract=off, every operation individually rounded in the reference's order.
#include "advect_math.h"
#include "history_kernels.h"
#include "small_grid_core.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

static_assert(sizeof(struct sfl_history_record) == 64, "include/sfl.h: 64 bytes");

__device__ __forceinline__ unsigned max_abs_bits(unsigned m, float x)
{
    const unsigned bits = __float_as_uint(x) & 0x7fffffffu;   // |x|
    return bits > m ? bits : m;
}

template <int kT>
__global__ void __launch_bounds__(kT) history_sample_kernel(const HistorySample a)
{
    constexpr int kWaves = kT / 64;
    static_assert(kT % 64 == 0 && kT % 3 != 0, "whole waves; a thread's consecutive dye words fall on all three channels");
    __shared__ unsigned wave_max[kWaves][3];
    __shared__ u64 wave_sum[kWaves][3];
    __shared__ float norm;
    // ---- which member, and the parameters its step ran with (workgroup-uniform)
    int member = a.first + (int)blockIdx.x, iters = a.iters;
    float dt = a.dt, dx = a.dx, two_dx_inv = a.two_dx_inv;
    if (a.members) {   // one workgroup per record of the launch's table: the record names its member
        const BatchMember rec = a.members[blockIdx.x];
        member = rec.member;
        if (member < a.first || member >= a.first + a.count) return;   // (not recorded)
        dt = rec.dt;
        dx = rec.prm.dx;
        two_dx_inv = rec.two_dx_inv;
        iters = rec.iters;
    }
    if (a.counts) iters = a.counts[2 * (size_t)member];   // the k the stopping rule ended this step's solve at
    const int dim_x = a.dim_x, dim_y = a.dim_y, cells = dim_x * dim_y, i_max = dim_x - 1, j_max = dim_y - 1;
    const size_t base = (size_t)member * (size_t)cells;   // in cells; offsets inside the member are 32-bit
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;

    // ---- the velocity: (gj, i) of the thread's cells by stepping, as update_norm_in_lds walks; four cells per trip, the
    // loads of all four in front of their arithmetic.  Every load is unconditional and inside the member (a neighbour the
    // field does not have is loaded from the cell itself; divergence_sum does not read it there)
    unsigned m[3] = {0u, 0u, 0u};
    {
        const float2 *v = reinterpret_cast<const float2 *>(a.vel) + base;
        const int step_j = kT / dim_x, step_i = kT - step_j * dim_x;
        int gj = (int)threadIdx.x / dim_x, i = (int)threadIdx.x - gj * dim_x;
        struct Cell {
            float2 own;
            float wx, ex, sy, ny;
            int i, gj;
            bool have;
        };
        const auto fetch = [&](int c) {
            Cell q;
            q.have = c < cells;
            if (i >= dim_x) {
                i -= dim_x;
                ++gj;
            }
            q.i = i;
            q.gj = gj;
            const int cc = q.have ? c : 0;
            const int west = (q.have && i > 0) ? 1 : 0, east = (q.have && i < i_max) ? 1 : 0;
            const int south = (q.have && gj > 0) ? dim_x : 0, north = (q.have && gj < j_max) ? dim_x : 0;
            q.own = v[cc];
            q.wx = v[cc - west].x;
            q.ex = v[cc + east].x;
            q.sy = v[cc - south].y;
            q.ny = v[cc + north].y;
            gj += step_j;
            i += step_i;
            return q;
        };
        const auto fold = [&](const Cell &q) {
            // the cell's neighbourhood as divergence_sum addresses it: a 3 x 3 window, rows 3 apart, the cell in the middle
            float2 win[9] = {};
            win[4] = q.own;
            win[3].x = q.wx;
            win[5].x = q.ex;
            win[1].y = q.sy;
            win[7].y = q.ny;
            const float d = advect_math::divergence_sum(win + 4, 3, q.i, q.gj, i_max, j_max) * two_dx_inv;
            if (q.have) {
                m[0] = max_abs_bits(m[0], q.own.x);
                m[1] = max_abs_bits(m[1], q.own.y);
                m[2] = max_abs_bits(m[2], d);
            }
        };
        for (int c = threadIdx.x; c < cells; c += 4 * kT) {
            const Cell q0 = fetch(c), q1 = fetch(c + kT), q2 = fetch(c + 2 * kT), q3 = fetch(c + 3 * kT);
            fold(q0);
            fold(q1);
            fold(q2);
            fold(q3);
        }
    }
    // ---- the dye: one stream of words, six loads in front of their sums
    u64 t0 = 0, t1 = 0, t2 = 0;   // by the position k mod 3 of the word among the thread's
    {
        const uint32_t *dye = a.dye + 3 * base;
        const int words = 3 * cells;
        int w = threadIdx.x;
        for (; w + 5 * kT < words; w += 6 * kT) {
            const uint32_t x0 = dye[w], x1 = dye[w + kT], x2 = dye[w + 2 * kT], x3 = dye[w + 3 * kT], x4 = dye[w + 4 * kT], x5 = dye[w + 5 * kT];
            t0 += x0;
            t1 += x1;
            t2 += x2;
            t0 += x3;
            t1 += x4;
            t2 += x5;
        }
        for (; w + 2 * kT < words; w += 3 * kT) {
            const uint32_t x0 = dye[w], x1 = dye[w + kT], x2 = dye[w + 2 * kT];
            t0 += x0;
            t1 += x1;
            t2 += x2;
        }
        if (w < words) t0 += dye[w];
        if (w + kT < words) t1 += dye[w + kT];
    }
    u64 s[3];
    {
        const int r0 = (int)threadIdx.x % 3, r1 = ((int)threadIdx.x + kT) % 3, r2 = ((int)threadIdx.x + 2 * kT) % 3;   // distinct
#pragma unroll
        for (int k = 0; k < 3; ++k) s[k] = (r0 == k ? t0 : 0) + (r1 == k ? t1 : 0) + (r2 == k ? t2 : 0);
    }
    // ---- the wave's maxima and sums, then the workgroup's through LDS
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const unsigned t = __shfl_xor(m[k], o);
            m[k] = t > m[k] ? t : m[k];
            s[k] += __shfl_xor(s[k], o);
        }
        if (lane == 0) {
            wave_max[wave][k] = m[k];
            wave_sum[wave][k] = s[k];
        }
    }
    // ---- the update norm of the pressure and divergence the step left (its barriers also publish the words above)
    small_core::update_norm_in_lds<kT>(a.p + base, a.d + base, dim_x, dim_y, dx, &norm);
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k)
#pragma unroll
            for (int w = 1; w < kWaves; ++w) {
                m[k] = wave_max[w][k] > m[k] ? wave_max[w][k] : m[k];
                s[k] += wave_sum[w][k];
            }
        struct sfl_history_record r;
        r.max_abs_vx = __uint_as_float(m[0]);
        r.max_abs_vy = __uint_as_float(m[1]);
        r.max_abs_div = __uint_as_float(m[2]);
        r.what = SFL_STATS_VELOCITY | SFL_STATS_DYE;
        r.dye_sum[0] = s[0];
        r.dye_sum[1] = s[1];
        r.dye_sum[2] = s[2];
        r.update_norm = norm;
        r.iterations = iters;
        r.step = a.step;
        r.dt = dt;
        r.dx = dx;
        a.out[member - a.first] = r;
    }
}

}  // namespace

hipError_t launch_history_sample(hipStream_t s, const HistorySample &a, int threads)
{
    // A member the one-workgroup kernels hold (at most kSmallGridMaxCells cells) gives a thread of the large workgroup too
    // few cells to keep loads in flight; a large member gives the small workgroup too few waves per CU (one member per CU):
    // profiles/history.txt has both measured both ways
    if (threads == 0) threads = (long long)a.dim_x * a.dim_y > kSmallGridMaxCells ? kHistoryThreads : kHistoryThreadsSmall;
    const int grid = a.members ? a.batch : a.count;
    switch (threads) {
        case 256: history_sample_kernel<256><<<grid, 256, 0, s>>>(a); break;
        case 512: history_sample_kernel<512><<<grid, 512, 0, s>>>(a); break;
        case 1024: history_sample_kernel<1024><<<grid, 1024, 0, s>>>(a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace sfl
