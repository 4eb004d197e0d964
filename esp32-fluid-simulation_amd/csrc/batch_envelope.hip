// batch_envelope.hip -- the per-cell envelope of the dye over the members of a batch (gfx950 / MI355X): mean, minimum,
// maximum and spread of every word over `count` members.  What sfl_batch_envelope leaves on the device (include/sfl.h).
//
// All four are exact integers -- unsigned minima and maxima, a 64-bit sum divided once -- so nothing depends on the
// order of reduction.  Bound by memory: every member is read once, 12 B per cell.
//   * the members of one word lie 12 * cells bytes apart, and a member holds few words (the sketch's 61 x 81: 14,823), so
//     one thread per word walking all members would leave most of the chip idle, waiting for one load at a time.  The
//     members are split into GROUPS of kEnvGroupMembers over the grid's x (a batch may hold millions of tiny members), the
//     words into blocks of kEnvBlockWords over its y (at most 237): 1024 sketch members are 32 x 58 workgroups;
//   * a thread owns ONE word and loads it from eight members in front of their arithmetic; every load of the wave is
//     256 B contiguous and asks for 4-byte alignment only, so a member stride that is no multiple of 16 B (the sketch's
//     59,292 B) costs nothing extra and needs no head or tail;
//   * a group leaves its partial sum (64-bit), minimum and maximum with plain stores; a second launch combines the groups
//     in group order and writes the four fields.  No atomics: deterministic by construction.  A range of one group takes
//     the same two launches.
// Member bases are formed in 64-bit, the word inside a member is 32-bit.
#include "../../include/sfl.h"
#include "ensemble_kernels.h"

namespace sfl {
namespace {

typedef unsigned long long u64;

constexpr int kLoads = 8;   // members whose loads are in flight together
static_assert(kEnvGroupMembers % kLoads == 0, "a group is walked in rounds of kLoads members");

// partials: sums of all groups first (8-byte aligned), then the minima, then the maxima; group g's at g * member_words
__global__ void __launch_bounds__(kEnvBlockWords)
envelope_group_kernel(const uint32_t *__restrict__ dye, size_t member_words, int count, u64 *__restrict__ sums,
                      uint32_t *__restrict__ minima, uint32_t *__restrict__ maxima)
{
    const unsigned w = blockIdx.y * kEnvBlockWords + threadIdx.x;
    if (w >= member_words) return;
    const int group = blockIdx.x, m0 = group * kEnvGroupMembers, m1 = min(m0 + kEnvGroupMembers, count);   // workgroup-uniform
    const uint32_t *p = dye + (size_t)m0 * member_words + w;
    u64 sum = 0;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int m = m0; m < m1; m += kLoads) {
        uint32_t x[kLoads];
        // (a member past the range is loaded from the range's last one and not read)
#pragma unroll
        for (int k = 0; k < kLoads; ++k) x[k] = p[(size_t)min(k, m1 - 1 - m) * member_words];
#pragma unroll
        for (int k = 0; k < kLoads; ++k)
            if (m + k < m1) {
                sum += x[k];
                lo = x[k] < lo ? x[k] : lo;
                hi = x[k] > hi ? x[k] : hi;
            }
        p += (size_t)kLoads * member_words;
    }
    const size_t at = (size_t)group * member_words + w;
    sums[at] = sum;
    minima[at] = lo;
    maxima[at] = hi;
}

__global__ void __launch_bounds__(kEnvBlockWords)
envelope_finish_kernel(uint32_t *__restrict__ fields, size_t member_words, int count, int groups, const u64 *__restrict__ sums,
                       const uint32_t *__restrict__ minima, const uint32_t *__restrict__ maxima)
{
    const unsigned w = blockIdx.x * kEnvBlockWords + threadIdx.x;
    if (w >= member_words) return;
    u64 sum = 0;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int g = 0; g < groups; ++g) {
        const size_t at = (size_t)g * member_words + w;
        sum += sums[at];
        lo = minima[at] < lo ? minima[at] : lo;
        hi = maxima[at] > hi ? maxima[at] : hi;
    }
    fields[SFL_ENV_MEAN * member_words + w] = (uint32_t)(sum / (u64)count);   // floor; < 2^32: a mean of uint32 values
    fields[SFL_ENV_MIN * member_words + w] = lo;
    fields[SFL_ENV_MAX * member_words + w] = hi;
    fields[SFL_ENV_SPREAD * member_words + w] = hi - lo;
}

}  // namespace

hipError_t launch_batch_envelope(hipStream_t s, uint32_t *fields, uint32_t *partials, const uint32_t *dye, size_t member_words,
                                 int count)
{
    const int groups = envelope_groups(count);
    const unsigned blocks = (unsigned)((member_words + kEnvBlockWords - 1) / kEnvBlockWords);
    u64 *sums = reinterpret_cast<u64 *>(partials);
    uint32_t *minima = partials + 2 * (size_t)groups * member_words, *maxima = minima + (size_t)groups * member_words;
    envelope_group_kernel<<<dim3((unsigned)groups, blocks), kEnvBlockWords, 0, s>>>(dye, member_words, count, sums, minima, maxima);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    envelope_finish_kernel<<<blocks, kEnvBlockWords, 0, s>>>(fields, member_words, count, groups, sums, minima, maxima);
    return hipGetLastError();
}

}  // namespace sfl
