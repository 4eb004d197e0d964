// history_pass_probe.hip -- one sample of a batch's history taken several ways on ONE stream, device events around each:
// the sampler of csrc/history.hip (one launch; at each of its three workgroup sizes and at the one the library chooses)
// against the passes that existed before it (csrc/flow_stats.hip: the memset and the two launches of launch_flow_stats).
// The update norm has no launch of its own for a batch -- update_norm.hip takes ONE field, a batch would need a launch per
// member -- so the old way is timed without it, and once more with ONE launch of update_norm.hip over the batch's pressure
// taken as a single field of members x dim_y rows: what such a pass would COST (8 B per cell), not a result -- its
// stencil reads across the members' seams.
// Built from the product's own sources (tools/history_probe.py has the command line and runs the binary):
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math tools/history_pass_probe.hip \
//         esp32-fluid-simulation_amd/csrc/history.hip esp32-fluid-simulation_amd/csrc/flow_stats.hip \
//         esp32-fluid-simulation_amd/csrc/update_norm.hip -o tools/history_pass_probe
//   tools/history_pass_probe DIM_X DIM_Y MEMBERS [ROUNDS [LAUNCHES]]
// Rounds alternate the ways; a round times LAUNCHES samples back to back and reports the time of one.  The fields are
// seeded noise: no way's time depends on the values.  All write the same maxima and sums, which is checked.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "../esp32-fluid-simulation_amd/csrc/history_kernels.h"
#include "../esp32-fluid-simulation_amd/csrc/stats_kernels.h"
#include "../esp32-fluid-simulation_amd/csrc/until_kernels.h"

#define TRY(expr)                                                                             \
    do {                                                                                      \
        hipError_t e_ = (expr);                                                               \
        if (e_ != hipSuccess) {                                                               \
            fprintf(stderr, "%s failed: %s (line %d)\n", #expr, hipGetErrorString(e_), __LINE__); \
            return 2;                                                                         \
        }                                                                                     \
    } while (0)

static double median(std::vector<float> v)
{
    std::sort(v.begin(), v.end());
    return v.size() % 2 ? v[v.size() / 2] : 0.5 * (v[v.size() / 2 - 1] + v[v.size() / 2]);
}

int main(int argc, char **argv)
{
    if (argc < 4) {
        fprintf(stderr, "usage: %s DIM_X DIM_Y MEMBERS [ROUNDS [LAUNCHES]]\n", argv[0]);
        return 2;
    }
    const int dim_x = atoi(argv[1]), dim_y = atoi(argv[2]), members = atoi(argv[3]);
    const int rounds = argc > 4 ? atoi(argv[4]) : 9, launches = argc > 5 ? atoi(argv[5]) : 200;
    if (!sfl::large_member_fits(dim_x, dim_y) || members < 1 || rounds < 1 || launches < 1) {
        fprintf(stderr, "a member of %d x %d is not one a batch holds, or a count is < 1\n", dim_x, dim_y);
        return 2;
    }
    const size_t cells = (size_t)dim_x * dim_y * members;
    std::vector<uint32_t> noise(3 * cells);
    uint32_t x = 2463534242u;
    for (uint32_t &w : noise) {   // xorshift32
        x ^= x << 13;
        x ^= x >> 17;
        x ^= x << 5;
        w = x;
    }
    float *vel = nullptr, *p = nullptr, *d = nullptr;
    uint32_t *dye = nullptr;
    sfl_history_record *rec = nullptr;
    sfl::FlowStatsRecord *stats = nullptr;
    TRY(hipMalloc((void **)&vel, cells * 8));
    TRY(hipMalloc((void **)&p, cells * 4));
    TRY(hipMalloc((void **)&d, cells * 4));
    TRY(hipMalloc((void **)&dye, cells * 12));
    TRY(hipMalloc((void **)&rec, sizeof(sfl_history_record) * members));
    TRY(hipMalloc((void **)&stats, sizeof(sfl::FlowStatsRecord) * members));
    std::vector<float> floats(2 * cells);
    for (size_t k = 0; k < 2 * cells; ++k) floats[k] = (float)(int32_t)noise[k] * (1.0f / 67108864.0f);   // +-32, no NaN
    TRY(hipMemcpy(vel, floats.data(), cells * 8, hipMemcpyHostToDevice));
    TRY(hipMemcpy(p, floats.data(), cells * 4, hipMemcpyHostToDevice));
    TRY(hipMemcpy(d, floats.data() + cells, cells * 4, hipMemcpyHostToDevice));
    TRY(hipMemcpy(dye, noise.data(), cells * 12, hipMemcpyHostToDevice));
    hipStream_t s;
    hipEvent_t e0, e1;
    TRY(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
    TRY(hipEventCreate(&e0));
    TRY(hipEventCreate(&e1));
    const float dx = 0.75f, two_dx_inv = 1.0f / (2.0f * dx);
    sfl::HistorySample a{};
    a.vel = vel, a.dye = dye, a.p = p, a.d = d;
    a.dim_x = dim_x, a.dim_y = dim_y, a.first = 0, a.count = members, a.batch = members;
    a.step = 1, a.dt = 0.05f, a.dx = dx, a.two_dx_inv = two_dx_inv, a.iters = 20;
    a.out = rec;
    unsigned *worst = nullptr;
    TRY(hipMalloc((void **)&worst, sizeof(unsigned)));
    const sfl::Slab all{dim_x, dim_y * members, 0, dim_y * members};   // the batch's pressure as ONE field (cost only)
    const auto passes = [&] { return sfl::launch_flow_stats(s, stats, SFL_STATS_VELOCITY | SFL_STATS_DYE, vel, dye, dim_x, dim_y, members, two_dx_inv, nullptr); };
    const auto way = [&](int which) {
        switch (which) {
            case 0: return sfl::launch_history_sample(s, a, 0);
            case 1: return sfl::launch_history_sample(s, a, 256);
            case 2: return sfl::launch_history_sample(s, a, 512);
            case 3: return sfl::launch_history_sample(s, a, 1024);
            case 4: return passes();
            default: {
                const hipError_t e = passes();
                return e != hipSuccess ? e : sfl::launch_update_norm(s, worst, p, d, all, 0, all.gdim_y, dx);
            }
        }
    };
    const char *names[6] = {"the sampler as the library launches it (one launch)", "  ... forced to 256 threads", "  ... forced to 512 threads",
                            "  ... forced to 1024 threads", "the passes of before (memset + 2 launches), NO update norm",
                            "  ... + one update-norm launch's COST (not a result)"};
    const double bytes_per_cell[6] = {28, 28, 28, 28, 20, 28};
    std::vector<float> us[6];
    for (int r = -2; r < rounds; ++r)   // (two rounds of warm-up)
        for (int which = 0; which < 6; ++which) {
            TRY(hipEventRecord(e0, s));
            for (int k = 0; k < launches; ++k) TRY(way(which));
            TRY(hipEventRecord(e1, s));
            TRY(hipEventSynchronize(e1));
            float ms = 0.0f;
            TRY(hipEventElapsedTime(&ms, e0, e1));
            if (r >= 0) us[which].push_back(1000.0f * ms / launches);
        }
    std::vector<sfl_history_record> h_rec(members);
    std::vector<sfl::FlowStatsRecord> h_stats(members);
    TRY(hipMemcpy(h_rec.data(), rec, sizeof(sfl_history_record) * members, hipMemcpyDeviceToHost));
    TRY(hipMemcpy(h_stats.data(), stats, sizeof(sfl::FlowStatsRecord) * members, hipMemcpyDeviceToHost));
    int differ = 0;
    for (int m = 0; m < members; ++m)
        differ += memcmp(&h_rec[m], &h_stats[m], 12) != 0 || memcmp(h_rec[m].dye_sum, h_stats[m].dye_sum, 24) != 0;
    printf("  %d x %d x %d members, %d rounds of %d samples back to back on one stream, device events; %.1f MB per sample at 28 B per cell\n", dim_x,
           dim_y, members, rounds, launches, 28.0 * cells / 1e6);
    for (int which = 0; which < 6; ++which) {
        const double med = median(us[which]);
        printf("  %-60s median %8.2f us   min %8.2f   max %8.2f   %6.0f GB/s of %2.0f B per cell\n", names[which], med,
               *std::min_element(us[which].begin(), us[which].end()), *std::max_element(us[which].begin(), us[which].end()),
               bytes_per_cell[which] * cells / 1e6 / med * 1e3, bytes_per_cell[which]);
    }
    printf("  members whose maxima or sums differ between the sampler and the passes: %d\n", differ);
    return differ ? 1 : 0;
}
