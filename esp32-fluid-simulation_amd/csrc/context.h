// context.h -- what the host-side translation units of libsfl_hip.so share (internal; the public boundary is
// include/sfl.h): the context struct, the error plumbing and the helpers every unit needs.
//
//   context.cpp       errors, device / plan queries, create / destroy, options, field I/O, synchronize, timers
//   transport.{h,cpp} halo transports behind one interface (virtual-rank group, RCCL, emulated rank), the exchange
//                     protocol around them, communicator attach / option check
//   sor_executor.cpp  poisson_solve: walks slab_plan.h programs (in line, early exchanges behind events, exchanges in
//                     time counted on the device)
//   solve_until.cpp   the update norm of a context, a continued solve, a solve stopped at a tolerance
//   flow_stats.cpp    the flow statistics of a context: maximum speeds, remaining divergence, dye totals
//   ensemble.cpp      the distance between two contexts or batch members, the dye envelope of a batch
//   operators.cpp     advection, divergence, projection, forces, setup / render
//   slab_step.cpp     sfl_step / sfl_step_n, the automatic advection halo of a slab's step
//   host_dropin.cpp   the host-pointer drop-ins (sfl_host_*) and their per-thread context
//   tracers.cpp       points that move with the flow (sfl_tracers_*, sfl_batch_tracers_*): sets, advances, samples, trails
//   context_solids.cpp solid cells of a whole-domain context (sfl_set_solids, _solids_info, _solids_download) and the masked launches
//   loads.cpp         the pressure load on solid bodies (sfl_loads*, sfl_batch_loads*, sfl_set_bodies, sfl_batch_set_bodies)
//   friction.cpp      the skin friction on solid bodies (sfl_friction*, sfl_batch_friction*); body_recorder.h: the calls both share
//   torque.cpp        the torque on solid bodies and their pivots (sfl_torque*, sfl_batch_torque*, sfl_[batch_]set_body_pivots)
//   means.cpp         per-cell sums over time of a context or a batch, added while stepping (sfl_mean_*, sfl_batch_mean_*)
//   context_viscous.cpp viscosity of a whole-domain context (sfl_set_viscosity, _viscosity_info, sfl_diffuse_velocity)
//   viscous.cpp       viscosity of a batch (sfl_batch_set_viscosity, _viscosity_info, _viscosity_download)
//   openings.cpp      inflow and outflow cells on the rim of a batch member (sfl_batch_set_openings, _set_inflow, _openings_info, ...)
//   context_openings.cpp  the same on a whole-domain context (sfl_set_openings, _set_inflow, _openings_info, _openings_download), with its
//                     inflow profile and flux (sfl_set_inflow_profile, _inflow_profile_info, _inflow_profile_download, sfl_openings_flux)
//   inflow.cpp        the inflow profile of a batch and the flux through its openings (sfl_batch_set_inflow_profile, ..., sfl_batch_openings_flux)
//
// There is deliberately no CPU compute path in any of them: every operator ends in a kernel launch and fails with
// SFL_ERR_HIP when no device is usable.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <memory>
#include <string>
#include <vector>

#include "../../include/sfl.h"
#include "kernels.h"
#include "slab_plan.h"
#include "wall_table.h"

namespace sfl {
namespace host {

// message of the last failing call on this thread (sfl_last_error)
std::string &last_error();
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

}  // namespace host
}  // namespace sfl

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess)                                                                          \
            return ::sfl::host::fail(e_ == hipErrorOutOfMemory ? SFL_ERR_NOMEM : SFL_ERR_HIP,          \
                                     "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__,  \
                                     __LINE__);                                                        \
    } while (0)

#define SFL_TRY(expr)                  \
    do {                               \
        int rc_ = (expr);              \
        if (rc_ != SFL_OK) return rc_; \
    } while (0)

namespace sfl {
namespace host {

constexpr int kGhostRows = 160;      // ghost rows allocated per side on a slab (nranks > 1): the deepest halo a solve's superstep may use
constexpr int kAdvectGhostRows = 64;  // ... of which an advection's halo may use this many (beyond: the field is gathered)
constexpr int kLegacySorHalo = 64;    // the solve's halo before it was chosen from the measured exchange (still its starting point)
constexpr size_t kAlternateSweepCells = 48u << 20;  // local cells from which successive SOR launches alternate direction
// Reach words of a slab (device ints, atomicMax'ed by backtrace_reach_kernel; zero them first):
//   [0] / [1]  rows the back-traces of the OWNED rows need below / above the slab;  [2] a back-trace left a guessed halo;
//   [3]        rows a cell's sources lie from its own row at most (the dye's tile kernel measures it);
//   [5]        rows the back-traces of the slab's FIRST row need above it, [6] those of its LAST row below it --
//              what the neighbour needs when it advects that row itself as a ghost row (slab_step_auto: the
//              velocity advection covers own +- 1 rows); [4], [7] come with them and are covered by [0] / [1].
// The pinned host copy of a report carries one word more: [8] = the context's "a wait inside a solve gave up" word.
constexpr int kReachWords = 8;
constexpr int kReportWords = kReachWords + 1;

class Transport;
class Group;

// The automatic halo depth of a slab's solves is DECIDED BY TIMING REAL SOLVES (sor_executor.cpp choose_halo): a model with the
// measured exchange as its input names up to three candidate depths, each of the first solves of a kind -- same iteration
// count, fuse depth, tail and schedule -- runs on one of them between two events (every depth gives the same bits), and the
// fastest is kept for that kind from then on (another depth has to beat the legacy one by 1.5 %).
constexpr int kCollectiveWords = 8;   // sfl_context::d_collective
constexpr int kNormWords = 2;         // sfl_context::d_norm / h_norm

struct HaloTuner {
    struct Kind {
        int iters, fuse, tail, in_time;
        bool operator==(const Kind &o) const { return iters == o.iters && fuse == o.fuse && tail == o.tail && in_time == o.in_time; }
    };
    struct Decided {
        Kind kind;
        int halo;
    };
    static constexpr int kCandidates = 3, kSolvesEach = 4;   // (the first round is not timed: new tilings, cold caches)
    static constexpr int kExplore = kCandidates * kSolvesEach;
    std::vector<Decided> decided;
    bool active = false;
    Kind kind{};
    int cand[kCandidates] = {0, 0, 0}, ncand = 0;
    int solve_no = 0;                    // exploratory solves issued so far
    int which[kExplore] = {0};           // the candidate exploratory solve n ran on
    // a pair of events around every exploratory solve, read TOGETHER when the kind is decided: a host wait between two solves
    // would time them in another regime than the one they run in afterwards (the GPU waiting for the host to queue launches
    // favours the plan with fewer launches: the deepest halo was chosen 4 % too slow)
    hipEvent_t ev[2 * kExplore] = {nullptr};
    ~HaloTuner()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// What sfl_set_option stores, with the defaults.  A solve reads these as plain members; everything else the library knows
// about an option is its row of kOptions below.
struct Options {
    int sor_kernel = 0, sor_fuse = 0, advect_halo = 0, sor_rows = 0, sor_lane_cells = 0, sor_halo = 0, fuse_projection = 1,
        advect_kernel = 0, fuse_divergence = 1, small_grid = 1, emulate_wire_us = 0, step_seams = 1, halo_timeout_ms = 0, sor_fold = 0;
    // the two halves of SFL_OPT_EXCHANGE_SCHEDULE: sor_overlap 0 = in line (1); sor_arrival -1 = automatic (the transport's choice,
    // Transport::arrival_by_default), 0 = behind events (2), 1 = in time (3)
    int sor_overlap = 1, sor_arrival = -1;
};

// One row per option number sfl_set_option / sfl_get_option accept.  How a set is checked:
enum OptionCheck {
    kRange,        // lo <= value <= hi
    kZeroOrRange,  // 0, or lo <= value <= hi
    kZeroOrEven,   // 0, or even and lo <= value <= hi
    kBool,         // any value, stored as 0 / 1
    kReadOnly,     // never
};
enum : unsigned {
    kForgetOnChange = 1,  // a CHANGED value forgets the measured exchange and the halo depths chosen from it (context.cpp)
    kForgetOnSet = 2,     // ... every set does
    kGroupWide = 4,       // sfl_group_link copies slab 0's value to the other members
    kHostReset = 8,       // the host drop-ins put a cached context back to the default (host_dropin.cpp)
};
struct OptionRow {
    int id;                // SFL_OPT_*
    int Options::*field;   // where the value lives; null: computed, or not one int (context.cpp handles those by hand)
    OptionCheck check;
    int lo, hi;
    const char *error;     // of a refused set: a printf format that is given (hi, value)
    unsigned flags;
    int block_word;        // RCCL ranks must agree on the value: its word of the option block (transport.cpp); 0: not compared
};
// Flags that look like omissions, and are (first item; closing them changes behaviour and the ABI version, so not
// here): linking a group leaves SFL_OPT_EMULATE_WIRE_US (12) and SFL_OPT_STEP_SEAMS (14) as each slab had them, and RCCL ranks
// never compare SFL_OPT_SOR_ROWS (3), SOR_LANE_CELLS (5), EMULATE_WIRE_US (12), STEP_SEAMS (14) and HALO_TIMEOUT_MS (18).
constexpr OptionRow kOptions[] = {
    {SFL_OPT_SOR_KERNEL, &Options::sor_kernel, kRange, 0, 2, "SOR kernel must be 0, 1 or 2", kGroupWide | kHostReset, 4},
    {SFL_OPT_SOR_FUSE, &Options::sor_fuse, kZeroOrEven, 2, SFL_MAX_FUSE, "fuse must be 0 (auto) or even, 2..%d (got %d)", kGroupWide | kHostReset, 5},
    {SFL_OPT_ADVECT_HALO, &Options::advect_halo, kRange, 0, kAdvectGhostRows, "advect halo must be 0 (auto) or 1..%d rows", kGroupWide, 8},
    // (a change: the timed solves the halo depth was chosen from ran on other tiles)
    {SFL_OPT_SOR_ROWS, &Options::sor_rows, kRange, 0, INT_MAX, "rows per chunk must be >= 0", kForgetOnChange | kGroupWide | kHostReset, 0},
    {SFL_OPT_TRANSPORT, nullptr, kReadOnly, 0, 0, "SFL_OPT_TRANSPORT is read-only: use sfl_comm_attach / sfl_group_link", 0, 0},
    {SFL_OPT_SOR_LANE_CELLS, &Options::sor_lane_cells, kZeroOrRange, 2, 2,
     "cells per lane must be 0 (auto) or 2 (the packed 4-cell flavour of round 1 is gone: never faster)", kGroupWide | kHostReset, 0},
    {SFL_OPT_SOR_HALO, &Options::sor_halo, kZeroOrRange, 2, kGhostRows, "SOR halo must be 0 (auto) or 2..%d rows", kGroupWide, 6},
    {SFL_OPT_FUSE_PROJECTION, &Options::fuse_projection, kBool, 0, 1, nullptr, kGroupWide, 9},
    {SFL_OPT_ADVECT_KERNEL, &Options::advect_kernel, kRange, 0, 2, "advection kernel must be 0, 1 or 2", kGroupWide | kHostReset, 10},
    {SFL_OPT_FUSE_DIVERGENCE, &Options::fuse_divergence, kBool, 0, 1, nullptr, kGroupWide, 11},
    {SFL_OPT_SMALL_GRID, &Options::small_grid, kBool, 0, 1, nullptr, kGroupWide, 12},
    // (every set: what an exchange costs is measured again before the next solve)
    {SFL_OPT_EMULATE_WIRE_US, &Options::emulate_wire_us, kRange, 0, 10000, "emulated wire delay must be 0..10000 us", kForgetOnSet, 0},
    {SFL_OPT_STEP_SEAMS, &Options::step_seams, kBool, 0, 1, nullptr, 0, 0},
    {SFL_OPT_LAST_EARLY_ROWS, nullptr, kReadOnly, 0, 0, "this option is read-only", 0, 0},
    {SFL_OPT_HALO_TIMEOUT_MS, &Options::halo_timeout_ms, kRange, 0, INT_MAX, "halo timeout must be >= 0 ms (0 = the transport's default)", kGroupWide, 0},
    // one number over the two stored halves: set, get, the group's copy and the option block (words 7 and 13) name them by hand
    {SFL_OPT_EXCHANGE_SCHEDULE, nullptr, kRange, 0, 3, "exchange schedule must be 0 (auto), 1 (in line), 2 (behind events) or 3 (in time)", kGroupWide, 0},
    {SFL_OPT_MEASURED_WIRE_US, nullptr, kReadOnly, 0, 0, "this option is read-only", 0, 0},
    {SFL_OPT_LAST_HALO, nullptr, kReadOnly, 0, 0, "this option is read-only", 0, 0},
    {SFL_OPT_SOR_FOLD, &Options::sor_fold, kBool, 0, 1, nullptr, kGroupWide | kHostReset, 14},
};

}  // namespace host
}  // namespace sfl

namespace sfl {
namespace host {

// A set of tracers (tracers.cpp; include/sfl.h "tracers"): what a context or a batch holds of it.  Plain data, so that the
// two destroy paths free it and the step calls admit a trail's slots without a symbol of tracers.cpp -- the units that
// step are linked without it by the host test harnesses; what launches is reached through the `tracers_follow` pointer
// of the two structs, which tracers.cpp sets while a following set is attached (null: the step calls do what they did).
struct TracerSet {
    float *d_xy = nullptr;     // positions on the device: `count` float2 (a batch: of every member, member-major)
    size_t count = 0;          // tracers of the context, or of ONE member of the batch; 0: no set
    bool follow = false;
    // the trail: after every `every`-th advance the positions also go to the next of `capacity` slots of d_trail
    bool trail_on = false;
    int every = 0, capacity = 0, written = 0;
    int64_t advances = 0;      // counted since trail_start
    float *d_trail = nullptr;
};

// SFL_ERR_STATE if the `advances` advances of a call would complete more slots than the trail has free: the rule of
// record_admit (batch_state.h) -- after the call's own argument checks, before anything is staged or launched
inline int trail_admit(const TracerSet &t, int64_t advances)
{
    if (!t.trail_on) return SFL_OK;
    const int64_t due = (t.advances + advances) / t.every - t.advances / t.every, room = t.capacity - t.written;
    if (due > room)
        return fail(SFL_ERR_STATE, "the trail has room for %lld more slots (%d of %d written) and %lld advances would complete %lld: "
                    "nothing stepped or advanced; read the trail and start it again to make room",
                    (long long)room, t.written, t.capacity, (long long)advances, (long long)due);
    return SFL_OK;
}
// ... of the steps of a step call: a set that does not follow is not advanced by them
inline int trail_admit_steps(const TracerSet &t, int n) { return t.follow && t.count ? trail_admit(t, n) : SFL_OK; }

// A history (history.cpp; include/sfl.h "HISTORIES"): what a context or a batch holds of it.  Plain data, as TracerSet and
// for the same reason: the destroy paths free the records and the step calls admit and count without a symbol of
// history.cpp; the sample is launched through the `history_step` pointer of the two structs, which history.cpp sets
// while a history is on (null: the step calls launch what they launched before there were histories).
struct History {
    bool on = false;
    int every = 0, first = 0, count = 0, capacity = 0, written = 0;   // members [first, first + count) (a context: [0, 1))
    int64_t steps = 0;            // counted since history_start
    void *d_records = nullptr;    // `capacity` samples of `count` records of 64 bytes, sample-major; kept by a restart that
    size_t d_bytes = 0;           //   does not need more, freed by history_stop and the destroy paths
    // a context's sample is written by the streaming passes, which know nothing of the step: what the host knows of
    // sample s waits here and is merged into the bytes read out
    struct HostWords {
        int32_t iterations;
        int64_t step;
        float dt, dx;
    };
    std::vector<HostWords> host_words;
};

// SFL_ERR_STATE if the n steps of a call would complete more samples than are free: the rule of record_admit
// (batch_state.h) -- after the call's own argument checks, before anything is staged or launched
inline int history_admit(const History &h, int64_t n)
{
    if (!h.on) return SFL_OK;
    const int64_t due = (h.steps + n) / h.every - h.steps / h.every, room = h.capacity - h.written;
    if (due > room)
        return fail(SFL_ERR_STATE, "the history has room for %lld more samples (%d of %d written) and %lld steps would complete %lld: "
                    "nothing stepped; read the samples (sfl_history_read, sfl_batch_history_read) and start the history again to make room",
                    (long long)room, h.written, h.capacity, (long long)n, (long long)due);
    return SFL_OK;
}
// how many of the next n steps may run in one launch before a sample is due (n without a history): record_run's rule
inline int history_run(const History &h, int n) { return h.on ? (int)std::min<int64_t>(n, h.every - h.steps % h.every) : n; }

// The recorder of one record per solid body (body_recorder.h), as the loads, the friction and the torque each hold one,
// independent of each other.  Plain data, as History and for the same reason: the destroy paths free the records and the
// step calls admit without a symbol of loads.cpp, friction.cpp or torque.cpp; the sample is launched through the `loads_step`,
// `friction_step` and `torque_step` pointers of the two structs, which those units set while their recorder is on (null: the
// step calls launch what they launched before there was such a recorder).
struct Recorder {
    bool on = false;
    int every = 0, first = 0, count = 0, capacity = 0, written = 0;   // members [first, first + count) (a context: [0, 1))
    int64_t steps = 0;            // counted since the recorder's start
    // the records (48 bytes; the torque's 64): in front those of ONE sample of every member (what the synchronous call
    // writes and copies out), behind them `capacity` samples of count * bodies, sample-major.  Kept by a restart that does
    void *d_records = nullptr;    //   not need more, freed by the recorder's stop and the destroy paths
    size_t d_bytes = 0;
};

// SFL_ERR_STATE if the n steps of a call would complete more samples than are free: history_admit's rule.  noun: "loads",
// read_calls: "sfl_loads_read, sfl_batch_loads_read"
inline int recorder_admit(const Recorder &r, int64_t n, const char *noun, const char *read_calls)
{
    if (!r.on) return SFL_OK;
    const int64_t due = (r.steps + n) / r.every - r.steps / r.every, room = r.capacity - r.written;
    if (due > room)
        return fail(SFL_ERR_STATE, "the %s recorder has room for %lld more samples (%d of %d written) and %lld steps would complete %lld: "
                    "nothing stepped; read the samples (%s) and start the recorder again to make room",
                    noun, (long long)room, r.written, r.capacity, (long long)n, (long long)due, read_calls);
    return SFL_OK;
}

// Loads (loads.cpp; include/sfl.h "LOADS"): the loads recorder and the bodies' labels, which every kind reads.
struct Loads : Recorder {
    uint8_t *d_labels = nullptr;   // one label byte per cell (a batch: of every member when per_member); null: every solid is body 1
    size_t d_label_bytes = 0;
    bool per_member = false;
    int bodies = 1;
};
inline int loads_admit(const Loads &l, int64_t n) { return recorder_admit(l, n, "loads", "sfl_loads_read, sfl_batch_loads_read"); }

// Friction (friction.cpp; include/sfl.h "FRICTION"): the recorder alone; the labels and `bodies` are Loads'.
struct Friction : Recorder {};
inline int friction_admit(const Friction &f, int64_t n) { return recorder_admit(f, n, "friction", "sfl_friction_read, sfl_batch_friction_read"); }

// Torque (torque.cpp; include/sfl.h "TORQUE"): the recorder and the pivots of the bodies; the labels and `bodies` are Loads'.
// The pivots live twice: on the host, for the records that need no launch (no solids set) and for the download, and in a
// small device table that the samplers read.
struct Torque : Recorder {
    // (x2, y2) per body, of every member when pivots_per_member; null / empty: every pivot is (0, 0)
    int32_t *d_pivot2 = nullptr;  //   freed by set_body_pivots(NULL), by a set_bodies that changes `bodies` and by the destroy paths
    size_t d_pivot_bytes = 0;
    bool pivots_per_member = false;
    std::vector<int32_t> h_pivot2;
};
inline int torque_admit(const Torque &t, int64_t n) { return recorder_admit(t, n, "torque", "sfl_torque_read, sfl_batch_torque_read"); }

// Averages (means.cpp; include/sfl.h "AVERAGES"): the per-cell sums over time that a context or a batch holds.  Plain data,
// as History and for the same reason: the destroy paths free the planes and batch.cpp finds the cut points of a replay
// (mean_run) without a symbol of means.cpp; the sample is launched through the `mean_step` pointer of the two structs, which
// means.cpp sets while averages are on with every >= 1 (null: the step calls launch what they launched before there were
// averages).  There is no capacity and so no admission.
struct Means {
    bool on = false;
    unsigned what = 0;            // the mask of SFL_MEAN_* groups whose planes exist
    int every = 0, first = 0, count = 0;   // members [first, first + count) (a context: [0, 1)); every == 0: manual samples only
    int64_t steps = 0, samples = 0;        // counted since mean_start
    // the live planes, in the order of their ids, each `count` members of `member_stride` values of 8 bytes (the cells of a
    // member rounded up to an even number: every member's plane starts on 16 bytes); freed by mean_stop and the destroy paths
    void *d_planes = nullptr;
    size_t member_stride = 0, d_bytes = 0;
};
// how many of the next n steps may run in one launch before a sample is due (n with no averages behind the steps): history_run's rule
inline int mean_run(const Means &m, int n) { return m.on && m.every > 0 ? (int)std::min<int64_t>(n, m.every - m.steps % m.every) : n; }

// What the view calls (views.cpp; include/sfl.h "VIEWS") keep on the device for a context or a batch: the staged palette
// of the call (kViewPaletteWords words, allocated at the first call) and the call's result, which only grows.  Plain
// data, freed by the two destroy paths, so that they need no symbol of views.cpp.
struct ViewScratch {
    uint32_t *d_palette = nullptr;
    void *d_out = nullptr;
    size_t out_bytes = 0;
};

// Solid cells of a whole-domain context (context_solids.cpp; include/sfl.h "SOLIDS OF A CONTEXT"): what the context holds
// of them.  Plain data, as TracerSet and History and for the same reason: sfl_destroy frees the code bytes, and the
// calls that honour solids live in units that the host test harnesses link without context_solids.cpp -- they reach
// the masked launches through these pointers, set there while a mask is set and null otherwise (then every call
// launches exactly what it launched before there were solids).
struct ContextSolids {
    bool set = false;
    uint8_t *d_codes = nullptr;   // one code byte per cell (solids.cpp solid_codes), dim_x * gdim_y of them
    size_t d_bytes = 0;
    int64_t solid_cells = 0;      // of the mask that is set (sfl_solids_info)
    // one step by the rule, behind sfl_step's checks: the unfused sequence (no seams, no small-grid step)
    int (*step)(sfl_context *c, float dt, float dx, int iters, float omega) = nullptr;
    int (*divergence)(sfl_context *c, float dx) = nullptr;
    // warm: `iters` more iterations on the pressure held instead of a solve from zero
    int (*solve)(sfl_context *c, float dx, int iters, float omega, bool warm) = nullptr;
    int (*gradient)(sfl_context *c, float dx) = nullptr;
    // the masked update norm / max |divergence| of the fields held, as bits into a device word (launches only; the word
    // is zeroed on the stream in front)
    int (*norm)(sfl_context *c, float dx, unsigned *d_word) = nullptr;
    int (*max_div)(sfl_context *c, float two_dx_inv, unsigned *d_word) = nullptr;
    // put the six pointers above back to what the mask alone makes them (context_openings.cpp, when its map is cleared)
    void (*rehook)(sfl_context *c) = nullptr;
};

// Openings of a whole-domain context (context_openings.cpp; include/sfl.h "OPENINGS OF A CONTEXT"): what the context holds of
// them.  Plain data, as ContextSolids and for the same reason; sfl_destroy frees the device arrays.  While `set`,
// context_openings.cpp puts its own functions into the six pointers of ContextSolids -- the step, the operators, the solves,
// the update norm, the statistics and the history's sample reach the openings' kernels through the pointers they already
// call, and ContextSolids::set and ::d_codes stay what the solids made them -- and sfl_set_solids calls `restage` behind a
// change of the mask, which forms the bytes again and puts the pointers back.
struct ContextOpenings {
    bool set = false;
    std::vector<uint8_t> map;          // dim_x * gdim_y bytes as given
    float inflow[2] = {0.0f, 0.0f};
    uint8_t *d_codes = nullptr;        // a copy of the solids' code bytes, or those of an all-fluid grid
    uint8_t *d_open = nullptr;         // the open byte of every cell (sor_open_tile.h)
    uint32_t *d_inflow_cells = nullptr;   // the fluid inflow cells, a compact list
    int64_t inflow_cells = 0, outflow_cells = 0;   // live ones
    int (*restage)(sfl_context *c) = nullptr;
    // the inflow profile and the flux (include/sfl.h "INFLOW PROFILES AND FLUX"): the compact list on the host, the records as
    // given (duplicates removed, in cell order; profile_on: a profile is held), and beside the list on the device one (u, v)
    // per list entry -- the record's velocity where the profile has one, the uniform inflow elsewhere --, formed again when
    // the profile, the inflow or the mask changes; the one flux record.  Freed where the list is.
    struct ProfileRecord {
        uint32_t cell;
        float u, v;
    };
    std::vector<uint32_t> list;
    bool profile_on = false;
    std::vector<ProfileRecord> profile;
    float *d_inflow_values = nullptr;
    void *d_flux = nullptr;
};

// Viscosity of a whole-domain context (context_viscous.cpp; include/sfl.h "VISCOSITY"): what the context holds of it.  Plain
// data, as ContextSolids and for the same reason: sfl_destroy frees the third buffer, and the step and the transports
// live in units that the host test harnesses link without context_viscous.cpp -- the step reaches the unfused sequence
// through `step`, set there while a viscosity is set and null otherwise (then every call launches exactly what it
// launched before there was viscosity).
struct ContextViscosity {
    bool set = false;
    float nu = 0.0f;
    int sweeps = 0;
    float *d_third = nullptr;   // a third velocity-sized buffer: u0 survives the launches of more than kD sweeps in it; allocated at the first such call
    // one step with item 3a, behind sfl_step's checks: the unfused sequence (no seams, no fused kernels, no small-grid step)
    int (*step)(sfl_context *c, float dt, float dx, int iters, float omega) = nullptr;
};

// Wall velocities of a whole-domain context (context_walls.cpp; include/sfl.h "WALL VELOCITIES"): the records as given,
// duplicates removed and in cell order (wall_table.h), and the same as a compact list on the device -- `records` cell
// indices, behind them one (u, v) each, in ONE allocation that sfl_destroy frees.  Plain data, as ContextSolids and for
// the same reason: while a table is held the step reaches the sequence with the walls' launches through `step`, in front
// of the viscosity's and the solids', and every successful sfl_set_solids calls `drop` (the stream is idle there), which
// frees the list and clears both.  Null, every call launches exactly what it launched before there were walls.
struct ContextWalls {
    bool on = false;
    std::vector<sfl::walls::Record> row;
    void *d_list = nullptr;
    size_t d_bytes = 0;
    const uint32_t *d_cells = nullptr;
    const float *d_vel = nullptr;
    int (*step)(sfl_context *c, float dt, float dx, int iters, float omega) = nullptr;
    void (*drop)(sfl_context *c) = nullptr;
};

}  // namespace host
}  // namespace sfl

struct sfl_context {
    int device = 0;
    int dim_x = 0, gdim_y = 0;
    int rank = 0, nranks = 1;
    int g0 = 0, g1 = 0;  // owned global rows
    int ghost = 0;       // ghost rows per side
    sfl::Slab geom{};
    hipStream_t stream = nullptr;
    bool owns_stream = true;
    hipEvent_t ev_start = nullptr, ev_stop = nullptr;
    // halo exchanges of a solve run on their own stream so that they overlap the launches that do
    // not depend on them (a slab with a transport of its own; a linked group keeps these in Group).  Created when the
    // transport is attached, not at the first solve; whether it really runs beside `stream` -- the runtime folds its streams
    // onto a few hardware queues, and a launch that waits for a message inside the kernel must not share a queue with the
    // stream that carries the message -- is MEASURED (transport.cpp streams_run_concurrently), never assumed.
    hipStream_t xstream = nullptr;
    hipEvent_t ev_ready = nullptr, ev_arrived = nullptr;

    // fields: local arrays of geom.lrows rows (allocated on first use)
    float *vel = nullptr, *vel_tmp = nullptr;
    uint32_t *col = nullptr, *col_tmp = nullptr;
    // div, p and p_alt are three thirds of ONE allocation (sor_block)
    float *sor_block = nullptr;
    float *div = nullptr;
    float *p = nullptr, *p_alt = nullptr;  // p = current pressure, p_alt = ping-pong partner
    int *halo_flag = nullptr;      // device words: [0] a back-trace left a fixed advection halo
    int *d_arrival = nullptr;      // [1] halo messages arrived (and relaxed) so far: what cut-adjacent tiles poll inside a
                                   //     launch (kernels.h HaloWait); [2] such a wait timed out
    int arrival_epoch = 0;         // the last value queued for [1]
    int *d_collective = nullptr;   // [4 .. 4 + kCollectiveWords) scratch of the ranks' small reductions (measure_exchange, the halo tuner): allocated
                                   //     with the context, so that no rank can drop out of a collective over a failed allocation
    int *d_done = nullptr;         // [3] sender tiles finished so far (kernels.h HaloWait::done): what the exchange stream waits
    int done_target = 0;           //     for before a halo message leaves; done_target = the count the launches queued so far reach
    unsigned *d_norm = nullptr;    // [4 + kCollectiveWords, + kNormWords) what a norm launch or the small-grid until kernel leaves: the bits
                                   //     of an update norm, then an iteration count (sfl_residual, sfl_poisson_solve_until)
    unsigned *h_norm = nullptr;    // ... and their pinned host copy: allocated with the context, nothing is allocated per call
    struct sfl_flow_stats *d_stats = nullptr, *h_stats = nullptr;   // sfl_flow_stats: the device record the two passes leave and its pinned host
                                   //     copy, allocated at the first call (flow_stats.cpp), nothing per call
    struct sfl_field_distance *d_dist = nullptr, *h_dist = nullptr;   // sfl_distance with this context as `a`: the same pair (ensemble.cpp)
    bool wait_error_seen = false;  // word [2] was found raised (download, a step's report): every call fails until sfl_synchronize
                                   // has reported and cleared it

    // queued point forces (ino:264-269): the records of step 0 of the timeline (include/sfl.h, "the timeline rule"), in
    // queue order; those of the steps behind it wait in force_later under their ABSOLUTE step number, force_base being
    // the number of step 0 (forces_advance: one step has run)
    std::vector<int> force_cells;
    std::vector<float> force_vel;
    struct StepForces {
        std::vector<int> cells;
        std::vector<float> vel;
    };
    std::map<int64_t, StepForces> force_later;
    int64_t force_base = 0;
    int *d_force_cells = nullptr;
    float *d_force_vel = nullptr;
    int d_force_cap = 0;
    // pinned staging of the queued forces, two slots used alternately: the copy of step k may
    // still be in flight while step k + 1 is being queued, never the one of step k - 1 (each
    // slot's last copy is fenced by its event before the slot is rewritten)
    struct ForceStage {
        int *cells = nullptr;
        float *vel = nullptr;
        int cap = 0;
        hipEvent_t copied = nullptr;
        bool pending = false;
    } force_stage[2];
    int force_slot = 0;

    // dye visualiser: device image + pinned host staging, kept between frames
    uint16_t *d_image = nullptr;
    size_t d_image_bytes = 0;

    // scratch field of sfl_host_advect_vec2f when the advected field is not the velocity
    float *host_scratch = nullptr;

    // automatic advection halo (SFL_OPT_ADVECT_HALO = 0): device scratch of the back-trace reach
    // {below, above}, and the whole advected field gathered on this GPU when the reach outruns the
    // ghost rows (allocated on first need; sized for the 12-byte dye element)
    int *d_reach = nullptr;
    void *gather_buf = nullptr;
    // ... without a host round trip inside sfl_step (slab_step_auto): the dye advection runs on a GUESSED halo,
    // the true reach of its back-traces and an "a back-trace left the halo" flag are reduced on the device,
    // land in pinned host memory behind ev_report, and are examined when the NEXT call touches the context
    int *d_report = nullptr;       // device reach words (launch_reach_set) with the flag in word [2]
    int *h_report = nullptr;       // pinned host copy (kReportWords)
    bool report_zeroed = false;    // d_report has been zeroed behind its copy to the host (post_reach_report)
    bool reach_in_report = false;  // the dye's kernel of this step has left the reach words in d_report already
    // slab_step_auto: the rows further than `early_rows` from both cuts were advected into vel_tmp BEFORE the host waited for the
    // last step's report (advect_interior_early); valid for the velocity of vel_epoch == early_epoch at early_dt
    int early_rows = 0;
    uint64_t early_epoch = 0;
    float early_dt = 0.0f;
    bool disp_in_report = false;   // the pending report carries word [3] (the tile kernel measured it)
    int last_early_kept = 0;       // slab_step_auto: rows from each cut beyond which the last step kept the early advection (0: none)
    int known_disp = -1;           // rows a cell's sources lie from its own row at most, for the velocity of known_epoch (-1: unknown)
    hipEvent_t ev_report = nullptr;
    hipEvent_t ev_color_halo = nullptr;  // the dye's halo, sent at the START of a step (slab_step_auto), has arrived
    hipEvent_t ev_vel_final = nullptr;   // recorded in front of the early interior advection (advect_interior_early)
    bool vel_final_recorded = false;     // ... in the step that is being queued
    bool color_unsettled = false;  // a dye advection on a guessed halo has not been checked yet
    float unsettled_dt = 0.0f;
    int known_reach = -1;          // reach of the back-traces of the CURRENT velocity at known_dt (-1: unknown)
    int known_reach_ext = -1;      // ... when own +- 1 rows are advected (reach_extended)
    uint64_t known_epoch = 0, vel_epoch = 1;   // vel_epoch counts the writes to the velocity field
    float known_dt = 0.0f;

    // tracers (tracers.cpp): the set, and the advance behind every step while it follows (one step has run, its
    // projected velocity is stored: launch the advance by dt on the context's stream)
    sfl::host::TracerSet tracers;
    int (*tracers_follow)(sfl_context *c, float dt) = nullptr;
    sfl::host::ViewScratch views;   // sfl_view_* (views.cpp)
    // the history (history.cpp), and its sample behind every step while it is on (one step has run and been counted by
    // nobody yet: count it and, when a sample is due, launch the statistics' passes on the context's stream)
    sfl::host::History history;
    int (*history_step)(sfl_context *c, float dt, float dx, int iters) = nullptr;
    sfl::host::ContextSolids solids;   // solid cells (context_solids.cpp)
    // loads (loads.cpp), and the recorder's sample behind every step while it is on (one step has run: count it and, when a
    // sample is due, launch it on the context's stream); called last, behind history_step
    sfl::host::Loads loads;
    int (*loads_step)(sfl_context *c) = nullptr;
    // the friction recorder (friction.cpp), by the same rule; called last, behind loads_step
    sfl::host::Friction friction;
    int (*friction_step)(sfl_context *c) = nullptr;
    // the pivots and the torque recorder (torque.cpp), by the same rule; called behind friction_step
    sfl::host::Torque torque;
    int (*torque_step)(sfl_context *c) = nullptr;
    // the averages (means.cpp), and their sample behind every step while they are on with every >= 1 (one step has run: count
    // it and, when a sample is due, launch it on the context's stream); called last, behind friction_step
    sfl::host::Means means;
    int (*mean_step)(sfl_context *c) = nullptr;
    sfl::host::ContextViscosity viscosity;  // item 3a of a step (context_viscous.cpp)
    sfl::host::ContextOpenings openings;     // inflow and outflow cells on the rim (context_openings.cpp)
    sfl::host::ContextWalls walls;           // solid cells that hold a velocity (context_walls.cpp)

    sfl::host::Options opt;  // what sfl_set_option stores (kOptions above: one row per option)

    // how halo rows reach the neighbouring slabs (transport.h); null on a whole-domain context and on a slab that has
    // not been attached / linked yet.  `group` = the same object when it is an in-process group of virtual ranks.
    std::shared_ptr<sfl::host::Transport> transport;
    sfl::host::Group *group = nullptr;
    std::shared_ptr<sfl::host::Transport> keepalive;   // a dissolved group's streams, while this context still runs on them
    bool options_dirty = false;         // an option changed since the ranks last compared their option blocks
    int streams_concurrent = -1;        // compute and exchange stream were seen to run side by side: 1, seen not to: 0, untested: -1
    // One halo exchange of this slab's transport, measured at attach / before the first solve (transport.cpp
    // measure_exchange): microseconds of a message of ~0 rows (latency: launch, protocol, wire) and nanoseconds per further
    // row of p (bandwidth).  Maximum over the ranks: every rank derives the same halo depth from it.  -1: not measured.
    int exchange_latency_us = -1, exchange_ns_per_row = 0;
    int last_halo = 0;                  // halo depth of the last solve's plan (SFL_OPT_LAST_HALO)
    sfl::host::HaloTuner halo_tuner;    // (a linked group keeps its own: Group::halo_tuner)

    int last_launches = 0, last_exchanges = 0, last_fuse = 0;
    int solve_tail = 0;   // ghost rows of p the next solve must leave exact (slab_step_auto: 1, for subtract_gradient)
    int p_ghost_valid = 0;  // ghost rows of p that are exact right now (set by the solve, cleared by whoever writes p)
    int v_ghost_valid = 0;  // ghost rows of the velocity that are exact right now (slab_step_auto advects own +- 1 rows)

    size_t local_cells() const { return (size_t)geom.lrows * dim_x; }
    size_t owned_offset_cells() const { return (size_t)ghost * dim_x; }
};

namespace sfl {
namespace host {

size_t field_elem_bytes(int field);
int use_device(sfl_context *c);
int ensure_bytes(sfl_context *c, void **ptr, size_t elem_bytes, bool zero);
template <class T>
int ensure(sfl_context *c, T *&ptr, size_t elem_bytes, bool zero)
{
    if (ptr) return SFL_OK;
    void *m = nullptr;
    SFL_TRY(ensure_bytes(c, &m, elem_bytes, zero));
    ptr = static_cast<T *>(m);
    return SFL_OK;
}
int ensure_field(sfl_context *c, int field);
void *field_ptr(sfl_context *c, int field);
// the contexts whose programs one host thread issues together: the members of a linked group, else the context itself
std::vector<sfl_context *> peers_of(sfl_context *c);
int min_owned_rows(const sfl_context *c);
inline int clip_lo(const sfl_context *, int g) { return g < 0 ? 0 : g; }
inline int clip_hi(const sfl_context *c, int g) { return g > c->gdim_y ? c->gdim_y : g; }
int upload_raw(sfl_context *c, void *dev, const void *host, size_t elem_bytes);
int download_raw(sfl_context *c, const void *dev, void *host, size_t elem_bytes);
// fails (SFL_ERR_HIP) when a wait inside one of the context's solves is known to have given up: p is not valid
int check_wait_error(sfl_context *c);

// ---- sor_executor.cpp ----
// warm: `iters` MORE iterations on the pressure the context holds instead of a solve from zero (whole-domain contexts
// on the general kernels)
int run_poisson(sfl_context *ctx, float dx, int iters, float omega, bool warm = false);
SorParams sor_params(const sfl_context *c, float dx, float omega);
// one workgroup, fields in LDS (small_grid.hip): may this context take that path?
bool small_grid(const sfl_context *c);
// halo timeout of the waits inside this context's launches, microseconds (kernels.h HaloWait::timeout_us)
int halo_timeout_us(const sfl_context *c);
// will the next solve count its halo exchanges on the device (SFL_OPT_EXCHANGE_SCHEDULE resolved; the streams' verdict is in)?
bool in_time_exchanges(const sfl_context *c);
// halo depth of a solve's supersteps: the option, or chosen from the measured exchange (sor_executor.cpp)
int effective_halo(const sfl_context *c, int fuse, int iters, bool in_time);

// ---- operators.cpp ----
struct AdvectPlan {
    int halo = 0;         // rows to exchange per side (fixed or measured)
    bool gather = false;  // sample a gathered copy of the whole field instead
    bool flag = true;     // fixed halo: let the kernel report a back-trace that leaves it
    bool report = false;  // ... into the context's reach report (a guessed halo, checked by settle_color)
                          // instead of the error flag sfl_synchronize turns into SFL_ERR_HALO
    bool halo_sent = false;  // the halo rows are already on their way (behind ev_color_halo): wait, do not exchange
};
int launch_reach_set(sfl_context *c, int *words, float dt);
inline int reach_own(const int *w) { return std::max(w[0], w[1]); }
inline int reach_extended(const int *w) { return std::max(reach_own(w), 1 + std::max(w[5], w[6])); }
int measure_reach(sfl_context *ctx, const std::vector<sfl_context *> &peers, float dt, int *reach_out,
                  int *reach_ext_out = nullptr);
int advect_velocity_planned(sfl_context *ctx, const std::vector<sfl_context *> &peers, float dt, int no_slip,
                            const AdvectPlan &plan, int extend = 0, int interior_done = 0);
int advect_color_planned(sfl_context *ctx, const std::vector<sfl_context *> &peers, float dt, int no_slip,
                         const AdvectPlan &plan);
int apply_queued_forces(sfl_context *c);
// one step of the context (and of its in-process peers) has run: what is left of step 0 goes, step 1 becomes step 0
void forces_advance(sfl_context *ctx);
int stage_queued_forces(sfl_context *c, int *count);
int project_and_advect_color(sfl_context *ctx, float dt, float dx, int halo, bool report, bool halo_sent = false);
bool can_fuse_divergence(const sfl_context *c);
int advect_velocity_and_divergence(sfl_context *c, float dt, float dx);

// ---- slab_step.cpp ----
// Examine the report of the last dye advection that ran on a guessed halo; repeat it when the guess was short.  Cheap
// when nothing is pending.  Every entry point that reads or writes the fields calls it.  `collective` = the caller is an
// operator every rank of a communicator issues (a solve, a step, an advection): only those may compare option blocks.
int settle_color(sfl_context *ctx, bool collective = false);

}  // namespace host
}  // namespace sfl
