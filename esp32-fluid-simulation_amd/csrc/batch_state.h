// batch_state.h -- what a batch of the C ABI holds (include/sfl.h group 4), shared by the two host units of the batches:
// batch.cpp (creation, field I/O, the step and solve calls) and batch_frames.cpp (the frames of many members in one
// launch, and the recorder that renders them between the step launches).  Host C++ only.
#pragma once
#include "batch.h"
#include "context.h"
#include "stats_kernels.h"
#include "view_kernels.h"

struct sfl_batch {
    int device = 0;
    int dim_x = 0, dim_y = 0, batch = 0;
    size_t cells = 0;   // per member
    bool large = false;   // made by sfl_batch_create_large: every launch is one of batch_large.hip, whatever the shape
    hipStream_t stream = nullptr;
    // fields, member-major; velocity and dye ping-pong between two buffers (ino:255, :286)
    float *vel = nullptr, *vel_tmp = nullptr;
    uint32_t *col = nullptr, *col_tmp = nullptr;
    float *div = nullptr, *p = nullptr;
    // the timeline of queued point forces (ino:264-269; include/sfl.h, "the timeline rule"), in queue order.  A record
    // carries the ABSOLUTE number of its step; force_base is the number of step 0, the next step any step call runs
    struct Force {
        int64_t step;
        int member, i, j;
        float vx, vy;
    };
    std::vector<Force> forces;
    int64_t force_base = 0;
    int64_t force_last = -1;   // the largest absolute step any record carries; < force_base: the timeline is empty
    // the staged timeline: ONE CSR table on the device, filled from pinned memory (two host slots used alternately, each
    // rewritten only after its last copy has completed).  Row r, r in [0, staged_rows), belongs to step staged_base + r
    // and is the BatchStep::force_offsets of that step: the `batch` + 1 ints at r * batch.  staged_rows * batch + 1
    // ints, then the cells of the staged_records records sorted by (step, member, queue order), then their velocities.
    // Staged once per change of the timeline (forces_staged), not once per step; staged_row_has[r]: row r has a record.
    void *d_forces = nullptr;
    size_t d_forces_bytes = 0;
    bool forces_staged = false;
    int64_t staged_base = 0;
    int staged_rows = 0;
    size_t staged_records = 0;
    std::vector<char> staged_row_has;
    struct Stage {
        void *host = nullptr;
        size_t bytes = 0;
        hipEvent_t copied = nullptr;
        bool pending = false;
    } stage[2];
    int slot = 0;
    // per-member parameters (sfl_batch_*_each): `batch` device records, filled from pinned memory by the same two-slot rule,
    // and one float per member for the update norm the *_each kernels leave (valid: see sfl_batch_residual)
    sfl::BatchMember *d_members = nullptr;
    Stage member_stage[2];
    int member_slot = 0;
    float *d_report = nullptr;
    bool report_valid = false;
    // stopping rules (sfl_batch_*_until): the members' sfl_member_stop behind their records, in the same device array and
    // in launch order, and two ints per member for the iterations the *_until kernels ran (valid: see sfl_batch_iterations)
    sfl::BatchStop *d_stops = nullptr;
    int *d_counts = nullptr;
    bool counts_valid = false;
    // flow statistics (sfl_batch_flow_stats[_each]): one record per member that the two passes leave, behind them one
    // 1 / (2 dx) per member; the same in pinned memory.  Allocated at the first call, nothing per call
    sfl::FlowStatsRecord *d_stats = nullptr, *h_stats = nullptr;
    // sfl_batch_distance (ensemble.cpp): one record per member on the device and in pinned memory, allocated at the first call
    struct sfl_field_distance *d_dist = nullptr, *h_dist = nullptr;
    // sfl_batch_envelope (ensemble.cpp): ONE allocation made at the first call -- the four fields of the snapshot (mean, min,
    // max, spread: 3 * cells words each), behind them the partial results of the member groups (ensemble_kernels.h) --
    // and the range [env_first, env_first + env_count) the snapshot holds (env_count == 0: none yet)
    uint32_t *d_env = nullptr;
    int env_first = 0, env_count = 0;
    // dye visualiser's device image, kept between frames
    uint16_t *d_image = nullptr;
    size_t d_image_bytes = 0;
    // ... and the images of sfl_batch_render_members: as many members as the largest call so far rendered
    uint16_t *d_images = nullptr;
    size_t d_images_bytes = 0;
    // the recorder (sfl_batch_record_*): `capacity` frames of members [first, first + count) at one scaling, frame f at
    // pixel f * count * H * W of d_frames; `written` of them are rendered, `steps` steps counted since record_start
    struct Recorder {
        bool on = false;
        int every = 0, first = 0, count = 0, scaling = 0, byteswap = 0, capacity = 0, written = 0;
        int64_t steps = 0;
        // what the frames show (sfl_batch_record_view): the dye, or this view, its palette in the batch's d_rec_palette
        bool view_on = false;
        sfl::ViewParams view{};
    } rec;
    uint16_t *d_frames = nullptr;   // kept by a restart that does not need more; freed by record_stop
    size_t d_frames_bytes = 0;
    // tracers (tracers.cpp; context.h has TracerSet): `count` per member, positions [member][k][2], a trail slot the
    // positions of every member.  tracers_follow: one step has been launched and the ping-pong swapped -- launch the
    // advance on the batch's stream behind it, member by member by the dt of its record (members: the device records
    // of the step's launch, in its launch order) or all by `dt` (members == nullptr)
    sfl::host::TracerSet tracers;
    int (*tracers_follow)(sfl_batch *b, const sfl::BatchMember *members, float dt) = nullptr;
    // the history (history.cpp; context.h has History): history_step: `steps` steps have been launched (one launch) and the
    // ping-pong swapped -- count them and, when a sample is due, launch it on the batch's stream behind them.  members: the
    // device records of the launch, in its launch order (nullptr: every member ran `step`'s dt, dx and iters); until: the
    // launch left each member's iterations in d_counts
    sfl::host::History history;
    int (*history_step)(sfl_batch *b, int steps, const sfl::BatchMember *members, bool until, const sfl::SmallStep &step) = nullptr;
    // views (views.cpp): the scratch of the view calls; the recorder's staged palette (allocated by the first
    // sfl_batch_record_view, kept until the batch goes) and the host copy its upload reads; record_view_frame: a frame of
    // the recorder's view (rec.view) is due -- launch its render into `images` on the batch's stream.  Set by
    // sfl_batch_record_view: batch_frames.cpp, which the host test harnesses link without views.cpp, calls through it
    sfl::host::ViewScratch views;
    uint32_t *d_rec_palette = nullptr;
    std::vector<uint32_t> rec_palette_host;
    int (*record_view_frame)(sfl_batch *b, uint16_t *images) = nullptr;
    // solid cells (solids.cpp; include/sfl.h "SOLIDS"): the code bytes on the device (batch.h BatchSolids: `batch` x cells of
    // them, or cells for a mask all members share), freed by the destroy path.  Plain data, as the history is and for the
    // same reason; while `set`, the step, solve and statistics calls of batch.cpp launch through the three pointers, which
    // solids.cpp sets and clears with it -- cleared, those calls launch exactly what they launched before there were solids.
    struct Solids {
        bool set = false, per_member = false;
        uint8_t *d_codes = nullptr;
        size_t d_bytes = 0;
        // one step is due: launch it (each: by the records of d_members, and the update norm into d_report)
        int (*step)(sfl_batch *b, bool each, const sfl::BatchStep &a) = nullptr;
        // the solve of d into p (each: as above; else iters and prm)
        int (*solve)(sfl_batch *b, bool each, int iters, sfl::SorParams prm) = nullptr;
        // the velocity part of the flow statistics into d_stats, zeroed in front on the stream
        int (*stats)(sfl_batch *b, float two_dx_inv, const float *d_member_two_dx_inv) = nullptr;
    } solids;
    // loads (loads.cpp; context.h has Loads): loads_step: `steps` steps have been launched and the ping-pong swapped --
    // count them and launch (without solids: zero) the samples that are due on the batch's stream behind them; called
    // last, behind history_step
    sfl::host::Loads loads;
    int (*loads_step)(sfl_batch *b, int steps) = nullptr;
    // the friction recorder (friction.cpp; context.h has Friction), by the same rule; called last, behind loads_step
    sfl::host::Friction friction;
    int (*friction_step)(sfl_batch *b, int steps) = nullptr;
    // the pivots and the torque recorder (torque.cpp; context.h has Torque), by the same rule; called behind friction_step
    sfl::host::Torque torque;
    int (*torque_step)(sfl_batch *b, int steps) = nullptr;
    // the averages (means.cpp; context.h has Means): mean_step: `steps` steps have been launched (one launch: mean_run saw to
    // it that no sample falls inside them) and the ping-pong swapped -- count them and, when a sample is due, launch it on
    // the batch's stream behind them; called last, behind friction_step
    sfl::host::Means means;
    int (*mean_step)(sfl_batch *b, int steps) = nullptr;
    // viscosity (viscous.cpp; include/sfl.h "VISCOSITY"): nu of every member on the host, and one record per member on the
    // device (viscous_kernels.h BatchViscous: a, c, sweeps), indexed by the member, filled from pinned memory by the
    // two-slot rule of member_stage.  Plain data, as the solids are and for the same reason: the destroy path frees the
    // table and the slots; while `set`, the step calls of batch.cpp stage the table once per call through `stage`
    // (params: the _each call's records, else dt and dx for all) and launch every step through `step`, which picks the
    // kernel with or without solids itself.  viscous.cpp sets and clears both with `set`.
    struct Viscosity {
        bool set = false, per_member = false;
        int sweeps = 0;
        std::vector<float> nu;   // `batch` floats while set
        void *d_table = nullptr;
        Stage stage_slot[2];
        int slot = 0;
        int (*stage)(sfl_batch *b, float dt, float dx, const sfl_member_params *params) = nullptr;
        int (*step)(sfl_batch *b, bool each, const sfl::BatchStep &a) = nullptr;
    } viscosity;
    // openings (openings.cpp; include/sfl.h "OPENINGS"): the map and the inflow as given, on the host; the open codes
    // (batch.h BatchOpenings: the solids' code byte with the opening above it, `batch` x cells of them or cells where neither
    // the map nor the mask is per member) and `batch` inflow velocities on the device, freed by the destroy path.  Plain data,
    // as the solids are and for the same reason; while `set`, the step, solve and statistics calls of batch.cpp launch
    // through the three pointers in front of the solids', and sfl_batch_set_solids calls `restage` behind a change of the
    // mask, which forms the open codes again -- an opening counts only where the cell is fluid.  openings.cpp sets and
    // clears all four with `set`.
    struct Openings {
        bool set = false, per_member = false, codes_per_member = false, inflow_per_member = false;
        std::vector<uint8_t> map;     // cells bytes, or batch x cells (per_member)
        std::vector<float> inflow;    // (x, y) of every member
        uint16_t *d_codes = nullptr;
        size_t d_bytes = 0;
        float *d_inflow = nullptr;    // 2 x batch floats
        int64_t inflow_cells = 0, outflow_cells = 0;   // live ones, over all members
        int (*step)(sfl_batch *b, bool each, const sfl::BatchStep &a) = nullptr;
        int (*solve)(sfl_batch *b, bool each, int iters, sfl::SorParams prm) = nullptr;
        int (*stats)(sfl_batch *b, float two_dx_inv, const float *d_member_two_dx_inv) = nullptr;
        int (*restage)(sfl_batch *b) = nullptr;
        // the inflow profile and the flux (inflow.cpp; include/sfl.h "INFLOW PROFILES AND FLUX").  The records as given,
        // duplicates removed and in cell order: one row for all members (profile_shared) or one per member; profile_on: a
        // profile is held (it may hold no record).  ONE CSR table on the device (batch.h BatchProfile: `batch` + 1 offsets, the
        // cells, the velocities) that names only the cells that are fluid inflow cells at the time, and `batch` flux records;
        // both freed where the codes are.  While a profile is held the openings' step launches through profile_step, and the
        // staging of the codes (a new mask) forms the table again through profile_restage with the codes it has just made
        // (member stride as in BatchOpenings).  inflow.cpp sets both; a new map and a clearing drop them with the profile.
        struct ProfileRecord {
            uint32_t cell;
            float u, v;
        };
        bool profile_on = false, profile_shared = false;
        std::vector<std::vector<ProfileRecord>> profile;
        void *d_profile = nullptr;
        size_t d_profile_bytes = 0;
        sfl::BatchProfile profile_table{nullptr, nullptr, nullptr};
        void *d_flux = nullptr;
        int (*profile_step)(sfl_batch *b, bool each, const sfl::BatchStep &a) = nullptr;
        int (*profile_restage)(sfl_batch *b, const uint16_t *codes, size_t member_stride) = nullptr;
    } openings;
    // wall velocities (walls.cpp; include/sfl.h "WALL VELOCITIES"): the rows as given, duplicates removed and in cell order
    // (wall_table.h: one row for all members or one per member), and ONE CSR table on the device (batch.h BatchProfile),
    // freed by the destroy path.  Plain data, as the solids are and for the same reason; while a table is held every step of
    // batch.cpp launches through `step`, in front of the viscosity's, the openings' and the solids', and every successful
    // sfl_batch_set_solids calls `drop` (the stream is idle there), which frees the table and clears both.  walls.cpp sets
    // both with `on`; null, a batch launches exactly what it launched before there were walls.
    struct Walls {
        bool on = false;
        sfl::walls::Rows rows;
        void *d_table = nullptr;
        size_t d_bytes = 0;
        sfl::BatchProfile table{nullptr, nullptr, nullptr};
        int (*step)(sfl_batch *b, bool each, const sfl::BatchStep &a) = nullptr;
        void (*drop)(sfl_batch *b) = nullptr;
    } walls;
};

namespace sfl {
namespace host {

// The two hooks of the step calls (batch.cpp) into the recorder (batch_frames.cpp); both do nothing for a batch that is
// not recording.  record_admit: SFL_ERR_STATE if the n steps of a call would complete more frames than are free -- after
// the call's own argument checks, before anything is staged or launched.  record_step: one step has been launched and
// the ping-pong swapped; counts it (or the `steps` steps of one launch) and, when the count reaches a multiple of `every`, launches the frame's render on the
// batch's stream behind it.
int record_admit(sfl_batch *b, int n);
int record_step(sfl_batch *b, int steps = 1);
// ... for a launch that runs several steps (batch_play.hip): how many of the next n steps may run before a frame is due
// (n for a batch that is not recording), and record_step(b, steps) once they are launched: no frame falls inside them.
int record_run(const sfl_batch *b, int n);

}  // namespace host
}  // namespace sfl
