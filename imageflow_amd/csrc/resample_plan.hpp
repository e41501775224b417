// resample_plan.hpp -- what a resample launch will be, decided on the host: the tables of a plan and, per launch, which kernel
// runs with which geometry.  Pure arithmetic on the weight tables: nothing here calls the HIP runtime or looks at a device, so
// all of it runs (and is tested) on a machine without a GPU.  api.cpp uploads the tables and launches what is chosen here.
#pragma once
#include <hip/hip_vector_types.h>         // uint4, float4: plain types, no runtime

#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "device.hpp"

namespace ifhip {

constexpr uint32_t kComputeUnits = 256;          // MI355X
void set_cu_budget(uint32_t compute_units);      // ifhip_set_cu_budget: CUs the launches plan for (0: all of them)

// A vertical schedule of the fused kernel, built by the planner; its device copy is uploaded by the launcher the first time
// the schedule is launched.  Lives in its plan's map (guarded by PlanTables::mu), so a steady-state launch builds nothing.
struct PlannedSchedule {
    VSchedule host;
    VStep* d_steps = nullptr;
    uint32_t* d_band_begin = nullptr;
};

// The host tables of a plan (ifhip_resample_plan = these, their device copies and the device it belongs to).
struct PlanTables {
    uint32_t in_w = 0, in_h = 0, out_w = 0, out_h = 0;
    AxisWeights wv, wh;
    // de-duplicated, 4-tap padded horizontal weight rows and their per-output records {first tap column rounded down to 4,
    // 4-tap groups, weight row offset, taps valid in the last group}
    std::vector<float> wu;
    std::vector<uint4> hmeta;
    uint32_t h_avg_groups = 0;      // mean 4-tap groups per horizontal chain
    // fast horizontal pass: every output runs the same number G <= 4 of 4-tap groups (moderate ratios)
    uint32_t h_fast_groups = 0;     // 0: not available (some output needs more than 4 groups)
    std::vector<float> wg;          // distinct weight rows, each zero-padded to G groups
    std::vector<uint32_t> hmeta2;   // [out_w] first group | row id << 16
    // ... and its two-column form: G2 groups of 2 taps where that computes at most 2/3 of the taps per output (windows of 5-6 taps
    // aligned to 4 columns take 3 groups = 12 taps, aligned to 2 columns 4 groups = 8); no alpha, BGRA sources
    uint32_t h_two_groups = 0;      // 0: not available / not worth it
    std::vector<float> wg2;         // distinct weight rows, each zero-padded to G2 groups of 2
    std::vector<uint32_t> hmeta3;   // [out_w] first 2-column group | row id << 16
    // fused-kernel geometry
    bool fused_possible = false;
    int slots = 0;
    struct StripSet {                // column strips for one (alpha) variant of the fused kernel
        std::vector<Strip> strips;
        uint32_t max_quads = 0;
        bool ok = false;
    } sets[2];                       // [in_alpha_meaningful]
    // lazily built, guarded by mu
    mutable std::mutex mu;
    mutable std::map<uint64_t, PlannedSchedule> schedules;      // key: bands | group << 32 | ahead << 40
};
// (`filter`, sharpen_percent_goal) as ifhip_resample_plan_create takes them -> the kernel's description, or InvalidArgument
int resample_filter_spec(int filter, float sharpen_percent_goal, FilterSpec* out);
int build_plan_tables(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, const FilterSpec& spec, PlanTables* out);

// What a launch decision reads besides the tables.
struct LaunchInputs {
    int alpha = 0;
    bool ycc = false;                // planar YCbCr source (in_stride = sample pitch, in_image_bytes = plane size)
    uint32_t n_images = 0;
    size_t in_image_bytes = 0;
    uint32_t in_stride = 0;
    uintptr_t src_low_bits = 0;      // low four bits of the source pointers, OR-ed: the planner needs alignment, never the address
    int force_kernel = -1;           // -1 auto, 0 fused, 1 generic, 2 banded
    int working_space = IFHIP_SPACE_LINEAR;
    bool probe = false;              // planar source: the caller only asks whether the fused kernel takes it
    uint32_t cu_budget = 0;          // 0: all of kComputeUnits
    // test hooks (debug switches banded_wgs / banded_strip / banded_flags): workgroups of a banded launch (0: the default), forced
    // strip width (0: none), mask over the banded plan's flags
    uint32_t banded_wgs = 0, banded_strip = 0, banded_flags = 0xffffffffu;
};
LaunchInputs launch_inputs_now();    // cu_budget and the test hooks as they are set in this process; the rest at its defaults

enum class LaunchKernel { Fused, Banded, Generic };
struct LaunchChoice {
    int status = IFHIP_OK;           // IFHIP_OK, kNotFusable, or the error the launch fails with (message: last_error())
    LaunchKernel kernel = LaunchKernel::Generic;
    uint32_t grid = 0;               // fused, banded
    size_t lds = 0;
    // fused
    uint32_t lanes_per_frame = 0, frames_per_wg = 1, n_strips = 0;
    bool per_pixel = false;
    uint32_t fast_groups = 0;        // groups per output of the fast horizontal pass (0: the general pass on wu / hmeta)
    bool two_col = false;            // ... of two columns (wg2 / hmeta3) instead of four (wg / hmeta2)
    bool w_in_lds = false, l2s_in_lds = false;
    uint32_t lut_copies_log2 = 0;
    uint32_t want_bands = 0, n_bands = 0;          // asked of the schedule, obtained
    PlannedSchedule* schedule = nullptr;
    // banded
    BandedArgs banded{};
    uint32_t instead_of_fused_lanes = 0;           // != 0: chosen over a fused workgroup of this many lanes
    // generic
    uint32_t chunk = 0;              // frames per pass through the HBM scratch
};
LaunchChoice choose_launch(const PlanTables& t, const LaunchInputs& in);
// One line of text (no newline): the shape and everything choose_launch decided.  What the `trace_launch` switch prints.
std::string format_launch(const PlanTables& t, const LaunchInputs& in, const LaunchChoice& c);

}  // namespace ifhip
