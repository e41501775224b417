// resample_plan.cpp -- the planner of resample launches (resample_plan.hpp): host tables of a plan, kernel choice, launch
// geometry, and ifhip_describe_launch, which reports a decision without a device.  No HIP runtime call in this file.
#include "resample_plan.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace ifhip {
namespace {

constexpr size_t kLdsLimit = 160 * 1024;       // gfx950 LDS per CU == per-workgroup maximum
constexpr uint32_t kMaxStripOutputs = 2048;
constexpr uint32_t kMinLutCopiesLog2 = 4;      // never fewer than 16 copies of the sRGB->float table (2-way conflicts)
std::atomic<uint32_t> g_cu_budget{0};

size_t fused_lds_bytes(uint32_t n_u, uint32_t nquads, int channels, uint32_t wu_floats, bool w_in_lds, bool l2s_in_lds,
                       uint32_t lut_copies_log2, bool per_pixel, uint32_t frames = 1, uint32_t fast_groups = 0) {
    return fused_lds_layout(n_u, nquads, wu_floats, channels, w_in_lds, l2s_in_lds, lut_copies_log2, per_pixel, frames, fast_groups).total;
}
// Horizontal pass mapping: one lane per output pixel (its C chains interleave, encode + store follow at once, no obuf
// round trip) measured faster than one lane per (pixel, channel) on every BASELINE shape (cfg2 -2.6 %, cfg2 with alpha
// -10 %, cfg3 -27 %); the per-channel form is kept for strips with less than one wave of outputs, where it is the only
// way to spread the (long) chains over more lanes.
bool use_per_pixel(uint32_t max_nu, int channels, uint32_t block) {
    return max_nu >= 64u || static_cast<uint64_t>(max_nu) * static_cast<uint32_t>(channels) > block;
}
uint32_t block_for(uint32_t max_quads, int px) {          // lanes of a frame slot: one per px source pixels, whole waves
    return std::max<uint32_t>(64u, (max_quads * static_cast<uint32_t>(4 / px) + 63u) & ~63u);
}

// Split the output columns into strips whose staged source span fits one workgroup (max_lanes lanes x 4 px)
// and whose minimal LDS footprint fits the CU.
bool plan_strips(const AxisWeights& wh, uint32_t max_lanes, int px, int channels, std::vector<Strip>* out, uint32_t* max_quads) {
    for (uint32_t n = 1; n <= wh.n_out; ++n) {
        std::vector<Strip> s;
        bool ok = true;
        uint32_t mq = 0, mu = 0;
        for (uint32_t i = 0; i < n && ok; ++i) {
            Strip t;
            t.u0 = static_cast<uint32_t>(static_cast<uint64_t>(wh.n_out) * i / n);
            t.u1 = static_cast<uint32_t>(static_cast<uint64_t>(wh.n_out) * (i + 1) / n);
            if (t.u1 <= t.u0) { ok = false; break; }
            uint32_t lo = wh.left[t.u0], hi = 0;
            for (uint32_t u = t.u0; u < t.u1; ++u) {
                lo = std::min(lo, wh.left[u]);
                hi = std::max(hi, wh.left[u] + wh.count[u]);
            }
            t.cx0 = lo & ~3u;
            t.nquads = (hi - t.cx0 + 3u) / 4u;
            if (t.nquads > max_lanes || (t.u1 - t.u0) > kMaxStripOutputs) ok = false;
            mq = std::max(mq, t.nquads);
            mu = std::max(mu, t.u1 - t.u0);
            s.push_back(t);
        }
        if (ok) {
            const bool pp = use_per_pixel(mu, channels, block_for(mq, px));
            for (const Strip& t : s)
                if (fused_lds_bytes(t.u1 - t.u0, t.nquads, channels, 0, false, false, kMinLutCopiesLog2, pp) > kLdsLimit) ok = false;
        }
        if (ok) { *out = std::move(s); *max_quads = mq; return true; }
        if (n > 4096) break;
    }
    return false;
}

PlannedSchedule* get_schedule(const PlanTables& t, uint32_t n_bands, int group, int ahead) {
    std::lock_guard<std::mutex> lk(t.mu);
    const uint64_t key = static_cast<uint64_t>(n_bands) | (static_cast<uint64_t>(group) << 32) | (static_cast<uint64_t>(ahead) << 40);
    auto it = t.schedules.find(key);
    if (it == t.schedules.end()) {
        PlannedSchedule s;
        if (!build_vschedule(t.wv, static_cast<int>(n_bands), group, ahead, &s.host)) {
            fail(IFHIP_INVALID_STATE, "InvalidState: vertical schedule could not be built");
            return nullptr;
        }
        it = t.schedules.emplace(key, std::move(s)).first;
    }
    return &it->second;
}

uint32_t choose_bands(const PlanTables& p, uint32_t cu_budget, uint32_t n_images, size_t n_strips) {
    // One workgroup occupies a CU (LDS), so a launch runs in ceil(workgroups / 256) rounds.  Cutting frames into bands
    // of output rows makes the rounds finer but every extra band re-reads its halo of source rows and stages the tables
    // again (a few microseconds per workgroup: `setup`, as a share of one frame's time on one CU); pick the band count with
    // the smallest estimated time.  Up to 64 bands: a launch of ONE frame (a job through the ABI) then spreads over 64 CUs
    // instead of 16 -- 3840x2160 -> 800x450 as a single frame: 118 us with 16 bands (round 5, profiles/r5_abi_*).
    const double wgs = static_cast<double>(n_images) * static_cast<double>(n_strips);
    const double halo = p.out_h ? static_cast<double>(p.wv.max_taps) / std::max<double>(1.0, p.in_h) : 0.0;
    const double setup = 0.01;
    const double cus = cu_budget ? static_cast<double>(cu_budget) : static_cast<double>(kComputeUnits);
    const uint32_t max_bands = std::max<uint32_t>(1u, std::min<uint32_t>(64u, p.out_h / 4u));
    uint32_t best = 1;
    double best_cost = 1e300;
    for (uint32_t b = 1; b <= max_bands; ++b) {
        const double rounds = std::ceil(wgs * b / cus);
        const double cost = rounds * ((1.0 + halo * (b - 1)) / b + setup);
        if (cost < best_cost - 1e-9) { best_cost = cost; best = b; }
    }
    return best;
}

bool fused_usable(const PlanTables& p, const LaunchInputs& in) {
    if (!p.fused_possible || !p.sets[in.alpha ? 1 : 0].ok) return false;
    if (in.ycc) {                       // three component planes: 4-byte reads of 4 samples
        if (in.alpha || fused_shape(p.slots, 3).px != 4) return false;
        if ((in.src_low_bits & 3u) || (in.in_image_bytes & 3u) || (in.in_stride & 3u)) return false;
        for (const Strip& s : p.sets[0].strips)
            if (static_cast<uint64_t>(s.cx0) + 4u * s.nquads > in.in_stride) return false;
        return true;
    }
    if ((in.src_low_bits & 15u) || (in.in_image_bytes & 15u) || (in.in_stride & 15u)) return false;
    for (const Strip& s : p.sets[in.alpha ? 1 : 0].strips)
        if (static_cast<uint64_t>(s.cx0 + 4u * s.nquads) * 4u > in.in_stride) return false;   // 16-byte row reads stay inside the row
    return true;
}

// Banded two-pass kernel (resample_kernels.hip): R output rows per workgroup, their source rows and vertically filtered
// rows in LDS beside the tables.  R is the largest of a short list for which two workgroups share a CU; failing that,
// whatever fits one.  A band's workgroups split the frames between them (frame_step), so that the tables are staged a few
// times per CU and not once per frame and band.
constexpr size_t kBandedTables = 16384 + 1024 + 16;
constexpr uint32_t kBandedWorkgroups = 8192;                 // sixteen rounds of two workgroups per CU (measured: 512 4.09, 1 024 3.91, 2 048 3.76, 4 096 3.70, 8 192 3.66 ms on the 3x shape)
bool banded_plan(const PlanTables& p, const LaunchInputs& in, LaunchChoice* bp) {
    if ((in.src_low_bits | in.in_image_bytes | in.in_stride) & 3u) return false;                  // 4-byte pixel reads
    if (in.in_image_bytes > 0xffffffffull) return false;                                           // 32-bit offsets inside a frame
    const AxisWeights& wv = p.wv;
    const uint32_t out_h = p.out_h;
    auto src_rows_of = [&](uint32_t R) {                    // widest source window of any band of R output rows
        uint32_t worst = 0;
        for (uint32_t j0 = 0; j0 < out_h; j0 += R) {
            uint32_t lo = 0xffffffffu, hi = 0;
            for (uint32_t j = j0; j < std::min(out_h, j0 + R); ++j) { lo = std::min(lo, wv.left[j]); hi = std::max(hi, wv.left[j] + wv.count[j]); }
            worst = std::max(worst, hi - lo);
        }
        return worst;
    };
    uint32_t src_rows_memo[65] = {};                        // (asked for the same dozen R by every candidate strip width)
    auto src_rows = [&](uint32_t R) { return R <= 64u ? (src_rows_memo[R] ? src_rows_memo[R] : (src_rows_memo[R] = src_rows_of(R))) : src_rows_of(R); };
    bool ascending = true;                                  // window starts and ends never step back (they do not, but the kernel's
    for (uint32_t j = 1; j < out_h; ++j)                    // shortcut rests on it, so it is checked, not assumed)
        if (wv.left[j] < wv.left[j - 1] || wv.left[j] + wv.count[j] < wv.left[j - 1] + wv.count[j - 1]) ascending = false;
    const AxisWeights& wh = p.wh;
    const uint32_t out_w = p.out_w;
    static const uint32_t kRows[] = {64, 48, 32, 24, 16, 12, 8, 6, 4, 3, 2, 1};
    const uint32_t wgs = in.banded_wgs ? in.banded_wgs : kBandedWorkgroups;      // test hook: the frame loop of a workgroup
    auto commit = [&](uint32_t R, uint32_t ns, uint32_t strip_w, uint32_t hwf, bool h_lds, size_t lds) {
        BandedArgs& b = bp->banded;
        b.rows_per_band = R; b.n_bands = (out_h + R - 1u) / R; b.src_rows_cap = ns;
        b.strip_w = strip_w; b.n_strips = (out_w + strip_w - 1u) / strip_w;
        b.frame_step = std::max<uint32_t>(1u, std::min<uint32_t>(in.n_images, wgs / std::max(1u, b.n_bands * b.n_strips)));
        b.h_w_floats = hwf;
        b.flags = (ascending ? 2u : 0u) | (h_lds ? 4u : 0u);
        bp->grid = b.n_bands * b.n_strips * b.frame_step;
        bp->lds = lds;
    };
    // ---- whole rows (small frames): R is the largest of the list for which two workgroups share a CU, else whatever fits one ----
    // horizontal tables in LDS when they are small (up-scales: ~5 taps per output column)
    const size_t h_bytes = ((3u * static_cast<size_t>(out_w) + wh.w.size()) * 4u + 15u) & ~static_cast<size_t>(15u);
    const bool h_lds = h_bytes <= 32u * 1024u;
    const size_t tables = kBandedTables + (h_lds ? h_bytes : 0u);
    const size_t row_bytes = static_cast<size_t>(p.in_w) * 16u;
    uint32_t whole_R = 0, whole_ns = 0; size_t whole_lds = 0;
    for (int pass = 0; pass < 2 && !whole_R; ++pass) {
        const size_t budget = pass == 0 ? kLdsLimit / 2 : kLdsLimit;
        for (uint32_t R0 : kRows) {
            const uint32_t R = std::min(R0, out_h);
            if (pass == 0 && R < 4u && out_h >= 4u) break;
            const uint32_t ns = src_rows(R);
            const size_t lds = tables + static_cast<size_t>(ns + R) * row_bytes;
            if (lds <= budget) { whole_R = R; whole_ns = ns; whole_lds = lds; break; }
        }
    }
    // ---- column strips (wide frames): where whole rows leave a band of fewer than 16 rows (each band converts its own halo of
    // source rows and stages the tables again) or do not fit at all, a workgroup takes a strip of S output columns of a band
    // of R rows; its source columns and its slice of the weights are the union of its columns' windows. ----
    const uint32_t forced_strip = in.banded_strip;          // test hook: strips on small frames
    const bool whole_good = whole_R != 0 && (whole_R >= 16u || whole_R >= out_h);
    if ((whole_good && !forced_strip) || out_w < 2u) {
        if (!whole_R) return false;
        commit(whole_R, whole_ns, out_w, static_cast<uint32_t>(wh.w.size()), h_lds, whole_lds);
        return true;
    }
    auto pad64 = [](uint32_t v) { return (v + 63u) / 64u * 64u; };
    const double nv = static_cast<double>(wv.w.size()) / std::max(1u, out_h);          // mean taps of the vertical windows
    // cost per output pixel, in tap steps (one 16-byte LDS read + its multiply-adds): converting the tile's source pixels (three
    // table reads each: 3), the vertical pass over the strip's source columns, both with their idle lanes; a tile that leaves no
    // room for a second workgroup on the CU waits out its own barriers (x 1.25)
    auto cost_of = [&](uint32_t R, uint32_t ns, uint32_t S, uint32_t sc, size_t lds) {
        const double px = static_cast<double>(R) * S;
        return (3.0 * ns * pad64(sc) + nv * R * pad64(sc) + 8.0 * R * pad64(S)) / px * (lds > kLdsLimit / 2 ? 1.25 : 1.0);
    };
    double best = 1e300;
    struct { uint32_t R, ns, S, hwf; bool h_lds; size_t lds; } pick{};
    if (whole_R && !forced_strip) {
        best = cost_of(whole_R, whole_ns, out_w, p.in_w, whole_lds);
        pick = {whole_R, whole_ns, out_w, static_cast<uint32_t>(wh.w.size()), h_lds, whole_lds};
    }
    static const uint32_t kStrips[] = {512, 384, 256, 192, 128, 112, 96, 64, 48, 32, 16};
    for (uint32_t S0 : kStrips) {
        const uint32_t S = forced_strip ? std::min(forced_strip, out_w) : S0;
        if (S >= out_w && !forced_strip) continue;
        uint32_t sc = 0, hwf = 0;                            // widest strip: source columns, floats of its weight slice
        for (uint32_t u0 = 0; u0 < out_w; u0 += S) {
            const uint32_t u1 = std::min(out_w, u0 + S);
            uint32_t lo = 0xffffffffu, hi = 0, wlo = 0xffffffffu, whi = 0;       // (as the kernel finds them)
            for (uint32_t u = u0; u < u1; ++u) {
                lo = std::min(lo, wh.left[u]); hi = std::max(hi, wh.left[u] + wh.count[u]);
                wlo = std::min(wlo, wh.offset[u]); whi = std::max(whi, wh.offset[u] + wh.count[u]);
            }
            sc = std::max(sc, hi - lo);
            hwf = std::max(hwf, whi - wlo);
        }
        const size_t hb = ((3u * static_cast<size_t>(S) + hwf) * 4u + 15u) & ~static_cast<size_t>(15u);
        const bool hl = hb <= 32u * 1024u;
        for (uint32_t R0 : kRows) {
            const uint32_t R = std::min(R0, out_h);
            const uint32_t ns = src_rows(R);
            const size_t lds = kBandedTables + (hl ? hb : 0u) + static_cast<size_t>(ns + R) * sc * 16u;
            if (lds > kLdsLimit) continue;
            const double c = cost_of(R, ns, S, sc, lds);
            if (c < best) { best = c; pick = {R, ns, S, hwf, hl, lds}; }
        }
        if (forced_strip) break;
    }
    if (best == 1e300) return false;
    commit(pick.R, pick.ns, pick.S, pick.hwf, pick.h_lds, pick.lds);
    return true;
}
// The banded kernel stands in for the generic pair wherever it fits (measured, MI355X: 3x up-scale 9.97 -> 3.65 ms), never for
// the fused kernel (the 2x up-scale the fused kernel takes is faster there: 2.93 vs 4.43 ms).

LaunchChoice failed(int status) { LaunchChoice c; c.status = status; return c; }

// Geometry of the fused kernel for this launch, or the error it fails with.
LaunchChoice fused_plan(const PlanTables& p, const LaunchInputs& in) {
    LaunchChoice c;
    c.kernel = LaunchKernel::Fused;
    const bool alpha = in.alpha != 0, linear = in.working_space == IFHIP_SPACE_LINEAR;
    const PlanTables::StripSet& ss = p.sets[alpha ? 1 : 0];
    c.n_strips = static_cast<uint32_t>(ss.strips.size());
    const int channels = alpha ? 4 : 3;
    const uint32_t block = block_for(ss.max_quads, fused_shape(p.slots, channels).px);
    uint32_t max_nu = 0;
    for (const Strip& s : ss.strips) max_nu = std::max(max_nu, s.u1 - s.u0);
    const bool per_pixel = use_per_pixel(max_nu, channels, block);
    const size_t limit = kLdsLimit;
    // The fast horizontal pass (same group count G for every output, rows padded with +0 weights) needs the padded
    // weight rows in LDS and the per-pixel mapping; when that does not fit, plan again for the general pass.
    uint32_t frames = 1, copies_log2 = kMinLutCopiesLog2, fast_g = 0, wu_floats = static_cast<uint32_t>(p.wu.size());
    bool w_in_lds = false, l2s_in_lds = false;
    // forms of the horizontal pass, best first: two-column groups, four-column groups (both: the fast pass), general
    const bool fast_ok = per_pixel && p.h_fast_groups && fused_shape(p.slots, channels).px == 4;
    const bool two_ok = fast_ok && p.h_two_groups && !alpha && !in.ycc;
    bool two = false;
    for (int attempt = two_ok ? -1 : (fast_ok ? 0 : 1); attempt < 2; ++attempt) {
        two = attempt < 0;
        fast_g = two ? p.h_two_groups : (attempt == 0 ? p.h_fast_groups : 0u);
        wu_floats = static_cast<uint32_t>(two ? p.wg2.size() : (fast_g ? p.wg.size() : p.wu.size()));
        // Frames per workgroup: a source narrower than half the workgroup would leave the CU with a handful of waves
        // (one workgroup per CU: the tables fill most of the LDS), so F frames share a workgroup and its tables.
        frames = 1;
        if (ss.strips.size() == 1) {
            const uint32_t max_f = std::min<uint32_t>(static_cast<uint32_t>(fused_max_threads(p.slots, channels)) / block, in.n_images);
            const Strip& s0 = ss.strips[0];
            for (uint32_t f = max_f; f > 1; --f)
                if (fused_lds_bytes(s0.u1 - s0.u0, s0.nquads, channels, wu_floats, true, linear, kMinLutCopiesLog2, per_pixel, f, fast_g) <= limit) {
                    frames = f;
                    break;
                }
        }
        // bands: by the number of workgroups the launch really has (frames / F per strip)
        c.want_bands = choose_bands(p, in.cu_budget, (in.n_images + frames - 1u) / frames, ss.strips.size());
        c.schedule = get_schedule(p, c.want_bands, fused_shape(p.slots, channels).rows_in_flight, fused_lookahead(p.slots, channels));
        if (!c.schedule) return failed(IFHIP_INVALID_STATE);
        c.n_bands = static_cast<uint32_t>(c.schedule->host.band_begin.size() - 1);
        // LDS budget beyond the minimum the strips were planned for (double-buffered rows + 16 copies of the sRGB->float
        // table): the de-duplicated horizontal weight rows, then -- by lookup cost -- the second 16 table copies and the
        // 16 KiB linear->sRGB table (otherwise encoded by threshold search)
        auto fits = [&](bool w, bool l2s, uint32_t copies_log2) {
            for (const Strip& s : ss.strips)
                if (fused_lds_bytes(s.u1 - s.u0, s.nquads, channels, wu_floats, w, l2s, copies_log2, per_pixel, frames, fast_g) > limit) return false;
            return true;
        };
        w_in_lds = fits(true, false, kMinLutCopiesLog2);
        // What goes next depends on where the lookups are: the 16 KiB linear->sRGB table saves an 8-step threshold
        // search (~40 instructions) per encoded channel, the second set of 16 table copies saves one LDS conflict cycle
        // per converted sample.  Per output row a strip encodes 3*n_u channels and converts 12*nquads*(in_h/out_h)
        // samples; thumbnail-sized outputs (cfg2) want the copies first, moderate ratios (cfg3) the encode table.
        const double enc_cost = 3.0 * max_nu * 40.0;
        const double conv_cost = 12.0 * ss.max_quads * (static_cast<double>(p.in_h) / std::max<uint32_t>(1u, p.out_h)) * 2.0;
        const bool l2s_allowed = linear;
        copies_log2 = kMinLutCopiesLog2;
        l2s_in_lds = false;
        if (enc_cost > conv_cost) {
            l2s_in_lds = l2s_allowed && fits(w_in_lds, true, kMinLutCopiesLog2);
            if (fits(w_in_lds, l2s_in_lds, 5)) copies_log2 = 5u;
        } else {
            if (fits(w_in_lds, false, 5)) copies_log2 = 5u;
            l2s_in_lds = l2s_allowed && fits(w_in_lds, true, copies_log2);
        }
        if (!fast_g || w_in_lds) break;
    }
    if (in.ycc && !(w_in_lds && per_pixel)) return failed(kNotFusable);     // the planar source is instantiated for that form only
    c.lanes_per_frame = block; c.frames_per_wg = frames; c.per_pixel = per_pixel;
    c.fast_groups = fast_g; c.two_col = two;
    c.w_in_lds = w_in_lds; c.l2s_in_lds = l2s_in_lds; c.lut_copies_log2 = copies_log2;
    for (const Strip& s : ss.strips)
        c.lds = std::max(c.lds, fused_lds_bytes(s.u1 - s.u0, s.nquads, channels, wu_floats, w_in_lds, l2s_in_lds, copies_log2, per_pixel, frames, fast_g));
    if (c.lds > kLdsLimit) return failed(fail(IFHIP_INVALID_STATE, "InvalidState: fused kernel LDS plan exceeds the CU (%zu bytes)", c.lds));
    const uint64_t grid = static_cast<uint64_t>((in.n_images + frames - 1u) / frames) * c.n_bands * c.n_strips;
    if (grid > 0x7fffffffull) return failed(fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: batch too large for one launch"));
    c.grid = static_cast<uint32_t>(grid);
    return c;
}

}  // namespace

void set_cu_budget(uint32_t compute_units) { g_cu_budget.store(compute_units, std::memory_order_relaxed); }

LaunchInputs launch_inputs_now() {
    LaunchInputs in;
    in.cu_budget = g_cu_budget.load(std::memory_order_relaxed);
    if (const char* e = debug_switch("banded_wgs")) in.banded_wgs = static_cast<uint32_t>(std::max(1, std::atoi(e)));
    if (const char* e = debug_switch("banded_strip")) in.banded_strip = static_cast<uint32_t>(std::max(0, std::atoi(e)));
    // masks the banded plan's flags (2 band rows from its first and last row, 4 horizontal tables in LDS) so that the kernel's
    // table-free forms, which real weight tables reach only at very wide outputs, run in the suite
    if (const char* e = debug_switch("banded_flags")) in.banded_flags = static_cast<uint32_t>(std::atoi(e));
    return in;
}

int resample_filter_spec(int filter, float sharpen_percent_goal, FilterSpec* out) {
    if (!filter_spec_for(filter, out)) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: unknown filter %d", filter);
    if (sharpen_percent_goal > 0.0f) {               // scaling.rs:103-105 -> LobeRatio::SharpenPercent
        out->lobe_mode = IFHIP_LOBE_SHARPEN_PERCENT;
        out->lobe_value = sharpen_percent_goal;
    }
    return IFHIP_OK;
}

int build_plan_tables(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, const FilterSpec& spec, PlanTables* p) {
    p->in_w = in_w; p->in_h = in_h; p->out_w = w; p->out_h = h;
    int rc = build_axis_weights(spec, h, in_h, &p->wv);
    if (rc) return rc;
    rc = build_axis_weights(spec, w, in_w, &p->wh);
    if (rc) return rc;

    // Horizontal weight rows for the fused kernel.  A row starts at the output's first tap rounded DOWN to a multiple
    // of 4 source columns (so that a lane gathers 4 taps with one aligned 16-byte LDS read), the skipped columns get
    // weight +0.0f (exact: fmaf(+0, x, +0) == +0 for finite x, and the chain starts at +0), and the row is zero-padded
    // to a multiple of 4 (the kernel predicates the taps of the last group).  Rows are then de-duplicated bit for
    // bit: at rational scale factors they recur with period out_w / gcd(in_w, out_w) (3840 -> 200: 36 rows of 200),
    // which is what lets the whole table live in LDS.
    std::vector<float>& wu = p->wu;
    std::vector<uint4>& hmeta = p->hmeta;
    hmeta.resize(w);
    {
        std::map<std::vector<uint32_t>, uint32_t> seen;        // row bits -> offset in wu
        uint64_t groups = 0;
        for (uint32_t u = 0; u < w; ++u) {
            const uint32_t n = p->wh.count[u], lead = p->wh.left[u] & 3u, total = lead + n, npad = (total + 3u) & ~3u;
            std::vector<uint32_t> bits(npad, 0u);
            std::memcpy(bits.data() + lead, p->wh.w.data() + p->wh.offset[u], n * sizeof(float));
            auto it = seen.find(bits);
            if (it == seen.end()) {
                const uint32_t off = static_cast<uint32_t>(wu.size());
                wu.resize(wu.size() + npad, 0.0f);
                std::memcpy(wu.data() + off, bits.data(), npad * sizeof(float));
                it = seen.emplace(std::move(bits), off).first;
            }
            hmeta[u] = make_uint4(p->wh.left[u] & ~3u, npad / 4u, it->second, ((total - 1u) & 3u) + 1u);
            groups += npad / 4u;
        }
        p->h_avg_groups = static_cast<uint32_t>((groups + w - 1u) / w);
    }
    // Fast horizontal pass: when no output needs more than 4 groups, pad every row to the common count G -- the extra
    // groups carry weight +0 (exact, as the leading zeros above) -- so that the kernel runs G unrolled groups per
    // output with immediate LDS offsets, no per-lane trip count and a 4-byte record per output.
    std::vector<float>& wg = p->wg;
    std::vector<uint32_t>& hmeta2 = p->hmeta2;
    hmeta2.resize(w);
    {
        uint32_t g_max = 0;
        for (uint32_t u = 0; u < w; ++u) g_max = std::max(g_max, hmeta[u].y);
        if (g_max >= 2u && g_max <= 4u) {
            std::map<std::vector<uint32_t>, uint32_t> seen;        // padded row bits -> row id
            const uint32_t row_floats = g_max * 4u;
            bool ok = true;
            for (uint32_t u = 0; u < w && ok; ++u) {
                std::vector<uint32_t> bits(row_floats, 0u);
                std::memcpy(bits.data(), wu.data() + hmeta[u].z, hmeta[u].y * 16u);
                auto it = seen.find(bits);
                if (it == seen.end()) {
                    const uint32_t id = static_cast<uint32_t>(seen.size());
                    if (id >= 65536u) { ok = false; break; }
                    wg.resize(wg.size() + row_floats);
                    std::memcpy(wg.data() + static_cast<size_t>(id) * row_floats, bits.data(), row_floats * 4u);
                    it = seen.emplace(std::move(bits), id).first;
                }
                if ((hmeta[u].x >> 2) >= 65536u) { ok = false; break; }
                hmeta2[u] = (hmeta[u].x >> 2) | (it->second << 16);
            }
            if (ok) p->h_fast_groups = g_max;
        }
    }
    // The same with groups of TWO source columns (8-byte LDS reads): a row starts at the first tap rounded down to an even
    // column.  Worth it where it computes a third fewer taps per output: 1600 -> 1200 Robidoux has 5-6 taps per output,
    // 3 groups of 4 (12 taps) or 4 groups of 2 (8): cfg3 level 1 2.91 -> 2.70 ms; 1200 -> 400 (16 taps or 12) measured equal
    // and stays with groups of four.  The taps keep their order and the padding is +0: same pixels.
    std::vector<float>& wg2 = p->wg2;
    std::vector<uint32_t>& hmeta3 = p->hmeta3;
    hmeta3.resize(w);
    if (p->h_fast_groups) {
        uint32_t g2_max = 0;
        for (uint32_t u = 0; u < w; ++u) g2_max = std::max(g2_max, ((p->wh.left[u] & 1u) + p->wh.count[u] + 1u) >> 1);
        if (g2_max >= 2u && g2_max <= 6u && 3u * g2_max <= 4u * p->h_fast_groups) {     // at most 2/3 of the taps (measured: 3/4 gains nothing)
            std::map<std::vector<uint32_t>, uint32_t> seen;
            const uint32_t row_floats = g2_max * 2u;
            bool ok = true;
            for (uint32_t u = 0; u < w && ok; ++u) {
                std::vector<uint32_t> bits(row_floats, 0u);
                std::memcpy(bits.data() + (p->wh.left[u] & 1u), p->wh.w.data() + p->wh.offset[u], p->wh.count[u] * sizeof(float));
                auto it = seen.find(bits);
                if (it == seen.end()) {
                    const uint32_t id = static_cast<uint32_t>(seen.size());
                    if (id >= 65536u) { ok = false; break; }
                    wg2.resize(wg2.size() + row_floats);
                    std::memcpy(wg2.data() + static_cast<size_t>(id) * row_floats, bits.data(), row_floats * 4u);
                    it = seen.emplace(std::move(bits), id).first;
                }
                if ((p->wh.left[u] >> 1) >= 65536u) { ok = false; break; }
                hmeta3[u] = (p->wh.left[u] >> 1) | (it->second << 16);
            }
            if (ok) {
                while (wg2.size() & 3u) wg2.push_back(0.0f);             // (staged into LDS in 16-byte pieces)
                p->h_two_groups = g2_max;
            }
        }
    }

    p->slots = max_live_rows(p->wv);
    VSchedule probe;
    p->fused_possible = p->slots >= 1 && p->slots <= kMaxSlots && build_vschedule(p->wv, 1, 4, 5, &probe);
    for (int al = 0; al < 2 && p->fused_possible; ++al) {
        const int channels = al ? 4 : 3;
        PlanTables::StripSet& ss = p->sets[al];
        const uint32_t max_lanes = static_cast<uint32_t>(fused_max_quads(p->slots, channels));      // in 4-pixel groups
        ss.ok = plan_strips(p->wh, max_lanes, fused_shape(p->slots, channels).px, channels, &ss.strips, &ss.max_quads);
    }
    return IFHIP_OK;
}

LaunchChoice choose_launch(const PlanTables& p, const LaunchInputs& in) {
    bool fused = fused_usable(p, in);
    if (in.ycc && !fused) return failed(kNotFusable);       // the planar source exists on the fused kernel only
    if (in.force_kernel == 0 && !fused)
        return failed(fail(IFHIP_INVALID_STATE, "InvalidState: fused kernel requested but its preconditions do not hold "
                           "(live rows %d > %d, or rows not 16-byte aligned / padded)", p.slots, kMaxSlots));
    if (in.force_kernel == 1) fused = false;

    // banded two-pass kernel: asked for (force_kernel 2), or in auto mode where the fused kernel does not apply
    if (!in.ycc && (in.force_kernel == 2 || in.force_kernel == -1)) {
        LaunchChoice c;
        c.kernel = LaunchKernel::Banded;
        if ((in.force_kernel == 2 || !fused) && banded_plan(p, in, &c)) {
            c.banded.flags &= in.banded_flags;
            return c;
        }
        if (in.force_kernel == 2)
            return failed(fail(IFHIP_INVALID_STATE, "InvalidState: banded kernel requested but a band's source rows do not fit the LDS "
                               "(or the source pixels are not 4-byte aligned)"));
    }

    if (fused) {
        const LaunchChoice c = fused_plan(p, in);
        // Up-scales with alpha whose geometry leaves the CU a workgroup of at most four waves (a 1 440 - 2 048 column source cut
        // into two strips, the output rows of one frame filling the LDS so that no second frame shares the workgroup) run on the
        // banded kernel's column strips instead: 0.34 - 0.89 of the fused kernel's time on every such shape and filter measured
        // (profiles/r6_fused_vs_banded_upscales.jsonl); with five or more waves, and without alpha, the fused kernel stays ahead.
        const uint32_t lanes = c.lanes_per_frame * c.frames_per_wg;
        if (c.status == IFHIP_OK && in.force_kernel == -1 && !in.ycc && !in.probe && in.alpha && lanes <= 256u &&
            4ull * p.out_w >= 5ull * p.in_w && 4ull * p.out_h >= 5ull * p.in_h) {
            LaunchChoice b;
            b.kernel = LaunchKernel::Banded;
            b.instead_of_fused_lanes = lanes;
            if (banded_plan(p, in, &b)) return b;
        }
        return c;
    }

    // generic two-pass path through an HBM scratch of [chunk][out_h][in_w] float4
    if (p.out_h > 65535u) return failed(fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: output taller than 65535 rows"));
    LaunchChoice c;
    const size_t per_image = static_cast<size_t>(p.out_h) * p.in_w * sizeof(float4);
    const size_t budget = static_cast<size_t>(1) << 30;
    c.chunk = static_cast<uint32_t>(std::max<size_t>(1, std::min<size_t>(in.n_images, budget / std::max<size_t>(per_image, 1))));
    c.chunk = std::min<uint32_t>(c.chunk, 65535u);
    return c;
}

std::string format_launch(const PlanTables& p, const LaunchInputs& in, const LaunchChoice& c) {
    char s[512];
    if (c.kernel == LaunchKernel::Banded && c.instead_of_fused_lanes)
        std::snprintf(s, sizeof s, "ifhip banded launch (instead of a %u-lane fused workgroup): %ux%u -> %ux%u rows/band=%u strip=%u strips=%u grid=%u lds=%zu images=%u",
                      c.instead_of_fused_lanes, p.in_w, p.in_h, p.out_w, p.out_h, c.banded.rows_per_band, c.banded.strip_w, c.banded.n_strips, c.grid, c.lds, in.n_images);
    else if (c.kernel == LaunchKernel::Banded)
        std::snprintf(s, sizeof s, "ifhip banded launch: %ux%u -> %ux%u alpha=%d rows/band=%u bands=%u src rows=%u strip=%u strips=%u frame step=%u flags=%u grid=%u lds=%zu images=%u",
                      p.in_w, p.in_h, p.out_w, p.out_h, in.alpha, c.banded.rows_per_band, c.banded.n_bands, c.banded.src_rows_cap,
                      c.banded.strip_w, c.banded.n_strips, c.banded.frame_step, c.banded.flags, c.grid, c.lds, in.n_images);
    else if (c.kernel == LaunchKernel::Fused)
        std::snprintf(s, sizeof s, "ifhip fused launch: %ux%u -> %ux%u K=%d alpha=%d ycc=%d lanes/frame=%u frames/wg=%u bands=%u strips=%u "
                      "grid=%llu lds=%zu fast_g=%u two_col=%d w_in_lds=%d l2s_in_lds=%d lut_copies=%u per_pixel=%d images=%u",
                      p.in_w, p.in_h, p.out_w, p.out_h, p.slots, in.alpha, in.ycc ? 1 : 0, c.lanes_per_frame, c.frames_per_wg, c.n_bands, c.n_strips,
                      static_cast<unsigned long long>(c.grid), c.lds, c.fast_groups, c.two_col ? 1 : 0, c.w_in_lds ? 1 : 0, c.l2s_in_lds ? 1 : 0,
                      1u << c.lut_copies_log2, c.per_pixel ? 1 : 0, in.n_images);
    else
        std::snprintf(s, sizeof s, "ifhip generic launch: %ux%u -> %ux%u alpha=%d chunk=%u images=%u", p.in_w, p.in_h, p.out_w, p.out_h, in.alpha, c.chunk, in.n_images);
    return s;
}

}  // namespace ifhip

extern "C" int ifhip_describe_launch(uint32_t in_w, uint32_t in_h, uint32_t w, uint32_t h, int filter, float sharpen_percent_goal,
                                     int in_alpha_meaningful, int planar_ycc_source, uint32_t n_images, uint32_t in_stride,
                                     size_t in_image_bytes, uint32_t source_alignment, int working_space, int force_kernel,
                                     char* line, size_t line_capacity) {
    using namespace ifhip;
    if (!line || line_capacity == 0) return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: null line buffer");
    line[0] = '\0';
    if (w == 0 || h == 0 || in_w == 0 || in_h == 0)
        return fail(IFHIP_INVALID_ARGUMENT, "InvalidArgument: Bitmap dimensions cannot be zero");
    if (working_space != IFHIP_SPACE_SRGB && working_space != IFHIP_SPACE_LINEAR)
        return fail(IFHIP_METHOD_NOT_IMPLEMENTED, "MethodNotImplemented: working floatspace %d", working_space);
    FilterSpec spec;
    int rc = resample_filter_spec(filter, sharpen_percent_goal, &spec);
    if (rc) return rc;
    PlanTables t;
    if ((rc = build_plan_tables(in_w, in_h, w, h, spec, &t))) return rc;
    if (n_images == 0) return IFHIP_OK;                 // (nothing is launched)
    LaunchInputs in = launch_inputs_now();
    in.alpha = in_alpha_meaningful; in.ycc = planar_ycc_source != 0; in.n_images = n_images;
    in.in_image_bytes = in_image_bytes; in.in_stride = in_stride;
    in.src_low_bits = source_alignment & 15u;           // a pointer aligned to A < 16 bytes and no further has bit A set
    in.force_kernel = force_kernel; in.working_space = working_space;
    const LaunchChoice c = choose_launch(t, in);
    if (c.status) return c.status == kNotFusable ? fail(IFHIP_INVALID_STATE, "InvalidState: the fused kernel does not take this planar source") : c.status;
    std::snprintf(line, line_capacity, "%s", format_launch(t, in, c).c_str());
    return IFHIP_OK;
}
