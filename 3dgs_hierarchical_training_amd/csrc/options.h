// options.h -- the library's run-time options (gsr_set_option, include/gsr.h): one struct that holds them with their defaults, one
// table of the names that set them, one table of the retired names, and a process-wide instance behind a mutex.  Plain C++17: the
// host code of gsr_kernels.hip includes it, and so does tests/options_check/options_check.cpp on its own.
//
// A new option is one member of Options (with its default and the reason for it) and one row of kOptionRows.
// An entry point of the library takes ONE options_snapshot() when it is called and reads nothing but that copy: a call sees one
// consistent set whatever other threads set meanwhile.
#pragma once
#include <limits.h>
#include <string.h>

#include <mutex>

namespace gsr {

struct Options {
    // prepare in backward: up to this many Gaussians the per-Gaussian backward kernel also counts the digits of the next depth sort
    // (saves that sort's histogram launch: ~7 us + a launch gap on small models); above, its ~2 global adds per key cost more inside
    // the HBM-bound kernel than the histogram kernel does on its own (1 M: +20 us against -8 us).  Both sides of the hand-over
    // evaluate the same predicate on N (prep_counts_digits): the backward that fills a prepared buffer and the forward that consumes
    // it, each on its own snapshot -- do not change the option between the two.
    int prep_hist_max_n = 262144;
    bool prep_counts_digits(int N) const { return N <= prep_hist_max_n; }
    // smallest N for which a forward with its own preprocess sorts depths in three 9-bit passes (0 = only above prep_hist_max_n).
    // Measured (same-box A/B, tools/ab_130k.sh): depth sort 53 -> 45 us at 130 k, 44 -> 37 us at 20 k
    int small_sort9 = 1;
    // bound of gsr_forward's busy-wait for R in units of ~50 ns (20 ms); 0 = no polling: hipStreamSynchronize at once
    int poll_iters = 400000;
    // 1: k_emit counts the tile sort's digits (no histogram launch); 0: k_radix_ghist
    int emit_hist = 1;
    // R-dependent stages launched against a capacity (the caller's hint), R read back late; 0 = read R, then launch
    int speculative_binning = 1;
    // 1: the blend backward accumulates per Gaussian in a fixed order (debug; slower)
    int deterministic_backward = 0;
    // workgroups a long tile's backward is split over (checkpoints from the forward); 1 = off; 0 = auto: 16 on a
    // 980x545 frame, fewer the more tiles there are (the parts that find nothing to do still cost a launch slot:
    // 16 x 17 408 workgroups for eight batched images spent 170 of 860 us on them) -- about 35 000 workgroups
    int bwd_split = 0;
    // 128-instance batches of a tile before the forward starts leaving checkpoints
    int ckpt_first = 1;
    // depth sort of large models in three 9-bit passes over (key - near-plane bits) (radix_sort.h); 0 = four 8-bit passes
    int depth_sort9 = 1;
    // round 5: no global depth sort in front of the direct binning -- every tile's pairs are sorted by depth where they lie (k_tile_sort).
    // 0 = off (depth sort + direct binning), 1 = where it wins: tile lists of up to tile_sort_max_avg pairs on average (by the caller's
    // last R, or 4 N before there is one), 2 = wherever the direct binning runs
    int tile_sort = 1;
    // behind the emit path (batched renders, frames above 4 096 tiles): models of up to this many Gaussians (no name sets it)
    int tile_sort_emit_max_n = 400000;
    // measured (tools/ab_tile_sort*.sh, 980x545): 20 k ... 300 k Gaussians (50 ... 620 pairs per tile) -3 ... -6 % of the step,
    // 1 M (2 070 per tile) +6 %: the per-tile sorts move R pairs where the depth sort moves N keys
    int tile_sort_max_avg = 700;
    // tile lists by direct placement (k_chunk_counts / k_chunk_scatter) instead of emit + tile sort + ranges; 0 = the sort route
    int direct_binning = 1;
    // balanced placement without a view id: a render belongs to the cached view whose pose is within this (x 1e-6) in every matrix entry
    int view_pose_tol_e6 = 2000;
    // round 6: tile lists written only up to where the tiles stopped at the frame's previous render (ListCut); 0 = full lists,
    // 1 = for models of at least list_cut_min_n Gaussians (where it was measured to pay), 2 = wherever the route allows
    int list_cut = 1;
    int list_cut_min_n = 2000000;
    // ... x (1 + this / 1000) of the depth its waves reached
    int list_cut_margin_e3 = 50;
    // tiles whose own cut may lie behind the frame's (served by cut_chunk_tiles)
    int list_cut_deep = 8;
    // the host learns R from the preprocess's per-block shares (published by the depth sort's histogram kernel) instead of from the scan
    int early_r = 1;
    // forward blend: place the waves by the visits each took at the previous render of the same view (balance_build)
    int blend_balance = 1;
};

// what a settable name does with a value outside [lo, hi]
enum class Outside {
    Refuse,         // nothing is stored
    StoreNonZero,   // value != 0 (a switch: lo = 0, hi = 1)
    StoreDefault,   // the member's default, from Options{}
    ClampToLo,
};
struct OptionRow { const char* name; int Options::*member; int lo, hi; Outside outside; };

inline constexpr OptionRow kOptionRows[] = {
    {"bwd_split", &Options::bwd_split, 0, 64, Outside::Refuse},
    {"ckpt_first", &Options::ckpt_first, 1, 64, Outside::Refuse},
    {"tile_sort", &Options::tile_sort, 0, 2, Outside::Refuse},
    {"tile_sort_max_avg", &Options::tile_sort_max_avg, 0, INT_MAX, Outside::Refuse},
    {"view_pose_tol_e6", &Options::view_pose_tol_e6, 0, INT_MAX, Outside::Refuse},
    {"small_sort9", &Options::small_sort9, 0, INT_MAX, Outside::Refuse},
    {"prep_hist_max_n", &Options::prep_hist_max_n, INT_MIN, INT_MAX, Outside::Refuse},
    {"list_cut", &Options::list_cut, 0, 2, Outside::StoreDefault},
    {"list_cut_min_n", &Options::list_cut_min_n, 0, INT_MAX, Outside::StoreDefault},
    {"list_cut_margin_e3", &Options::list_cut_margin_e3, 0, INT_MAX, Outside::StoreDefault},
    {"list_cut_deep", &Options::list_cut_deep, 0, INT_MAX, Outside::StoreDefault},
    {"poll_iters", &Options::poll_iters, 0, INT_MAX, Outside::ClampToLo},
    {"blend_balance", &Options::blend_balance, 0, 1, Outside::StoreNonZero},
    {"early_r", &Options::early_r, 0, 1, Outside::StoreNonZero},
    {"depth_sort9", &Options::depth_sort9, 0, 1, Outside::StoreNonZero},
    {"direct_binning", &Options::direct_binning, 0, 1, Outside::StoreNonZero},
    {"speculative_binning", &Options::speculative_binning, 0, 1, Outside::StoreNonZero},
    {"emit_hist", &Options::emit_hist, 0, 1, Outside::StoreNonZero},
    {"deterministic_backward", &Options::deterministic_backward, 0, 1, Outside::StoreNonZero},
};

// Names whose alternatives have left the tree (DESIGN_HISTORY.md).  They stay for callers that pass them through: the values that
// selected what is now the only code path are accepted and set nothing, every other value is refused.
struct RetiredRow { const char* name; bool any; int a, b; };   // accepted: a or b, or (any) every value
inline constexpr RetiredRow kRetiredRows[] = {
    {"blend_fwd_ppt", false, 0, 7},   // one wave per 8x8 sub-tile with reach bits, the only forward blend (6, the same without the bits, and the
                                      // tile-per-workgroup A/B kernels of rounds 1-4, values 1-5, are gone)
    {"tile_map", false, 2, 2},        // 2x2 tile blocks dealt to the XCDs: the only map (blend_common.h)
    {"sort_algo", false, 2, 2},       // onesweep, the only sort
    {"blend_bwd_ppt", false, 0, 2},   // the packed two-pixel kernel, the only backward blend
    {"ab_variants", true, 0, 0},      // query kept for callers of the round-4 ABI: no A/B kernels in the library
};

inline std::mutex g_options_mutex;
inline Options g_options;   // guarded by g_options_mutex

enum class SetResult { Stored, Refused, Unknown };   // Unknown: neither table has the name (the caller may know it as an action)

inline SetResult options_set(const char* name, int value)
{
    for (const OptionRow& r : kOptionRows) {
        if (strcmp(name, r.name)) continue;
        if (value < r.lo || value > r.hi) {
            switch (r.outside) {
                case Outside::Refuse: return SetResult::Refused;
                case Outside::StoreNonZero: value = value != 0; break;
                case Outside::StoreDefault: value = Options{}.*r.member; break;
                case Outside::ClampToLo: value = r.lo; break;
            }
        }
        std::lock_guard<std::mutex> lk(g_options_mutex);
        g_options.*r.member = value;
        return SetResult::Stored;
    }
    for (const RetiredRow& r : kRetiredRows)
        if (!strcmp(name, r.name)) return (r.any || value == r.a || value == r.b) ? SetResult::Stored : SetResult::Refused;
    return SetResult::Unknown;
}

inline Options options_snapshot()
{
    std::lock_guard<std::mutex> lk(g_options_mutex);
    return g_options;
}

}  // namespace gsr
