// Stand-alone check of csrc/options.h (tests/test_abi_cpu.py builds and runs it): the defaults, what every out-of-range rule stores,
// and that a refused call stores nothing -- the half of gsr_set_option's semantics the C ABI cannot show (it has no getter).
// `options_check race`: one thread sets options while two take snapshots, for a run under -fsanitize=thread.
#include "../../3dgs_hierarchical_training_amd/csrc/options.h"

#include <stdio.h>
#include <stdlib.h>

#include <atomic>
#include <thread>

using namespace gsr;

#define CHECK(cond) do { if (!(cond)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); exit(1); } } while (0)

static bool same(const Options& a, const Options& b)
{
    for (const OptionRow& r : kOptionRows)
        if (a.*r.member != b.*r.member) return false;
    return a.tile_sort_emit_max_n == b.tile_sort_emit_max_n;
}

static int get(const char* name)
{
    const Options o = options_snapshot();
    for (const OptionRow& r : kOptionRows)
        if (!strcmp(name, r.name)) return o.*r.member;
    CHECK(!"no such option");
    return 0;
}

static void check_values()
{
    const Options d;
    CHECK(d.bwd_split == 0 && d.ckpt_first == 1 && d.tile_sort == 1 && d.tile_sort_max_avg == 700 && d.tile_sort_emit_max_n == 400000);
    CHECK(d.view_pose_tol_e6 == 2000 && d.small_sort9 == 1 && d.list_cut == 1 && d.list_cut_min_n == 2000000);
    CHECK(d.list_cut_margin_e3 == 50 && d.list_cut_deep == 8 && d.poll_iters == 400000 && d.prep_hist_max_n == 262144);
    CHECK(d.blend_balance == 1 && d.early_r == 1 && d.depth_sort9 == 1 && d.direct_binning == 1 && d.speculative_binning == 1);
    CHECK(d.emit_hist == 1 && d.deterministic_backward == 0);
    CHECK(same(options_snapshot(), d));
    CHECK(d.prep_counts_digits(262144) && !d.prep_counts_digits(262145));

    // refuse: in range is stored, beyond either end is refused and leaves every member as it was
    struct { const char* name; int lo, hi; } refuse[] = {{"bwd_split", 0, 64}, {"ckpt_first", 1, 64}, {"tile_sort", 0, 2},
        {"tile_sort_max_avg", 0, INT_MAX}, {"view_pose_tol_e6", 0, INT_MAX}, {"small_sort9", 0, INT_MAX}};
    for (auto& c : refuse) {
        CHECK(options_set(c.name, c.hi) == SetResult::Stored && get(c.name) == c.hi);
        CHECK(options_set(c.name, c.lo) == SetResult::Stored && get(c.name) == c.lo);
        const Options before = options_snapshot();
        CHECK(options_set(c.name, c.lo - 1) == SetResult::Refused && same(options_snapshot(), before));
        if (c.hi != INT_MAX) CHECK(options_set(c.name, c.hi + 1) == SetResult::Refused && same(options_snapshot(), before));
    }
    for (int v : {INT_MIN, -1, 0, 262144, INT_MAX}) CHECK(options_set("prep_hist_max_n", v) == SetResult::Stored && get("prep_hist_max_n") == v);

    // store the default
    struct { const char* name; int hi, dflt; } dfl[] = {{"list_cut", 2, 1}, {"list_cut_min_n", INT_MAX, 2000000},
        {"list_cut_margin_e3", INT_MAX, 50}, {"list_cut_deep", INT_MAX, 8}};
    for (auto& c : dfl) {
        CHECK(options_set(c.name, 0) == SetResult::Stored && get(c.name) == 0);
        CHECK(options_set(c.name, -1) == SetResult::Stored && get(c.name) == c.dflt);
        CHECK(options_set(c.name, c.hi) == SetResult::Stored && get(c.name) == c.hi);
        CHECK(options_set(c.name, INT_MIN) == SetResult::Stored && get(c.name) == c.dflt);
    }
    CHECK(options_set("list_cut", 0) == SetResult::Stored && options_set("list_cut", 3) == SetResult::Stored && get("list_cut") == 1);

    // store 0
    CHECK(options_set("poll_iters", 7) == SetResult::Stored && get("poll_iters") == 7);
    CHECK(options_set("poll_iters", -1) == SetResult::Stored && get("poll_iters") == 0);
    CHECK(options_set("poll_iters", INT_MAX) == SetResult::Stored && get("poll_iters") == INT_MAX);

    // store value != 0
    for (const char* name : {"blend_balance", "early_r", "depth_sort9", "direct_binning", "speculative_binning", "emit_hist", "deterministic_backward"}) {
        for (int v : {0, 1, 2, -1, INT_MIN, INT_MAX, 0}) CHECK(options_set(name, v) == SetResult::Stored && get(name) == (v != 0));
    }

    // retired names set nothing; neither do unknown ones
    const Options before = options_snapshot();
    CHECK(options_set("blend_fwd_ppt", 0) == SetResult::Stored && options_set("blend_fwd_ppt", 7) == SetResult::Stored);
    CHECK(options_set("blend_fwd_ppt", 6) == SetResult::Refused && options_set("blend_fwd_ppt", -1) == SetResult::Refused);
    CHECK(options_set("tile_map", 2) == SetResult::Stored && options_set("tile_map", 1) == SetResult::Refused && options_set("tile_map", 3) == SetResult::Refused);
    CHECK(options_set("sort_algo", 2) == SetResult::Stored && options_set("sort_algo", 0) == SetResult::Refused && options_set("sort_algo", 3) == SetResult::Refused);
    CHECK(options_set("blend_bwd_ppt", 0) == SetResult::Stored && options_set("blend_bwd_ppt", 2) == SetResult::Stored);
    CHECK(options_set("blend_bwd_ppt", 1) == SetResult::Refused && options_set("blend_bwd_ppt", 3) == SetResult::Refused);
    for (int v : {INT_MIN, -1, 0, 1, INT_MAX}) CHECK(options_set("ab_variants", v) == SetResult::Stored);
    CHECK(options_set("no_such_option", 1) == SetResult::Unknown && options_set("", 0) == SetResult::Unknown);
    CHECK(options_set("tile_sort_emit_max_n", 1) == SetResult::Unknown);   // a member that no name sets
    CHECK(options_set("profile", 1) == SetResult::Unknown);                // an action: the library's own code
    CHECK(same(options_snapshot(), before));

    // every row names its own member, once
    for (const OptionRow& r : kOptionRows) {
        int n = 0;
        for (const OptionRow& q : kOptionRows) n += !strcmp(r.name, q.name) + (r.member == q.member);
        CHECK(n == 2 && r.lo <= r.hi);
        const int dv = d.*r.member;
        CHECK(dv >= r.lo && dv <= r.hi);
    }
}

static void race()
{
    std::atomic<bool> stop{false};
    std::atomic<long long> sum{0};
    auto reader = [&] {
        long long s = 0;
        while (!stop.load(std::memory_order_relaxed)) { const Options o = options_snapshot(); s += o.tile_sort + o.poll_iters + o.list_cut_deep; }
        sum += s;
    };
    std::thread r1(reader), r2(reader);
    for (int i = 0; i < 200000; i++) {
        options_set("tile_sort", i % 3);
        options_set("poll_iters", i);
        options_set("list_cut_deep", i & 15);
        options_set("tile_sort", 9);   // refused
    }
    stop = true;
    r1.join(); r2.join();
    printf("race: done (%lld)\n", sum.load());
}

int main(int argc, char** argv)
{
    if (argc > 1 && !strcmp(argv[1], "race")) { race(); return 0; }
    check_values();
    printf("options_check: ok\n");
    return 0;
}
