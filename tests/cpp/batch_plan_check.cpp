// batch_plan.hpp on the host: what a ray batch's size, mode and knobs make of it, and what the probe's verdict words turn into
// (tests/test_cpp_batch_plan.py).  No parity test sees these -- they change the order rays are walked in and nothing else -- so
// they are pinned here to what the rules gave while they stood inline in intersect_device_impl.  Plain g++, no HIP.  Prints one
// "... ok" line per group; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "batch_plan.hpp"

using namespace rtk;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s (line %d): ", #cond, __LINE__);           \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            if (++g_failed > 20) std::exit(1);                               \
        }                                                                    \
    } while (0)

const BatchKnobs kDefault = {true, false, 6, 14, -1};
constexpr size_t k18 = size_t(1) << 18, k32 = size_t(1) << 32;
const int kModes[] = {RTK_TRACE_AUTO, RTK_TRACE_LANE, RTK_TRACE_WAVE, RTK_TRACE_REPACK};

void thresholds() {
    struct Row { size_t n; bool big, sortable; };
    const Row rows[] = {{0, false, false}, {1, false, false}, {2, false, true}, {k18 - 1, false, true}, {k18, true, true},
                        {k32 - 1, true, true}, {k32, false, false}, {k32 + 1, false, false}};
    for (const Row &r : rows) {
        for (int mode : kModes) {
            const BatchPlan p = plan_batch(r.n, mode, false, kDefault);
            const bool forced = mode == RTK_TRACE_REPACK;
            CHECK(p.big == r.big && p.sortable == r.sortable && p.forced == forced, "n %zu mode %d", r.n, mode);
            CHECK(p.mode == (forced ? RTK_TRACE_AUTO : mode), "n %zu mode %d -> %d", r.n, mode, p.mode);
            CHECK(p.probe == (mode == RTK_TRACE_AUTO && r.big), "n %zu mode %d probe %d", r.n, mode, int(p.probe));
            CHECK(p.workspace == (p.probe || (forced && r.sortable)), "n %zu mode %d", r.n, mode);
            CHECK(p.keys_ahead == p.probe, "n %zu mode %d", r.n, mode);
            // without a probe a forced batch is sorted on all key bits and walked by RTK_TRACE_AUTO; nothing else is sorted
            const SortPlan s = plan_sort(p, 0u, 0u, kDefault);
            CHECK(s.sort == (forced && r.sortable), "n %zu mode %d", r.n, mode);
            CHECK(s.mode == p.mode && s.sort_from_bit == 0u && s.rebound == s.sort, "n %zu mode %d", r.n, mode);
        }
        // RTK_REPACK=0: never a probe; RTK_TRACE_REPACK still sorts
        BatchKnobs off = kDefault; off.repack = false;
        CHECK(!plan_batch(r.n, RTK_TRACE_AUTO, false, off).workspace, "n %zu", r.n);
        CHECK(plan_batch(r.n, RTK_TRACE_REPACK, false, off).workspace == r.sortable, "n %zu", r.n);
    }
    std::printf("thresholds ok\n");
}

void stats_never_sort() {
    for (size_t n : {size_t(0), size_t(2), k18, size_t(1) << 24, k32 - 1, k32})
        for (int mode : kModes)
            for (uint32_t w16 : {0u, 1u})
                for (uint32_t w17 = 0; w17 <= 6; ++w17) {
                    const BatchPlan p = plan_batch(n, mode, true, kDefault);
                    const SortPlan s = plan_sort(p, w16, w17, kDefault);
                    CHECK(!p.probe && !p.workspace && !s.sort && !s.rebound, "n %zu mode %d", n, mode);
                    CHECK(s.mode == (mode == RTK_TRACE_REPACK ? RTK_TRACE_AUTO : mode), "n %zu mode %d -> %d", n, mode, s.mode);
                }
    std::printf("stats ok\n");
}

void strides() {
    // the probe: about 4,096 waves looked at, never fewer than every 16th; the unprobed sort's bounds: about 4,096, every wave below that
    for (size_t n : {size_t(1), size_t(64), size_t(65), k18, k18 + 1, size_t(1) << 22, (size_t(1) << 22) + 1, size_t(1) << 24,
                     (size_t(1) << 24) + 77, size_t(1) << 28, k32 - 1}) {
        const size_t waves = (n + 63) / 64;
        const uint32_t ps = probe_stride(n), ss = sample_stride(n, false);
        const size_t looked = (waves + ps - 1) / ps, sampled = (waves + ss - 1) / ss;
        CHECK(ps >= 16u, "n %zu stride %u", n, ps);
        CHECK(looked <= 4096, "n %zu looks at %zu waves", n, looked);
        CHECK(ps == 16u || looked > 2048, "n %zu looks at %zu waves", n, looked);        // (a stride one smaller would pass 4,096)
        CHECK(ps == 16u || (waves + ps - 2) / (ps - 1) > 4096, "n %zu stride %u is not the smallest", n, ps);
        CHECK(ss >= 1u && sampled <= 4096 && (ss == 1u || (waves + ss - 2) / (ss - 1) > 4096), "n %zu stride %u", n, ss);
        CHECK(sample_stride(n, true) == 1u, "n %zu", n);
        CHECK(plan_batch(n, RTK_TRACE_AUTO, false, kDefault).probe_stride == ps, "n %zu", n);
        CHECK(plan_batch(n, RTK_TRACE_REPACK, false, kDefault).bounds_stride == ss, "n %zu", n);
    }
    CHECK(probe_stride(k18) == 16u && probe_stride(size_t(1) << 22) == 16u && probe_stride((size_t(1) << 22) + 1) == 17u, "16 until 2^22 rays");
    CHECK(probe_stride(size_t(1) << 24) == 64u && sample_stride(size_t(1) << 24, false) == 64u && sample_stride(k18, false) == 1u, "2^24 rays");
    CHECK(sample_stride(0, false) == 0u, "no waves");                        // launch_ray_bounds takes 0 as 1
    BatchKnobs full = kDefault; full.repack_full_bounds = true;
    const BatchPlan p = plan_batch(size_t(1) << 24, RTK_TRACE_AUTO, false, full);
    const SortPlan s = plan_sort(p, 1u, 2u, full);
    CHECK(p.probe && !p.keys_ahead && s.sort && s.rebound && s.bounds_stride == 1u, "full bounds behind a probe");
    const BatchPlan pf = plan_batch(size_t(1) << 24, RTK_TRACE_REPACK, false, full);
    CHECK(!pf.probe && !pf.keys_ahead && pf.bounds_stride == 1u && plan_sort(pf, 0u, 0u, full).rebound, "full bounds of a forced sort");
    const SortPlan sd = plan_sort(plan_batch(size_t(1) << 24, RTK_TRACE_AUTO, false, kDefault), 1u, 2u, kDefault);
    CHECK(sd.sort && !sd.rebound, "the probe's bounds serve the keys");
    std::printf("strides ok\n");
}

void verdict_table() {
    const size_t n = size_t(1) << 20;
    for (int skip : {0, 14})
        for (int skip2 : {0, 22})
            for (int trace : {-1, int(RTK_TRACE_AUTO), int(RTK_TRACE_LANE), int(RTK_TRACE_WAVE)}) {
                const BatchKnobs k = {true, false, skip, skip2, trace};
                const BatchPlan p = plan_batch(n, RTK_TRACE_AUTO, false, k);
                CHECK(p.probe && p.workspace, "probe");
                for (uint32_t dims = 0; dims <= 6; ++dims) {
                    const SortPlan coherent = plan_sort(p, 0u, dims, k);
                    CHECK(!coherent.sort && !coherent.rebound && coherent.mode == RTK_TRACE_AUTO, "dims %u", dims);
                    const SortPlan s = plan_sort(p, 1u, dims, k);
                    const int by_probe = dims <= 3u ? RTK_TRACE_WAVE : RTK_TRACE_AUTO;
                    const unsigned from = dims <= 2u ? unsigned(skip2) : (dims == 3u ? unsigned(skip) : 0u);
                    CHECK(s.sort && s.sorted_mode == by_probe && s.sort_from_bit == from, "dims %u: mode %d from bit %u", dims, s.sorted_mode, s.sort_from_bit);
                    CHECK(s.mode == (trace >= 0 ? trace : by_probe), "dims %u trace %d -> %d", dims, trace, s.mode);
                    CHECK(s.sort_from_bit < 30u, "dims %u", dims);
                    // a word other than 0 or 1 still says sort
                    CHECK(plan_sort(p, 7u, dims, k).sort, "dims %u", dims);
                }
                // forced: the verdict words are not read
                const BatchPlan f = plan_batch(n, RTK_TRACE_REPACK, false, k);
                for (uint32_t dims = 0; dims <= 6; ++dims) {
                    const SortPlan s = plan_sort(f, 0u, dims, k);
                    CHECK(s.sort && s.sort_from_bit == 0u && s.sorted_mode == RTK_TRACE_AUTO && s.mode == (trace >= 0 ? trace : int(RTK_TRACE_AUTO)), "forced, dims %u", dims);
                }
            }
    std::printf("verdict table ok\n");
}

}  // namespace

int main() {
    thresholds();
    stats_never_sort();
    strides();
    verdict_table();
    if (g_failed) return 1;
    std::printf("all ok\n");
    return 0;
}
