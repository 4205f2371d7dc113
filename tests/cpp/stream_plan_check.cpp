// stream_plan.hpp on the host: the queue plans of the streaming pipeline's two clients (tests/test_stream_plan.py).
// Pins derived by hand from the rules as they stood inside the launch path, then the invariants over a grid of inputs.
// Plain g++, no HIP.  Prints "pins N ok", "frame plans N ok", "radiance plans N ok"; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "stream_plan.hpp"

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

constexpr uint64_t GiB = uint64_t(1) << 30;

int pin_frame(int n_pass, uint64_t nps, uint64_t budget, int lanes, int batch, uint64_t bpn, int e_batch, int e_launch, int e_lanes) {
    const FramePlan f = plan_frame_batches(n_pass, nps, bpn, budget, lanes, batch);
    CHECK(f.batch == e_batch && f.n_launch == e_launch && f.lanes == e_lanes, "frame n_pass %d nodes %llu: {%d, %d, %d}, expected {%d, %d, %d}",
          n_pass, (unsigned long long)nps, f.batch, f.n_launch, f.lanes, e_batch, e_launch, e_lanes);
    return 1;
}

int pins() {
    int n = 0;
    n += pin_frame(16, 1000000, GiB, 4, 0, 120, 4, 4, 2);
    n += pin_frame(16, 5000000, GiB, 4, 0, 120, 1, 16, 1);
    n += pin_frame(16, uint64_t(1) << 31, 256 * GiB, 4, 0, 1, 1, 16, 4);          // the 0xF0000000 node bound, not the budget
    for (uint64_t nps : {uint64_t(1), uint64_t(1000000), uint64_t(1) << 40})       // one sample: whatever it costs
        for (uint64_t budget : {GiB, 256 * GiB}) n += pin_frame(1, nps, budget, 4, 0, 120, 1, 1, 1);
    n += pin_frame(5, 1000, GiB, 2, 2, 120, 2, 3, 2);
    {
        const RadiancePlan r = plan_radiance_chunks(uint64_t(1) << 20, 400, 120, GiB, 4);
        CHECK(r.chunk == 4096 && r.nodes == 1642496 && r.n_chunks == 256 && r.lanes == 4, "radiance 2^20 x 400: {%llu, %llu, %llu, %d}",
              (unsigned long long)r.chunk, (unsigned long long)r.nodes, (unsigned long long)r.n_chunks, r.lanes);
        n += 1;
    }
    {
        const RadiancePlan r = plan_radiance_chunks(100, 3, 120, 96 * GiB, 4);
        CHECK(r.chunk == 128 && r.nodes == 4480 && r.n_chunks == 1 && r.lanes == 1, "radiance 100 x 3: {%llu, %llu, %llu, %d}",
              (unsigned long long)r.chunk, (unsigned long long)r.nodes, (unsigned long long)r.n_chunks, r.lanes);
        n += 1;
    }
    {
        const RadiancePlan r = plan_radiance_chunks((uint64_t(1) << 22) + 1, 3, 120, 96 * GiB, 4);
        CHECK(r.chunk == (uint64_t(1) << 22) && r.n_chunks == 2 && r.lanes == 2, "radiance 2^22 + 1: {%llu, %llu, %llu, %d}",
              (unsigned long long)r.chunk, (unsigned long long)r.nodes, (unsigned long long)r.n_chunks, r.lanes);
        n += 1;
    }
    // the formula the ~120 B stand for: 48 + 32 + 4 + (32 + 4 + 8 * lights) / 2 + 1
    CHECK(stream_bytes_per_node(48, 32, 32, 8, 0) == 107 && stream_bytes_per_node(48, 32, 32, 8, 1) == 107 &&
          stream_bytes_per_node(48, 32, 32, 8, 4) == 119 && stream_bytes_per_node(48, 32, 32, 8, 5) == 123, "bytes per node");
    return n + 1;
}

const uint64_t kBudgets[] = {GiB, 3 * GiB, 96 * GiB, 256 * GiB};
const uint64_t kNodeBytes[] = {1, 107, 120, 1131};

int frame_invariants() {
    int n = 0;
    const int passes[] = {1, 2, 3, 5, 16, 128, 4096};
    // nodes of one sample: from a 64-pixel frame to more than one launch may hold
    const uint64_t nodes[] = {4096 + 192, 1000, 1000000, 5000000, 400000000, 0xF0000000ull, uint64_t(1) << 32, uint64_t(1) << 40};
    for (int n_pass : passes) for (uint64_t nps : nodes) for (uint64_t bpn : kNodeBytes) for (uint64_t budget : kBudgets)
        for (int lanes = 1; lanes <= 8; ++lanes) for (int batch : {0, 1, 7}) {
            const FramePlan f = plan_frame_batches(n_pass, nps, bpn, budget, lanes, batch);
            const uint64_t launch_nodes = nps * uint64_t(f.batch);
            CHECK(f.batch >= 1 && f.lanes >= 1 && f.lanes <= lanes, "n_pass %d nodes %llu bpn %llu budget %llu lanes %d batch %d: {%d, %d, %d}",
                  n_pass, (unsigned long long)nps, (unsigned long long)bpn, (unsigned long long)budget, lanes, batch, f.batch, f.n_launch, f.lanes);
            CHECK(int64_t(f.n_launch) * f.batch >= n_pass && n_pass > int64_t(f.n_launch - 1) * f.batch, "n_pass %d: batch %d n_launch %d", n_pass, f.batch, f.n_launch);
            CHECK(launch_nodes <= kStreamNodeBound || f.batch == 1, "nodes %llu batch %d", (unsigned long long)nps, f.batch);
            CHECK(launch_nodes * bpn * uint64_t(f.lanes) <= budget || (f.batch == 1 && f.lanes == 1), "nodes %llu bpn %llu budget %llu: batch %d lanes %d",
                  (unsigned long long)nps, (unsigned long long)bpn, (unsigned long long)budget, f.batch, f.lanes);
            n += 1;
        }
    return n;
}

int radiance_invariants() {
    int n = 0;
    const uint64_t rays[] = {1, 63, 64, 65, 100, 10000, (uint64_t(1) << 20) - 1, uint64_t(1) << 22, (uint64_t(1) << 22) + 1, uint64_t(1) << 32, uint64_t(1) << 38};
    for (uint64_t nr : rays) for (uint64_t factor : {uint64_t(1), uint64_t(3), uint64_t(8), uint64_t(400)}) for (uint64_t bpn : kNodeBytes)
        for (uint64_t budget : kBudgets) for (int lanes = 1; lanes <= 8; ++lanes) {
            const RadiancePlan r = plan_radiance_chunks(nr, factor, bpn, budget, lanes);
            CHECK(r.chunk % 64 == 0 && r.chunk >= 64 && r.chunk <= kRadianceChunkRays, "n %llu: chunk %llu", (unsigned long long)nr, (unsigned long long)r.chunk);
            CHECK(r.n_chunks * r.chunk >= nr && (r.n_chunks - 1) * r.chunk < nr, "n %llu: chunk %llu n_chunks %llu", (unsigned long long)nr,
                  (unsigned long long)r.chunk, (unsigned long long)r.n_chunks);
            CHECK(r.nodes == r.chunk * factor + 4096 && r.nodes <= kStreamNodeBound, "n %llu factor %llu: nodes %llu", (unsigned long long)nr,
                  (unsigned long long)factor, (unsigned long long)r.nodes);
            CHECK(r.lanes >= 1 && r.lanes <= lanes && uint64_t(r.lanes) <= r.n_chunks, "n %llu: lanes %d of %d", (unsigned long long)nr, r.lanes, lanes);
            CHECK(r.nodes * bpn * uint64_t(r.lanes) <= budget || (r.chunk == 64 && r.lanes == 1), "n %llu factor %llu bpn %llu budget %llu: chunk %llu lanes %d",
                  (unsigned long long)nr, (unsigned long long)factor, (unsigned long long)bpn, (unsigned long long)budget, (unsigned long long)r.chunk, r.lanes);
            n += 1;
        }
    return n;
}

}  // namespace

int main() {
    const int np = pins();
    if (!g_failed) std::printf("pins %d ok\n", np);
    const int nf = frame_invariants();
    if (!g_failed) std::printf("frame plans %d ok\n", nf);
    const int nr = radiance_invariants();
    if (!g_failed) std::printf("radiance plans %d ok\n", nr);
    return g_failed ? 1 : 0;
}
