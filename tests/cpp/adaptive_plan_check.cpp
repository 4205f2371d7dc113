// adaptive_plan.hpp on the host: the plan of rtk_render_adaptive (tests/test_cpp_adaptive_plan.py).  Pins worked out by hand: the
// refusals in rtk.h's order, the checkpoint schedules (step not dividing spp - min, min == spp, step > spp, sums past 2^31), the
// blocks of 70x36, 5x3 and 8x8 frames with the first round's offsets, the chunk walks (every pixel of a round exactly once), and
// the count word.  Plain g++, no HIP.  Prints "refusals ok", "checkpoints ok", "blocks ok", "chunks ok", "count ok", "all ok"; any
// failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "adaptive_plan.hpp"

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

bool has(const char *why, const char *word) { return why != nullptr && std::strstr(why, word) != nullptr; }

rtk_render_params params(int spp) {
    rtk_render_params p;
    std::memset(&p, 0, sizeof(p));
    p.width = 8; p.height = 8; p.spp = spp; p.trace_mode = RTK_TRACE_STREAM;
    return p;
}

void refusals() {
    const int before = g_failed;
    static_assert(sizeof(rtk_adaptive_params) == 16, "two ints and two floats");
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    const rtk_adaptive_params ok = {2, 2, 0.1f, 0.01f};
    rtk_render_params p = params(8);
    CHECK(adaptive_refusal(p, ok, 8, 8) == nullptr, "a valid call");
    p.trace_mode = RTK_TRACE_AUTO;
    CHECK(adaptive_refusal(p, ok, 8, 8) == nullptr, "RTK_TRACE_AUTO");
    const rtk_adaptive_params zero = {2, 1, 0.0f, 1e-30f};
    CHECK(adaptive_refusal(params(2), zero, 1, 1) == nullptr, "threshold 0, min == spp == 2, a 1x1 frame");
    CHECK(adaptive_refusal(p, ok, 65536, 32768) == nullptr, "2^31 pixels");
    // the order: a call wrong in every way from k on reports way k
    rtk_adaptive_params a = ok;
    a.floor = 0.0f;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "floor"), "floor");
    CHECK(has(adaptive_refusal(p, a, 65536, 65536), "floor"), "floor before the pixel count");
    CHECK(has(adaptive_refusal(p, ok, 65536, 32769), "too many pixels"), "the pixel count last");
    a.threshold = -1.0f;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "threshold"), "threshold before floor");
    a.step = 0;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "step"), "step before threshold");
    a.min_samples = 1;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "min_samples"), "min_samples before step");
    p.world_size = 2;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "not sharded"), "world_size before min_samples");
    p.collect_stats = 2;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "statistics"), "collect_stats before world_size");
    p.sample_count = 8;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "not progressive"), "sample_count before collect_stats");
    p.spp = 1;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "spp >= 2"), "spp before the progressive fields");
    p.trace_mode = RTK_TRACE_GROUP4;
    CHECK(has(adaptive_refusal(p, a, 8, 8), "RTK_TRACE_AUTO or RTK_TRACE_STREAM"), "trace_mode first");
    // every form of each
    for (const int m : {RTK_TRACE_LANE, RTK_TRACE_WAVE, RTK_TRACE_GROUP4, RTK_TRACE_GROUP8, RTK_TRACE_GROUP16, RTK_TRACE_TWOPASS}) {
        rtk_render_params q = params(8);
        q.trace_mode = m;
        CHECK(has(adaptive_refusal(q, ok, 8, 8), "RTK_TRACE_AUTO or RTK_TRACE_STREAM"), "mode %d", m);
    }
    rtk_render_params q = params(8);
    q.sample_begin = 1; q.sample_count = 1;
    CHECK(has(adaptive_refusal(q, ok, 8, 8), "not progressive"), "sample_begin");
    for (const int m : {1, 0, -7, 9, std::numeric_limits<int>::min(), std::numeric_limits<int>::max()}) {
        rtk_adaptive_params b = ok;
        b.min_samples = m;
        CHECK(has(adaptive_refusal(params(8), b, 8, 8), "min_samples"), "min_samples %d", m);
    }
    for (const int s : {0, -1, std::numeric_limits<int>::min()}) {
        rtk_adaptive_params b = ok;
        b.step = s;
        CHECK(has(adaptive_refusal(params(8), b, 8, 8), "step"), "step %d", s);
    }
    for (const float t : {-1e-30f, -0.5f, inf, -inf, nan}) {
        rtk_adaptive_params b = ok;
        b.threshold = t;
        CHECK(has(adaptive_refusal(params(8), b, 8, 8), "threshold"), "threshold %g", double(t));
    }
    for (const float f : {0.0f, -0.0f, -1.0f, inf, -inf, nan}) {
        rtk_adaptive_params b = ok;
        b.floor = f;
        CHECK(has(adaptive_refusal(params(8), b, 8, 8), "floor"), "floor %g", double(f));
    }
    rtk_adaptive_params b = ok;
    b.threshold = -0.0f;                                          // -0 >= 0
    CHECK(adaptive_refusal(params(8), b, 8, 8) == nullptr, "threshold -0");
    if (g_failed == before) std::printf("refusals ok\n");
}

std::vector<int32_t> schedule(int32_t spp, int32_t min_samples, int32_t step) {
    std::vector<int32_t> v;
    for (int32_t n = 0; n != spp && v.size() < 100;) {
        n = adaptive_next_checkpoint(n, spp, min_samples, step);
        v.push_back(n);
    }
    return v;
}

void checkpoints() {
    const int before = g_failed;
    const int32_t big = std::numeric_limits<int32_t>::max();
    CHECK((schedule(8, 2, 2) == std::vector<int32_t>{2, 4, 6, 8}), "step divides spp - min");
    CHECK((schedule(9, 2, 3) == std::vector<int32_t>{2, 5, 8, 9}), "step does not divide spp - min: the last round is shorter");
    CHECK((schedule(11, 3, 4) == std::vector<int32_t>{3, 7, 11}), "11, 3, 4");
    CHECK((schedule(4, 4, 1) == std::vector<int32_t>{4}), "min == spp: one round");
    CHECK((schedule(8, 2, 100) == std::vector<int32_t>{2, 8}), "step > spp");
    CHECK((schedule(8, 2, big) == std::vector<int32_t>{2, 8}), "step 2^31 - 1: no overflow");
    CHECK((schedule(big, big - 3, 2) == std::vector<int32_t>{big - 3, big - 1, big}), "spp 2^31 - 1");
    CHECK((schedule(128, 16, 16) == std::vector<int32_t>{16, 32, 48, 64, 80, 96, 112, 128}), "128, 16, 16");
    const struct { int32_t spp, mn, st; } cases[] = {{8, 2, 2}, {9, 2, 3}, {11, 3, 4}, {4, 4, 1}, {8, 2, 100}, {128, 16, 16}, {7, 2, 1}, {2, 2, 5}};
    for (const auto &c : cases) {
        const std::vector<int32_t> s = schedule(c.spp, c.mn, c.st);
        CHECK(s.size() == adaptive_checkpoints(c.spp, c.mn, c.st), "count of (%d, %d, %d): %zu", c.spp, c.mn, c.st, s.size());
        CHECK(s.front() == c.mn && s.back() == c.spp, "ends of (%d, %d, %d)", c.spp, c.mn, c.st);
        size_t at = 0;
        for (int32_t n = 0; n <= c.spp; ++n) {
            const bool is = at < s.size() && s[at] == n;
            CHECK(adaptive_is_checkpoint(n, c.spp, c.mn, c.st) == is, "is_checkpoint(%d) of (%d, %d, %d)", n, c.spp, c.mn, c.st);
            at += is ? 1 : 0;
        }
        for (size_t i = 1; i < s.size(); ++i) CHECK(s[i] > s[i - 1] && s[i] - s[i - 1] <= c.st, "round %zu of (%d, %d, %d)", i, c.spp, c.mn, c.st);
    }
    CHECK(adaptive_checkpoints(big, 2, 1) == uint64_t(big) - 1u, "2^31 - 2 checkpoints");
    if (g_failed == before) std::printf("checkpoints ok\n");
}

void blocks() {
    const int before = g_failed;
    CHECK(adaptive_blocks_x(70) == 9 && adaptive_blocks(70, 36) == 45, "70x36: 9 x 5 blocks");
    CHECK(adaptive_blocks(5, 3) == 1 && adaptive_blocks(8, 8) == 1 && adaptive_blocks(9, 8) == 2 && adaptive_blocks(1, 1) == 1, "small frames");
    CHECK(adaptive_blocks(65536, 32768) == (uint64_t(1) << 25), "2^31 pixels: 2^25 blocks");
    CHECK(adaptive_groups(45) == 12 && adaptive_groups(1) == 1 && adaptive_groups(4) == 1 && adaptive_groups(5) == 2, "workgroups of four waves");
    CHECK(adaptive_groups(uint64_t(1) << 25) == (1u << 23), "groups of the largest frame");
    // the first round's list: the blocks in frame order, each with its valid pixels; the offsets are the running pixel count
    const struct { uint32_t w, h; } frames[] = {{70, 36}, {5, 3}, {8, 8}, {64, 64}, {9, 17}, {1, 1}, {1, 100}, {100, 1}};
    for (const auto &f : frames) {
        uint64_t at = 0;
        const uint32_t bxn = adaptive_blocks_x(f.w), byn = (f.h + 7) / 8;
        for (uint32_t by = 0; by < byn; ++by)
            for (uint32_t bx = 0; bx < bxn; ++bx) {
                CHECK(adaptive_first_offset(bx, by, f.w, f.h) == at, "%ux%u block (%u, %u): %llu, expected %llu", f.w, f.h, bx, by,
                      (unsigned long long)adaptive_first_offset(bx, by, f.w, f.h), (unsigned long long)at);
                const uint32_t bw = f.w - bx * 8 < 8 ? f.w - bx * 8 : 8, bh = f.h - by * 8 < 8 ? f.h - by * 8 : 8;
                at += uint64_t(bw) * bh;
            }
        CHECK(at == uint64_t(f.w) * f.h, "%ux%u: the blocks hold every pixel", f.w, f.h);
    }
    CHECK(adaptive_first_offset(8191, 4095, 65536, 32768) == (uint64_t(1) << 31) - 64, "the last block of the largest frame");
    if (g_failed == before) std::printf("blocks ok\n");
}

void chunks() {
    const int before = g_failed;
    const struct { uint64_t active, chunk; } cases[] = {{2520, 1000}, {2520, 2520}, {2520, 1u << 20}, {15, 1}, {1, 1000}, {2000, 1000},
                                                        {(uint64_t(1) << 31), uint64_t(1) << 20}, {(uint64_t(1) << 31), uint64_t(1) << 30}, {7, 0}};
    for (const auto &c : cases) {
        std::vector<uint8_t> seen(size_t(c.active < 100000 ? c.active : 0), 0);
        uint64_t expect_first = 0, n_chunks = 0;
        const uint64_t eff = c.chunk < 1 ? 1 : c.chunk;
        for (AdaptiveChunks w(c.active, c.chunk); !w.done(); w.next()) {
            CHECK(w.first == expect_first, "chunks begin where the one before ended");
            CHECK(w.n() >= 1 && w.n() <= eff && w.first + w.n() <= c.active, "chunk %llu of (%llu, %llu)", (unsigned long long)n_chunks,
                  (unsigned long long)c.active, (unsigned long long)c.chunk);
            CHECK(w.n() <= adaptive_chunk_capacity(c.active, c.chunk), "a chunk fits the buffers");
            for (uint64_t i = w.first; i < w.first + w.n() && !seen.empty(); ++i) seen[size_t(i)] += 1;
            expect_first += w.n();
            n_chunks += 1;
            if (n_chunks > 4096) break;
        }
        CHECK(expect_first == c.active, "(%llu, %llu): every pixel walked", (unsigned long long)c.active, (unsigned long long)c.chunk);
        CHECK(n_chunks == AdaptiveChunks(c.active, c.chunk).count(), "(%llu, %llu): %llu chunks", (unsigned long long)c.active,
              (unsigned long long)c.chunk, (unsigned long long)n_chunks);
        for (const uint8_t s : seen) CHECK(s == 1, "exactly once");
    }
    CHECK(AdaptiveChunks(0, 1000).done() && AdaptiveChunks(0, 1000).count() == 0, "an empty round has no chunk");
    CHECK(AdaptiveChunks(2520, 1000).count() == 3, "2520 pixels in chunks of 1000");
    CHECK(adaptive_chunk_capacity(2520, 1000) == 1000 && adaptive_chunk_capacity(15, kAdaptiveChunkPixels) == 15 &&
          adaptive_chunk_capacity(uint64_t(1) << 31, kAdaptiveChunkPixels) == kAdaptiveChunkPixels, "buffer sizes");
    if (g_failed == before) std::printf("chunks ok\n");
}

void count_word() {
    const int before = g_failed;
    const uint64_t px = uint64_t(1) << 31, bl = uint64_t(1) << 25;
    CHECK(ad_count_pixels(ad_count_word(px, bl)) == px && ad_count_blocks(ad_count_word(px, bl)) == bl, "the largest frame fits the word");
    // what the kernel adds per block: its pixels and one block
    uint64_t w = 0;
    for (int i = 0; i < 45; ++i) w += ad_count_word(i % 9 == 8 ? 24 : 64, 1);
    CHECK(ad_count_pixels(w) == 40u * 64 + 5u * 24 && ad_count_blocks(w) == 45, "45 blocks added up");
    CHECK(ad_count_word(0, 0) == 0 && ad_count_word(1, 0) == 1 && ad_count_word(0, 1) == (uint64_t(1) << 36), "the fields");
    if (g_failed == before) std::printf("count ok\n");
}

}  // namespace

int main() {
    refusals();
    checkpoints();
    blocks();
    chunks();
    count_word();
    if (g_failed != 0) return 1;
    std::printf("all ok\n");
    return 0;
}
