// stage_plan.hpp on the host: the layout of a host variant's staging buffer (tests/test_cpp_stage_plan.py).  Layouts worked out by
// hand: the planes of rtk_temporal_accumulate at 37x19 with everything present and with the noise planes, the mesh planes and the
// whole history absent in turn, and at 5x3; the g-buffer of two 5x3 views with each single plane and with all eight, and of one
// 37x19 view; byte planes of 1, 4, 5 and 257 bytes; a present plane of size zero; nothing present.  Invariants over a grid of sizes
// and presence masks.  Sums that stay exact at 2^31 pixels, and sums that leave 64 bits or a size_t, which are refused and never
// wrapped.  Plain g++, no HIP.  Prints "temporal ok", "gbuffer ok", "bytes ok", "empty ok", "grid ok", "large ok", "all ok"; any
// failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "gbuffer_plan.hpp"
#include "stage_plan.hpp"

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

constexpr uint64_t X = kStageAbsent;

// the layout has exactly these offsets (X: absent) and this total
void expect(const StageLayout &L, const uint64_t *off, int n, uint64_t total, const char *what) {
    CHECK(L.n == n && L.total == total && L.fits(), "%s: n %d total %llu", what, L.n, (unsigned long long)L.total);
    for (int i = 0; i < n && i < L.n; ++i) {
        CHECK(L.off[i] == off[i], "%s: plane %d at %llu, not %llu", what, i, (unsigned long long)L.off[i], (unsigned long long)off[i]);
        CHECK(L.present(i) == (off[i] != X), "%s: plane %d presence", what, i);
    }
}

// as api_temporal.hip lays a call out: 6 planes of the frame, 7 of the history, 3 outputs
StageLayout temporal(uint64_t n, bool noise, bool mesh, bool history) {
    const uint64_t each[13] = {3, 1, 3, 3, 1, 1, 3, 1, 1, 3, 3, 1, 1};
    StageLayout L;
    for (int i = 0; i < 13; ++i) {
        const bool is_noise = i == 1 || i == 7, is_mesh = i == 5 || i == 12;
        L.add(each[i] * n, (i < 6 || history) && (noise || !is_noise) && (mesh || !is_mesh));
    }
    L.add(3 * n); L.add(n, noise); L.add(n);
    return L;
}

void temporal_layouts() {
    const int before = g_failed;
    static_assert(kStageAlign == 256 && kStageAlignWords == 64 && kStageMaxPlanes >= 16, "the pins below are for 256 bytes");
    // 37 x 19 = 703 pixels: a plane of n words takes 704, one of 3n = 2109 words takes 2112
    const uint64_t all[16] = {0, 2112, 2816, 4928, 7040, 7744, 8448, 10560, 11264, 11968, 14080, 16192, 16896, 17600, 19712, 20416};
    expect(temporal(703, true, true, true), all, 16, 21120, "temporal 37x19");
    const uint64_t no_noise[16] = {0, X, 2112, 4224, 6336, 7040, 7744, X, 9856, 10560, 12672, 14784, 15488, 16192, X, 18304};
    expect(temporal(703, false, true, true), no_noise, 16, 19008, "temporal without noise");
    const uint64_t no_mesh[16] = {0, 2112, 2816, 4928, 7040, X, 7744, 9856, 10560, 11264, 13376, 15488, X, 16192, 18304, 19008};
    expect(temporal(703, true, false, true), no_mesh, 16, 19712, "temporal without mesh");
    const uint64_t no_history[16] = {0, 2112, 2816, 4928, 7040, 7744, X, X, X, X, X, X, X, 8448, 10560, 11264};
    expect(temporal(703, true, true, false), no_history, 16, 11968, "temporal without history");
    // 5 x 3 = 15 pixels: every plane fits one unit of 64 words
    uint64_t small[16];
    for (int i = 0; i < 16; ++i) small[i] = uint64_t(i) * 64;
    expect(temporal(15, true, true, true), small, 16, 1024, "temporal 5x3");
    const StageLayout L = temporal(703, true, true, true);
    CHECK(L.bytes[0] == 2109u * 4 && L.bytes[1] == 703u * 4 && L.bytes[15] == 703u * 4, "a copy moves the plane, not its padding");
    if (g_failed == before) std::printf("temporal ok\n");
}

StageLayout gbuffer(uint32_t mask, uint64_t views, uint32_t w, uint32_t h) {
    StageLayout L;
    for (int i = 0; i < kGbPlanes; ++i) L.add(gbuffer_plane_elems(i, views, w, h), (mask >> i & 1u) != 0u);
    return L;
}

void gbuffer_layouts() {
    const int before = g_failed;
    // two views of 5 x 3: 30, 90, 90, 90, 60, 30, 30, 30 words -> 64, 128, 128, 128, 64, 64, 64, 64
    const uint64_t padded[kGbPlanes] = {64, 128, 128, 128, 64, 64, 64, 64};
    const uint64_t all[kGbPlanes] = {0, 64, 192, 320, 448, 512, 576, 640};
    expect(gbuffer(kGbAllPlanes, 2, 5, 3), all, kGbPlanes, 704, "g-buffer, all planes");
    for (int i = 0; i < kGbPlanes; ++i) {
        uint64_t one[kGbPlanes];
        for (int k = 0; k < kGbPlanes; ++k) one[k] = k == i ? 0 : X;
        expect(gbuffer(1u << i, 2, 5, 3), one, kGbPlanes, padded[i], "g-buffer, one plane");
    }
    // one view of 37 x 19: 703, 2109, 2109, 2109, 1406, 703, 703, 703 words -> 704, 2112, 2112, 2112, 1408, 704, 704, 704
    const uint64_t big[kGbPlanes] = {0, 704, 2816, 4928, 7040, 8448, 9152, 9856};
    expect(gbuffer(kGbAllPlanes, 1, 37, 19), big, kGbPlanes, 10560, "g-buffer 37x19");
    if (g_failed == before) std::printf("gbuffer ok\n");
}

void byte_planes() {
    const int before = g_failed;
    const uint64_t sizes[4] = {1, 4, 5, 257}, words[4] = {64, 64, 64, 128};
    for (int i = 0; i < 4; ++i) {
        StageLayout L;
        const int a = L.add_bytes(sizes[i]), b = L.add(1);
        CHECK(a == 0 && b == 1 && L.off[0] == 0 && L.bytes[0] == sizes[i], "%llu bytes: the copy moves exactly them", (unsigned long long)sizes[i]);
        CHECK(L.off[1] == words[i] && L.total == words[i] + 64 && L.fits(), "%llu bytes take whole words: next plane at %llu",
              (unsigned long long)sizes[i], (unsigned long long)L.off[1]);
    }
    if (g_failed == before) std::printf("bytes ok\n");
}

void empty_planes() {
    const int before = g_failed;
    StageLayout none;
    CHECK(none.n == 0 && none.total == 0 && none.fits() && !none.present(0) && !none.present(-1), "no plane at all");
    StageLayout absent;
    absent.add(100, false); absent.add_bytes(7, false);
    CHECK(absent.n == 2 && absent.total == 0 && absent.fits() && !absent.present(0) && !absent.present(1), "nothing present");
    CHECK(absent.off[0] == X && absent.bytes[0] == 0 && absent.off[1] == X && absent.bytes[1] == 0, "an absent plane has no offset and no bytes");
    StageLayout zero;
    const int z = zero.add(0), next = zero.add(1);
    CHECK(zero.present(z) && zero.off[z] == 0 && zero.bytes[z] == 0, "a present plane of size zero has an offset");
    CHECK(zero.off[next] == 0 && zero.total == 64, "... and takes no room");
    if (g_failed == before) std::printf("empty ok\n");
}

void grid() {
    const int before = g_failed;
    const uint64_t sizes[] = {0, 1, 63, 64, 65, 127, 128, 703, 2109, 2520, 7560, 65535, 65536, 65537};
    const int n_sizes = int(sizeof(sizes) / sizeof(sizes[0]));
    uint32_t rng = 12345u;
    for (int planes = 1; planes <= kStageMaxPlanes; planes += 5) {
        for (uint32_t mask = 0; mask < (1u << 6); ++mask) {            // the mask repeats every six planes
            StageLayout L;
            uint64_t want[kStageMaxPlanes], bytes[kStageMaxPlanes], sum = 0;
            for (int i = 0; i < planes; ++i) {
                rng = rng * 1664525u + 1013904223u;
                const bool present = (mask >> (i % 6) & 1u) != 0u, as_bytes = (rng >> 20 & 1u) != 0u;
                want[i] = sizes[(rng >> 8) % uint32_t(n_sizes)];
                bytes[i] = as_bytes ? want[i] : want[i] * 4;
                const int at = as_bytes ? L.add_bytes(want[i], present) : L.add(want[i], present);
                CHECK(at == i, "plane %d got index %d", i, at);
                if (present) sum += (bytes[i] + 3) / 4;
            }
            CHECK(L.fits() && L.n == planes, "mask %u planes %d", mask, planes);
            CHECK(L.total >= sum && L.total % kStageAlignWords == 0, "the total holds every plane: %llu < %llu", (unsigned long long)L.total, (unsigned long long)sum);
            uint64_t end = 0;                                           // planes come in order: each begins at or behind the previous one's end
            for (int i = 0; i < planes; ++i) {
                const bool present = (mask >> (i % 6) & 1u) != 0u;
                CHECK(L.present(i) == present, "plane %d presence", i);
                if (!present) { CHECK(L.off[i] == X && L.bytes[i] == 0, "absent plane %d is null and empty", i); continue; }
                CHECK(L.off[i] % kStageAlignWords == 0 && (uint64_t(0x7f0000000000) + L.off[i] * 4) % kStageAlign == 0, "plane %d is aligned", i);
                CHECK(L.off[i] >= end, "plane %d at %llu overlaps what ends at %llu", i, (unsigned long long)L.off[i], (unsigned long long)end);
                CHECK(L.bytes[i] == bytes[i], "plane %d bytes", i);
                end = L.off[i] + (bytes[i] + 3) / 4;
            }
            CHECK(end <= L.total, "the last plane ends inside the buffer");
            // an absent plane takes no room: the layout of the present ones alone has the same total
            StageLayout P;
            for (int i = 0; i < planes; ++i)
                if (L.present(i)) P.add_bytes(bytes[i]);
            CHECK(P.total == L.total, "absent planes take room: %llu vs %llu", (unsigned long long)L.total, (unsigned long long)P.total);
        }
    }
    if (g_failed == before) std::printf("grid ok\n");
}

void large() {
    const int before = g_failed;
    const uint64_t px = uint64_t(1) << 31;
    // a full g-buffer of 2^31 pixels: every plane is a multiple of the alignment already, so the offsets are the plain prefix sums
    const uint64_t off[kGbPlanes] = {0, px, 4 * px, 7 * px, 10 * px, 12 * px, 13 * px, 14 * px};
    expect(gbuffer(kGbAllPlanes, 1, 65536, 32768), off, kGbPlanes, 15 * px, "g-buffer of 2^31 pixels");
    StageLayout L;
    L.add(17 * px); L.add(17 * px + 1); L.add(3);
    CHECK(L.off[1] == 17 * px && L.off[2] == 34 * px + 64 && L.total == 34 * px + 128 && L.fits(), "17 words per pixel at 2^31 pixels, exactly");
    CHECK(L.bytes[1] == 68 * px + 4, "bytes past 2^32: %llu", (unsigned long long)L.bytes[1]);
    // sums that leave 64 bits are refused, whichever plane does it, and stay refused
    StageLayout a;
    a.add(uint64_t(1) << 62);
    CHECK(!a.fits() && !a.present(0), "2^62 words are 2^64 bytes");
    StageLayout b;
    b.add(kStageAbsent);
    CHECK(!b.fits(), "the largest word count");
    StageLayout c;
    c.add_bytes(kStageAbsent); c.add(1);
    CHECK(!c.fits() && !c.present(1), "the largest byte count; nothing is laid out behind a refusal");
    StageLayout d;
    d.add(uint64_t(1) << 61);
    CHECK(d.fits() == (sizeof(size_t) >= 8) && d.total == uint64_t(1) << 61, "2^63 bytes are a size_t of 64 bits");
    d.add(uint64_t(1) << 61);
    CHECK(!d.fits() && d.total == uint64_t(1) << 61, "two of them are not; the total is not wrapped");
    StageLayout e;
    e.add((uint64_t(1) << 62) - 64); e.add(1);
    CHECK(!e.fits(), "the padding of the last plane counts");
    // one plane more than the capacity
    StageLayout f;
    for (int i = 0; i < kStageMaxPlanes; ++i) f.add(1);
    CHECK(f.fits() && f.n == kStageMaxPlanes && f.total == uint64_t(kStageMaxPlanes) * 64, "a full table");
    const int over = f.add(1);
    CHECK(!f.fits() && f.n == kStageMaxPlanes && over == kStageMaxPlanes - 1, "a plane too many is refused, not written");
    if (g_failed == before) std::printf("large ok\n");
}

}  // namespace

int main() {
    temporal_layouts();
    gbuffer_layouts();
    byte_planes();
    empty_planes();
    grid();
    large();
    if (g_failed != 0) { std::printf("%d check(s) FAILED\n", g_failed); return 1; }
    std::printf("all ok\n");
    return 0;
}
