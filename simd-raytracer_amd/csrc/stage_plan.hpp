// Layout of a host variant's staging buffer (host_stage.hpp): the planes a call moves up or down, one behind the other in ONE buffer
// of 4-byte words.  An absent plane takes no room and has no offset; every present plane begins at a multiple of kStageAlign.
// Plain 64-bit integers, no HIP, no accel: tests/cpp/stage_plan_check.cpp runs it.
#pragma once

#include <cstddef>
#include <cstdint>

namespace rtk {

// Bytes every staged plane is aligned to: what hipMalloc itself guarantees, so a plane of the stage is as well aligned as a plane the
// caller allocated for the _device variant (k_intersect stores its hits as float4; the _device variants ask for 4 or 16 bytes).
constexpr uint64_t kStageAlign = 256;
constexpr uint64_t kStageAlignWords = kStageAlign / 4;
constexpr int kStageMaxPlanes = 16;                           // the most any call stages: rtk_temporal_accumulate, 13 inputs + 3 outputs
constexpr uint64_t kStageAbsent = ~uint64_t(0);

struct StageLayout {
    uint64_t off[kStageMaxPlanes];                            // words from the buffer's base; kStageAbsent for an absent plane
    uint64_t bytes[kStageMaxPlanes];                          // what a copy of the plane moves (0 for an absent plane)
    int n = 0;
    uint64_t total = 0;                                       // words of the buffer: where the next plane would begin
    bool wrapped = false;                                     // a sum left 64 bits (total is then meaningless, fits() false)

    // -> the plane's index.  `words`: the plane's size.  A present plane of size 0 has an offset and takes no room.
    int add(uint64_t words, bool present = true) { return add_bytes(words <= kStageAbsent / 4 ? words * 4 : kStageAbsent, present); }
    // the same for a plane of single bytes (the answers of rtk_accel_occluded): it takes whole words, the copy moves `b` bytes
    int add_bytes(uint64_t b, bool present = true) {
        static_assert(kStageMaxPlanes >= 16 && kStageAlign % 4 == 0, "temporal stages 16 planes; offsets are whole words");
        if (n == kStageMaxPlanes) { wrapped = true; return n - 1; }         // (one plane too many is a bug of the caller's: refused, nothing written)
        const int i = n++;
        off[i] = kStageAbsent; bytes[i] = 0;
        if (!present) return i;
        const uint64_t words = b / 4 + (b % 4 != 0), units = words / kStageAlignWords + (words % kStageAlignWords != 0);
        if (wrapped || units > (kStageAbsent / 4 - total) / kStageAlignWords) { wrapped = true; return i; }
        off[i] = total; bytes[i] = b;
        total += units * kStageAlignWords;
        return i;
    }
    bool present(int i) const { return i >= 0 && i < n && off[i] != kStageAbsent; }
    // whether the buffer's byte count is a size_t: a layout that does not fit is refused like an allocation that cannot succeed
    bool fits() const { return !wrapped && total <= uint64_t(SIZE_MAX) / 4; }
};

}  // namespace rtk
