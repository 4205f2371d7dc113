// Host plan of rtk_render_adaptive (api_adaptive.hip): what the call refuses and in which order, the checkpoints at which the 8x8
// pixel blocks of a frame are judged, where a block's pixels sit in the first round's list, how a round's list of active pixels is
// walked in chunks, and the one word the decide kernel counts the next round into.  Plain integers, no HIP, no accel:
// tests/cpp/adaptive_plan_check.cpp runs it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"

namespace rtk {

// Pixels of one chunk at most: rays and colours of a chunk are 36 B per pixel, and a chunk is one radiance batch per sample, which
// likes a few hundred thousand rays at least.  rtk_knobs::adaptive_chunk_pixels (RTK_ADAPTIVE_CHUNK_PIXELS lowers it for a test).
constexpr uint64_t kAdaptiveChunkPixels = uint64_t(1) << 20;
// Pixels of a frame at most: a pixel is its uint32_t frame index in the lists, and the workspace is 24 B per pixel.
constexpr uint64_t kAdaptiveMaxPixels = uint64_t(1) << 31;
constexpr uint32_t kAdWavesPerGroup = 4;                      // k_adaptive_decide: one wave per block, four to a workgroup

// The next round's size as ONE 64-bit word, so that a block reserves its pixels and its slot in the block list with one atomic add
// and the host reads one word per round: pixels in the low 36 bits (<= 2^31), blocks above them (<= 2^25).
constexpr int kAdCountBlockShift = 36;
constexpr uint64_t ad_count_word(uint64_t pixels, uint64_t blocks) { return pixels | (blocks << kAdCountBlockShift); }
constexpr uint64_t ad_count_pixels(uint64_t word) { return word & ((uint64_t(1) << kAdCountBlockShift) - 1u); }
constexpr uint64_t ad_count_blocks(uint64_t word) { return word >> kAdCountBlockShift; }

// What the call refuses once rtk_render_frame's own checks of *p have passed (frame_geom), in the order rtk.h gives; nullptr = the
// call goes on to the device.  width, height: the frame's, as frame_geom resolved them.
inline const char *adaptive_refusal(const rtk_render_params &p, const rtk_adaptive_params &ap, uint32_t width, uint32_t height) {
    if (p.trace_mode != RTK_TRACE_AUTO && p.trace_mode != RTK_TRACE_STREAM)
        return "trace_mode of an adaptive render must be RTK_TRACE_AUTO or RTK_TRACE_STREAM";
    if (p.spp < 2) return "an adaptive render needs spp >= 2 (the ceiling)";
    if (p.sample_begin != 0 || p.sample_count != 0) return "an adaptive render is not progressive: sample_begin and sample_count must be 0";
    if (p.collect_stats != 0) return "an adaptive render collects no per-ray statistics";
    if (p.world_size > 1) return "an adaptive render is not sharded";
    if (ap.min_samples < 2 || ap.min_samples > p.spp) return "min_samples must be in [2, spp]";
    if (ap.step < 1) return "step must be >= 1";
    if (!std::isfinite(ap.threshold) || ap.threshold < 0.0f) return "threshold must be finite and >= 0";
    if (!std::isfinite(ap.floor) || !(ap.floor > 0.0f)) return "floor must be finite and > 0";
    if (uint64_t(width) * height > kAdaptiveMaxPixels) return "too many pixels for an adaptive render";
    return nullptr;
}

// The checkpoints: min_samples, min_samples + step, ... and spp itself as the last one (the last round may be shorter than step).
// `n`: a checkpoint below spp (or 0: no sample taken yet).  64-bit inside: n + step may pass 2^31.
inline int32_t adaptive_next_checkpoint(int32_t n, int32_t spp, int32_t min_samples, int32_t step) {
    if (n < min_samples) return min_samples;
    const int64_t next = int64_t(n) + step;
    return next < spp ? int32_t(next) : spp;
}
// is `n` one of them?
inline bool adaptive_is_checkpoint(int32_t n, int32_t spp, int32_t min_samples, int32_t step) {
    return n == spp || (n >= min_samples && n < spp && (n - min_samples) % step == 0);
}
// how many there are (= rounds a pixel that never converges lives through)
inline uint64_t adaptive_checkpoints(int32_t spp, int32_t min_samples, int32_t step) {
    return uint64_t(int64_t(spp) - min_samples + step - 1) / uint64_t(step) + 1u;
}

// The 8x8 blocks of the frame's own grid, row-major; edge blocks are partial.
inline uint32_t adaptive_blocks_x(uint32_t width) { return (width + 7u) / 8u; }
inline uint64_t adaptive_blocks(uint32_t width, uint32_t height) { return uint64_t(adaptive_blocks_x(width)) * ((height + 7u) / 8u); }
inline uint32_t adaptive_groups(uint64_t blocks) { return uint32_t((blocks + kAdWavesPerGroup - 1u) / kAdWavesPerGroup); }
// The first round's list holds every block in frame order, each with its valid pixels row-major.  All blocks of block row `by` are
// `bh` pixels high and their widths add up to the frame's, so block (bx, by) begins at:
inline uint64_t adaptive_first_offset(uint32_t bx, uint32_t by, uint32_t width, uint32_t height) {
    const uint32_t y0 = by * 8u, bh = height - y0 < 8u ? height - y0 : 8u;
    return uint64_t(y0) * width + uint64_t(bx) * 8u * bh;
}

// The chunk walk of a round: [first, first + n) of the list of `active` pixels, chunk after chunk, every pixel exactly once.
struct AdaptiveChunks {
    uint64_t active, chunk, first = 0;
    AdaptiveChunks(uint64_t active_pixels, uint64_t chunk_pixels) : active(active_pixels), chunk(chunk_pixels < 1u ? 1u : chunk_pixels) {}
    bool done() const { return first >= active; }
    uint32_t n() const { return uint32_t(active - first < chunk ? active - first : chunk); }
    void next() { first += n(); }
    uint64_t count() const { return (active + chunk - 1u) / chunk; }
};
// rays and colours are sized for the largest chunk a frame of `pixels` can have
inline uint64_t adaptive_chunk_capacity(uint64_t pixels, uint64_t chunk_pixels) {
    const uint64_t c = chunk_pixels < 1u ? 1u : chunk_pixels;
    return pixels < c ? pixels : c;
}

}  // namespace rtk
