// Host plan of rtk_denoise_frame (api_denoise.hip, denoise.hip): what the calls refuse and in which order, which pixels a workgroup
// owns, the halo and the LDS bytes of a tile at a step, which steps are staged in LDS, and the layout of the caller's workspace.
// Plain integers, no HIP: tests/cpp/denoise_plan_check.cpp runs it, and the kernel finds its tile with the same denoise_tile().
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/rtk.h"

#ifndef RTK_DN_FN
#if defined(__HIPCC__)
#define RTK_DN_FN __host__ __device__ inline
#else
#define RTK_DN_FN inline
#endif
#endif

namespace rtk {

constexpr uint64_t kDnMaxImagePixels = uint64_t(1) << 28;    // an image's pixel index and its tile count fit 32 bits with room
constexpr uint64_t kDnMaxPixels = uint64_t(1) << 31;         // of all images: 64 B of workspace each
constexpr int kDnMaxIterations = 8, kDnMaxNormalPower = 8;
constexpr uint32_t kDnTile = 16;                             // a workgroup owns 16 x 16 pixels of ONE image: thread t = (t & 15, t >> 4)
constexpr uint32_t kDnThreads = kDnTile * kDnTile;
constexpr uint32_t kDnRecord = 16;                           // bytes of a packed record
constexpr uint32_t kDnRecordsPerPixel = 3;                   // (r g b var), (n.xyz hit), (P.xyz 0): what a tap reads
constexpr uint32_t kDnLdsPerCu = 160u * 1024u;
constexpr uint32_t kDnMaxGrid = 1u << 20;                    // workgroups of a launch at most: they stride over the tiles
// The largest step a halo'd tile of which fits a workgroup's LDS at all (48 x 48 records of 48 B = 108 KiB; step 16 would need 300 KiB).
constexpr int kDnLdsStepLimit = 8;
// Steps up to this one are staged in LDS (RTK_DENOISE_LDS_MAX_STEP; 0 = none).  Measured at 1920 x 1080:
// staged beats direct at steps 1, 2 and 4 (0.097 / 0.097 / 0.107 ms against 0.169 / 0.166 / 0.147) and loses at step 8 (0.293
// against 0.171), where the 108 KiB tile leaves one workgroup per CU and loads the records of nine pixels per pixel it owns.
constexpr int kDnLdsMaxStepDefault = 4;

// ---- refusals, in the order rtk.h gives; nullptr = go on
inline const char *denoise_refusal(const rtk_denoise_params &p, int32_t n_images) {
    if (p.width < 1 || p.height < 1) return "width and height must be >= 1";
    if (uint64_t(p.width) * uint64_t(p.height) > kDnMaxImagePixels) return "too many pixels per image (more than 2^28)";
    if (p.iterations < 1 || p.iterations > kDnMaxIterations) return "iterations must be in [1, 8]";
    if (p.normal_power_log2 < 0 || p.normal_power_log2 > kDnMaxNormalPower) return "normal_power_log2 must be in [0, 8]";
    if (!std::isfinite(p.sigma_luminance) || !(p.sigma_luminance > 0.0f)) return "sigma_luminance must be finite and > 0";
    if (!std::isfinite(p.sigma_plane) || !(p.sigma_plane > 0.0f)) return "sigma_plane must be finite and > 0";
    if (!std::isfinite(p.albedo_floor) || !(p.albedo_floor > 0.0f)) return "albedo_floor must be finite and > 0";
    if (n_images < 0) return "n_images must be >= 0";
    if (uint64_t(p.width) * uint64_t(p.height) * uint64_t(n_images) > kDnMaxPixels) return "too many pixels in total (more than 2^31)";
    return nullptr;
}
// behind n_images == 0: the planes a call cannot do without
inline const char *denoise_missing_plane(const rtk_denoise_inputs &in, const void *out) {
    if (!in.rgb || !in.normal || !in.position || !in.depth || !out) return "null rgb, normal, position, depth or output plane";
    return nullptr;
}
// behind that, the device variant alone: `need` = denoise_workspace(..).bytes
inline const char *denoise_device_refusal(const rtk_denoise_inputs &in, const void *out, const void *ws, uint64_t ws_bytes, uint64_t need) {
    const void *const planes[7] = {in.rgb, in.noise, in.albedo, in.normal, in.position, in.depth, out};
    for (const void *q : planes)
        if ((reinterpret_cast<uintptr_t>(q) & 3u) != 0u) return "plane pointers must be 4-byte aligned";
    if (!ws) return "null workspace";
    if ((reinterpret_cast<uintptr_t>(ws) & 15u) != 0u) return "the workspace must be 16-byte aligned";
    if (ws_bytes < need) return "the workspace is smaller than rtk_denoise_workspace_bytes asks for";
    return nullptr;
}

// ---- tiles: every image is cut into its own grid of 16 x 16 tiles anchored at its corner (edge tiles are partial), and the tiles
// of all images are numbered image by image, row-major inside one.  So a tile never spans two images.
struct DnTiling {
    uint32_t width, height, tiles_x, tiles_y;
    uint64_t tiles_per_image, n_tiles;
};
inline DnTiling denoise_tiling(uint32_t width, uint32_t height, uint32_t n_images) {
    DnTiling t;
    t.width = width; t.height = height;
    t.tiles_x = (width + kDnTile - 1u) / kDnTile; t.tiles_y = (height + kDnTile - 1u) / kDnTile;
    t.tiles_per_image = uint64_t(t.tiles_x) * t.tiles_y;
    t.n_tiles = t.tiles_per_image * n_images;
    return t;
}
struct DnTile { uint32_t image, x0, y0, w, h; };             // the pixels [x0, x0 + w) x [y0, y0 + h) of `image`
RTK_DN_FN DnTile denoise_tile(const DnTiling &t, uint64_t tile) {
    DnTile o;
    o.image = uint32_t(tile / t.tiles_per_image);
    const uint32_t in_image = uint32_t(tile - uint64_t(o.image) * t.tiles_per_image);
    const uint32_t ty = in_image / t.tiles_x, tx = in_image - ty * t.tiles_x;
    o.x0 = tx * kDnTile; o.y0 = ty * kDnTile;
    o.w = t.width - o.x0 < kDnTile ? t.width - o.x0 : kDnTile;
    o.h = t.height - o.y0 < kDnTile ? t.height - o.y0 : kDnTile;
    return o;
}
inline uint32_t denoise_grid(uint64_t n_tiles) { return uint32_t(n_tiles < kDnMaxGrid ? n_tiles : kDnMaxGrid); }

// ---- steps: iteration k filters at step 1 << k; its taps reach 2 * step pixels beyond the tile on every side
constexpr uint32_t denoise_step(int iteration) { return uint32_t(1) << iteration; }
constexpr uint32_t denoise_halo(uint32_t step) { return 2u * step; }
constexpr uint32_t denoise_lds_side(uint32_t step) { return kDnTile + 2u * denoise_halo(step); }       // pixels of a halo'd tile's edge
// A row of the tile in LDS begins at a multiple of 16 records (256 B, one row of the 64 banks): then the 16-lane groups of a
// 128-bit LDS read, which mix two rows of the tile, touch every bank once.
constexpr uint32_t denoise_lds_pitch(uint32_t step) { return (denoise_lds_side(step) + 15u) / 16u * 16u; }
constexpr uint32_t denoise_lds_bytes(uint32_t step) {
    return denoise_lds_pitch(step) * denoise_lds_side(step) * kDnRecordsPerPixel * kDnRecord;
}
// RTK_DENOISE_LDS_MAX_STEP as the environment has it (null = unset): 0 .. kDnLdsStepLimit, anything else = the default
inline int denoise_lds_max_step(const char *env) {
    if (!env || !*env) return kDnLdsMaxStepDefault;
    char *end = nullptr;
    const long v = std::strtol(env, &end, 10);
    if (end == env || *end != '\0' || v < 0 || v > kDnLdsStepLimit) return kDnLdsMaxStepDefault;
    return int(v);
}
// is the step's tile staged in LDS (else every tap reads the packed records from global memory)?
constexpr bool denoise_staged(uint32_t step, int lds_max_step) {
    return lds_max_step > 0 && step <= uint32_t(lds_max_step < kDnLdsStepLimit ? lds_max_step : kDnLdsStepLimit);
}

// ---- the workspace: the two guide records of every pixel, then the signal records twice (an iteration reads one and writes the
// other; the last one writes rgb_out, so a single iteration needs one).  Offsets in bytes from a 16-byte aligned base.
struct DnWorkspace { uint64_t g0, g1, c[2], bytes; };
inline DnWorkspace denoise_workspace(uint64_t pixels, int iterations) {
    DnWorkspace w;
    const uint64_t plane = pixels * kDnRecord;
    w.g0 = 0; w.g1 = plane; w.c[0] = 2u * plane;
    w.c[1] = iterations > 1 ? 3u * plane : w.c[0];
    w.bytes = (iterations > 1 ? 4u : 3u) * plane;
    return w;
}
// which of c[0], c[1] iteration k reads; it writes the other one (or, as the last, rgb_out)
constexpr int denoise_source(int iteration) { return iteration & 1; }

}  // namespace rtk
