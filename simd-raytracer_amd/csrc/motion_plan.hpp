// Host plan of rtk_render_motion (api_motion.hip, motion.hip): what the calls refuse and in which order, the alignment the device
// variant asks for, the scalars the kernel is handed, and the grid.  The tiles are the denoiser's (denoise_plan.hpp denoise_tiling /
// denoise_tile, one image), the projection's scalars are camera_plan.hpp's as for rtk_temporal_accumulate.
// Plain host arithmetic, no HIP, no accel: tests/cpp/motion_plan_check.cpp runs it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"
#include "camera_plan.hpp"
#include "denoise_plan.hpp"
#include "motion_math.hpp"

namespace rtk {

constexpr int32_t kMvMaxSide = 16384;                  // so a pixel index fits 28 bits and 3 * it 32
constexpr uint32_t kMvThreads = kDnThreads;            // one workgroup per 16 x 16 tile
// workgroups of a launch at most: what 256 CUs hold at once at 8 waves per SIMD (8 workgroups of 4 waves each); more tiles than
// that are strided over
constexpr uint32_t kMvMaxGrid = 2048;

// ---- refusals, in the order rtk.h gives; nullptr = go on
inline const char *motion_refusal(const void *accel, const rtk_motion_params *p, const void *tri, const void *bary, const void *prev_vertices,
                                  const rtk_view *prev_view, const rtk_motion_outputs *out) {
    if (!accel || !p || !tri || !bary || !prev_vertices || !out) return "null accel, params, tri, bary, prev_vertices or outputs";
    if (p->width < 1 || p->width > kMvMaxSide) return "width must be in [1, 16384]";
    if (p->height < 1 || p->height > kMvMaxSide) return "height must be in [1, 16384]";
    if (!std::isfinite(p->fov_degrees) || !(p->fov_degrees > 0.0) || !(p->fov_degrees < 180.0)) return "fov_degrees must be finite and in (0, 180)";
    if (!out->prev_position && !out->motion) return "prev_position and motion are both null";
    if (out->motion && !prev_view) return "motion needs prev_view";
    return nullptr;
}
// behind that, the device variant alone
inline const char *motion_device_refusal(const void *tri, const void *bary, const void *prev_vertices, const rtk_motion_outputs &out) {
    const void *const planes[5] = {tri, bary, prev_vertices, out.prev_position, out.motion};
    for (const void *q : planes)
        if ((reinterpret_cast<uintptr_t>(q) & 3u) != 0u) return "plane and vertex pointers must be 4-byte aligned";
    return nullptr;
}

// ---- the scalars of the projection; view null = no motion plane, and then the kernel never reads them
inline tp::Consts motion_consts(const rtk_motion_params &p, const rtk_view *view) {
    tp::Consts k = {};
    const CameraScalars c = camera_scalars(uint32_t(p.width), uint32_t(p.height), p.fov_degrees);
    for (int i = 0; i < 3; ++i) k.cam[i] = view ? view->position[i] : 0.0f;
    for (int i = 0; i < 9; ++i) k.m[i] = view ? view->matrix[i] : 0.0f;
    k.th = c.tan_half_fov; k.aspect = c.aspect; k.wf = c.width_f; k.hf = c.height_f;
    return k;
}

// ---- the grid: one workgroup per tile up to kMvMaxGrid
inline DnTiling motion_tiling(const rtk_motion_params &p) { return denoise_tiling(uint32_t(p.width), uint32_t(p.height), 1u); }
inline uint32_t motion_grid(uint64_t n_tiles) { return uint32_t(n_tiles < kMvMaxGrid ? n_tiles : kMvMaxGrid); }

// ---- the host variant's stage (stage_plan.hpp): words of each plane, in this order
enum : int { kMvStageTri = 0, kMvStageBary, kMvStageVerts, kMvStagePrevPosition, kMvStageMotion, kMvStagePlanes };
inline uint64_t motion_stage_words(int plane, uint64_t pixels, uint64_t n_vertices) {
    switch (plane) {
        case kMvStageTri: return pixels;
        case kMvStageBary: return 2u * pixels;
        case kMvStageVerts: return 3u * n_vertices;
        case kMvStagePrevPosition: return 3u * pixels;
        case kMvStageMotion: return 2u * pixels;
        default: return 0u;
    }
}

}  // namespace rtk
