// Host plan of rtk_temporal_accumulate (api_temporal.hip, temporal.hip): what the calls refuse and in which order, the scalars the
// kernel is handed, and the grid.  The tiles are the denoiser's (denoise_plan.hpp denoise_tiling / denoise_tile, one image).
// Plain host arithmetic, no HIP: tests/cpp/temporal_plan_check.cpp runs it.
#pragma once

#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/rtk.h"
#include "camera_plan.hpp"
#include "denoise_plan.hpp"
#include "temporal_math.hpp"

namespace rtk {

constexpr int32_t kTpMaxSide = 16384;                  // so a pixel index fits 28 bits and a tap's coordinates convert exactly
constexpr int32_t kTpMaxHistory = 1 << 20;
constexpr uint32_t kTpThreads = kDnThreads;            // one workgroup per 16 x 16 tile
// workgroups of a launch at most: about what 256 CUs hold at once at 7 waves per SIMD (7 workgroups of 4 waves each); more tiles
// than that are strided over
constexpr uint32_t kTpMaxGrid = 2048;

// ---- refusals, in the order rtk.h gives; nullptr = go on
inline const char *temporal_refusal(const rtk_temporal_params &p) {
    if (p.width < 1 || p.width > kTpMaxSide) return "width must be in [1, 16384]";
    if (p.height < 1 || p.height > kTpMaxSide) return "height must be in [1, 16384]";
    if (!std::isfinite(p.fov_degrees) || !(p.fov_degrees > 0.0) || !(p.fov_degrees < 180.0)) return "fov_degrees must be finite and in (0, 180)";
    if (!std::isfinite(p.alpha_min) || !(p.alpha_min > 0.0f) || !(p.alpha_min <= 1.0f)) return "alpha_min must be finite and in (0, 1]";
    if (!std::isfinite(p.plane_tolerance) || !(p.plane_tolerance > 0.0f)) return "plane_tolerance must be finite and > 0";
    if (!std::isfinite(p.normal_min_dot) || !(p.normal_min_dot >= -1.0f) || !(p.normal_min_dot <= 1.0f)) return "normal_min_dot must be finite and in [-1, 1]";
    if (p.max_history < 1 || p.max_history > kTpMaxHistory) return "max_history must be in [1, 1048576]";
    return nullptr;
}
// behind that: the planes a call cannot do without, then the families
inline const char *temporal_missing_plane(const rtk_temporal_frame &cur, const rtk_temporal_history *prev, const rtk_temporal_outputs &out) {
    if (!cur.rgb || !cur.position || !cur.normal || !cur.depth) return "null rgb, position, normal or depth plane of the new frame";
    if (!out.rgb || !out.length) return "null rgb or length plane of the outputs";
    if (prev && (!prev->rgb || !prev->length || !prev->position || !prev->normal || !prev->depth || !prev->view))
        return "null rgb, length, position, normal, depth plane or view of the history";
    const bool noise = cur.noise != nullptr;
    if ((out.noise != nullptr) != noise || (prev && (prev->noise != nullptr) != noise))
        return "the noise planes of the new frame, the history and the outputs must be all set or all null";
    if (prev && (prev->mesh != nullptr) != (cur.mesh != nullptr)) return "the mesh planes of the new frame and the history must be both set or both null";
    return nullptr;
}
// behind that, the device variant alone
inline const char *temporal_device_refusal(const rtk_temporal_frame &cur, const rtk_temporal_history *prev, const rtk_temporal_outputs &out) {
    const void *planes[16] = {cur.rgb, cur.noise, cur.position, cur.normal, cur.depth, cur.mesh, out.rgb, out.noise, out.length};
    if (prev) {
        const void *const more[7] = {prev->rgb, prev->noise, prev->length, prev->position, prev->normal, prev->depth, prev->mesh};
        for (int i = 0; i < 7; ++i) planes[9 + i] = more[i];
    } else {
        for (int i = 9; i < 16; ++i) planes[i] = nullptr;
    }
    for (const void *q : planes)
        if ((reinterpret_cast<uintptr_t>(q) & 3u) != 0u) return "plane pointers must be 4-byte aligned";
    return nullptr;
}

// ---- the scalars: the camera's are camera_plan.hpp's, the one copy a frame's rays are made from; view null = no history, and
// then the kernel never reads cam and m
inline tp::Consts temporal_consts(const rtk_temporal_params &p, const rtk_view *view) {
    tp::Consts k;
    const CameraScalars c = camera_scalars(uint32_t(p.width), uint32_t(p.height), p.fov_degrees);
    for (int i = 0; i < 3; ++i) k.cam[i] = view ? view->position[i] : 0.0f;
    for (int i = 0; i < 9; ++i) k.m[i] = view ? view->matrix[i] : 0.0f;
    k.th = c.tan_half_fov; k.aspect = c.aspect; k.wf = c.width_f; k.hf = c.height_f;
    k.nmax = static_cast<float>(p.max_history);
    k.alpha_min = p.alpha_min; k.plane_tolerance = p.plane_tolerance; k.normal_min_dot = p.normal_min_dot;
    return k;
}

// ---- the grid: one workgroup per tile up to kTpMaxGrid
inline DnTiling temporal_tiling(const rtk_temporal_params &p) { return denoise_tiling(uint32_t(p.width), uint32_t(p.height), 1u); }
inline uint32_t temporal_grid(uint64_t n_tiles) { return uint32_t(n_tiles < kTpMaxGrid ? n_tiles : kTpMaxGrid); }

}  // namespace rtk
