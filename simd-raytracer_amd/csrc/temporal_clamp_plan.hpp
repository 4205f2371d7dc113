// Host plan of rtk_temporal_accumulate_clamped (api_temporal.hip, temporal_clamp.hip) on top of temporal_plan.hpp: what the calls
// refuse beyond the plain call and in which order, the aliasing they refuse, and the LDS a workgroup stages the new frame's tile
// and halo in.  Plain host arithmetic, no HIP: tests/cpp/temporal_clamp_plan_check.cpp runs it.
#pragma once

#include "temporal_plan.hpp"

namespace rtk {

constexpr int32_t kTcMinRadius = 1, kTcMaxRadius = 3;
constexpr uint32_t kTcPlanes = 5;                      // words per staged pixel, each a plane of its own: r, g, b, var, mesh

// ---- refusals of rtk_temporal_clamp, in the struct's order; nullptr = go on
inline const char *temporal_clamp_refusal(const rtk_temporal_clamp &k) {
    if (k.radius < kTcMinRadius || k.radius > kTcMaxRadius) return "radius must be in [1, 3]";
    if (!std::isfinite(k.gamma) || !(k.gamma >= 0.0f)) return "gamma must be finite and >= 0";
    if (!std::isfinite(k.history_keep) || !(k.history_keep >= 0.0f) || !(k.history_keep <= 1.0f)) return "history_keep must be finite and in [0, 1]";
    return nullptr;
}
// neighbours of the new frame are read, so its colour and noise planes cannot be written
inline const char *temporal_clamp_alias(const rtk_temporal_frame &cur, const rtk_temporal_outputs &out) {
    if (out.rgb == cur.rgb) return "out->rgb must not be cur->rgb: the clamped call reads the new frame's neighbours";
    if (out.noise && cur.noise && out.noise == cur.noise) return "out->noise must not be cur->noise: the clamped call reads the new frame's neighbours";
    return nullptr;
}
// every refusal behind the null structs, in rtk.h's order; device: the device variant's alignment as the last one
inline const char *temporal_clamped_refusal(const rtk_temporal_params &p, const rtk_temporal_clamp &k, const rtk_temporal_frame &cur,
                                            const rtk_temporal_history *prev, const rtk_temporal_outputs &out, bool device) {
    if (const char *why = temporal_refusal(p)) return why;
    if (const char *why = temporal_clamp_refusal(k)) return why;
    if (const char *why = temporal_missing_plane(cur, prev, out)) return why;
    if (const char *why = temporal_clamp_alias(cur, out)) return why;
    if (device)
        if (const char *why = temporal_device_refusal(cur, prev, out)) return why;
    return nullptr;
}

// ---- LDS: the 16 x 16 tile with a halo of `radius` pixels on every side, kTcPlanes planes of one word per pixel
constexpr uint32_t temporal_clamp_side(int32_t radius) { return kDnTile + 2u * uint32_t(radius); }
constexpr uint32_t temporal_clamp_lds_pixels(int32_t radius) { return temporal_clamp_side(radius) * temporal_clamp_side(radius); }
constexpr uint32_t temporal_clamp_lds_bytes(int32_t radius) { return temporal_clamp_lds_pixels(radius) * kTcPlanes * 4u; }

}  // namespace rtk
