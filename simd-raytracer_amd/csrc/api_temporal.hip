// C-ABI, rtk_temporal_accumulate: a frame blended with the history of the previous camera, reprojected through the world positions
// of its g-buffer.  The arithmetic of the calls -- refusals, scalars, grid -- is temporal_plan.hpp; the arithmetic of a pixel is
// temporal_math.hpp; the kernel is temporal.hip.  The calls take no accel and touch none: they depend on no scene state.
// rtk_temporal_accumulate_clamped is the same call with the history bounded by the new frame's neighbourhood: its refusals and LDS
// are temporal_clamp_plan.hpp, its arithmetic temporal_clamp_math.hpp, its kernel temporal_clamp.hip; both host variants stage
// their planes through temporal_staged below.
#include "accel.hpp"
#include "temporal.hpp"
#include "temporal_clamp.hpp"

using namespace rtk;

namespace {

// every refusal that both variants share, in rtk.h's order
int temporal_check(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev, const rtk_temporal_outputs *out) {
    if (!p || !cur || !out) return fail(RTK_ERR_INVALID, "null params, frame or outputs");
    if (const char *why = temporal_refusal(*p)) return fail(RTK_ERR_INVALID, why);
    if (const char *why = temporal_missing_plane(*cur, prev, *out)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

// the kernel's arguments from device planes that have passed the checks; prev->view is read here, on the host
dev::TemporalArgs temporal_args(const rtk_temporal_params &p, const rtk_temporal_frame &cur, const rtk_temporal_history *prev,
                                const rtk_temporal_outputs &out) {
    dev::TemporalArgs A;
    A.rgb = cur.rgb; A.noise = cur.noise; A.position = cur.position; A.normal = cur.normal; A.depth = cur.depth; A.mesh = cur.mesh;
    A.p_rgb = prev ? prev->rgb : nullptr; A.p_noise = prev ? prev->noise : nullptr; A.p_length = prev ? prev->length : nullptr;
    A.p_position = prev ? prev->position : nullptr; A.p_normal = prev ? prev->normal : nullptr; A.p_depth = prev ? prev->depth : nullptr;
    A.p_mesh = prev ? prev->mesh : nullptr;
    A.o_rgb = out.rgb; A.o_noise = out.noise; A.o_length = out.length;
    A.tiling = temporal_tiling(p);
    A.k = temporal_consts(p, prev ? prev->view : nullptr);
    return A;
}

// The one launch of a call, on `s`.
int temporal_device_impl(const rtk_temporal_params &p, const rtk_temporal_frame &cur, const rtk_temporal_history *prev,
                         const rtk_temporal_outputs &out, hipStream_t s) {
    RTK_HIP_AS(launch_temporal_accumulate(temporal_args(p, cur, prev, out), s), "launch k_temporal_accumulate");
    return RTK_OK;
}
int temporal_clamped_device_impl(const rtk_temporal_params &p, const rtk_temporal_clamp &k, const rtk_temporal_frame &cur,
                                 const rtk_temporal_history *prev, const rtk_temporal_outputs &out, hipStream_t s) {
    const dev::TemporalClampArgs B = {temporal_args(p, cur, prev, out), k.radius, k.gamma, k.history_keep};
    RTK_HIP_AS(launch_temporal_accumulate_clamped(B, s), "launch k_temporal_accumulate_clamped");
    return RTK_OK;
}

// The host variants: every plane of the frame, of the history and of the outputs in one staging buffer (the mesh ids are words too);
// the buffer is the call's own and is freed when it returns.  launch(dcur, dprev or null, dout) runs the call's kernel on the null
// stream.
template <typename Launch>
int temporal_staged(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                    const rtk_temporal_outputs *out, Launch &&launch) {
    const uint64_t n = uint64_t(p->width) * uint64_t(p->height);
    const rtk_temporal_history none = {};
    const rtk_temporal_history &h = prev ? *prev : none;
    const void *const host[13] = {cur->rgb, cur->noise, cur->position, cur->normal, cur->depth, cur->mesh,
                                  h.rgb, h.noise, h.length, h.position, h.normal, h.depth, h.mesh};
    const uint64_t each[13] = {3, 1, 3, 3, 1, 1, 3, 1, 1, 3, 3, 1, 1};
    StageLayout L;
    for (int i = 0; i < 13; ++i) L.add(each[i] * n, host[i] != nullptr);
    const int o_rgb = L.add(3 * n), o_noise = L.add(n, out->noise != nullptr), o_length = L.add(n);
    HostStage stage;
    RTK_MEM(stage.reserve(L));
    for (int i = 0; i < 13; ++i) RTK_HIP(stage.upload(i, host[i]));
    const rtk_temporal_frame dcur = {stage.at<float>(0), stage.at<float>(1), stage.at<float>(2), stage.at<float>(3), stage.at<float>(4),
                                     stage.at<uint32_t>(5)};
    const rtk_temporal_history dprev = {stage.at<float>(6), stage.at<float>(7), stage.at<float>(8), stage.at<float>(9), stage.at<float>(10),
                                        stage.at<float>(11), stage.at<uint32_t>(12), h.view};
    const rtk_temporal_outputs dout = {stage.at<float>(o_rgb), stage.at<float>(o_noise), stage.at<float>(o_length)};
    RTK_TRY(launch(dcur, prev ? &dprev : nullptr, dout));
    // (a copy on the null stream is behind the kernel and blocks the host)
    RTK_HIP(stage.download(o_rgb, out->rgb));
    RTK_HIP(stage.download(o_noise, out->noise));
    RTK_HIP(stage.download(o_length, out->length));
    return RTK_OK;
}

// every refusal that both clamped variants share, in rtk.h's order
int temporal_clamped_check(const rtk_temporal_params *p, const rtk_temporal_clamp *k, const rtk_temporal_frame *cur,
                           const rtk_temporal_history *prev, const rtk_temporal_outputs *out, bool device) {
    if (!p || !k || !cur || !out) return fail(RTK_ERR_INVALID, "null params, clamp, frame or outputs");
    if (const char *why = temporal_clamped_refusal(*p, *k, *cur, prev, *out, device)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_temporal_accumulate_device(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                                   const rtk_temporal_outputs *out, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_check(p, cur, prev, out));
        if (const char *why = temporal_device_refusal(*cur, prev, *out)) return fail(RTK_ERR_INVALID, why);
        RTK_TRY(need_device());
        return temporal_device_impl(*p, *cur, prev, *out, static_cast<hipStream_t>(stream));
    });
}

int rtk_temporal_accumulate(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                            const rtk_temporal_outputs *out) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_check(p, cur, prev, out));
        RTK_TRY(need_device());
        return temporal_staged(p, cur, prev, out, [&](const rtk_temporal_frame &dcur, const rtk_temporal_history *dprev, const rtk_temporal_outputs &dout) {
            return temporal_device_impl(*p, dcur, dprev, dout, nullptr);
        });
    });
}

int rtk_temporal_accumulate_clamped_device(const rtk_temporal_params *p, const rtk_temporal_clamp *k, const rtk_temporal_frame *cur,
                                           const rtk_temporal_history *prev, const rtk_temporal_outputs *out, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_clamped_check(p, k, cur, prev, out, true));
        RTK_TRY(need_device());
        return temporal_clamped_device_impl(*p, *k, *cur, prev, *out, static_cast<hipStream_t>(stream));
    });
}

int rtk_temporal_accumulate_clamped(const rtk_temporal_params *p, const rtk_temporal_clamp *k, const rtk_temporal_frame *cur,
                                    const rtk_temporal_history *prev, const rtk_temporal_outputs *out) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_clamped_check(p, k, cur, prev, out, false));
        RTK_TRY(need_device());
        // (the staged planes are distinct, so the aliasing that was refused above cannot come back)
        return temporal_staged(p, cur, prev, out, [&](const rtk_temporal_frame &dcur, const rtk_temporal_history *dprev, const rtk_temporal_outputs &dout) {
            return temporal_clamped_device_impl(*p, *k, dcur, dprev, dout, nullptr);
        });
    });
}

}  // extern "C"
