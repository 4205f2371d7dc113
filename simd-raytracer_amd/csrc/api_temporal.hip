// C-ABI, rtk_temporal_accumulate: a frame blended with the history of the previous camera, reprojected through the world positions
// of its g-buffer.  The arithmetic of the calls -- refusals, scalars, grid -- is temporal_plan.hpp; the arithmetic of a pixel is
// temporal_math.hpp; the kernel is temporal.hip.  The calls take no accel and touch none: they depend on no scene state.
#include "accel.hpp"
#include "temporal.hpp"

using namespace rtk;

namespace {

// every refusal that both variants share, in rtk.h's order
int temporal_check(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev, const rtk_temporal_outputs *out) {
    if (!p || !cur || !out) return fail(RTK_ERR_INVALID, "null params, frame or outputs");
    if (const char *why = temporal_refusal(*p)) return fail(RTK_ERR_INVALID, why);
    if (const char *why = temporal_missing_plane(*cur, prev, *out)) return fail(RTK_ERR_INVALID, why);
    return RTK_OK;
}

int temporal_need_device() {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(RTK_ERR_NO_DEVICE, "no usable HIP device (this engine has no CPU path)");
    return RTK_OK;
}

// The one launch of a call, on `s`: device planes that have passed the checks; prev->view is read here, on the host.
int temporal_device_impl(const rtk_temporal_params &p, const rtk_temporal_frame &cur, const rtk_temporal_history *prev,
                         const rtk_temporal_outputs &out, hipStream_t s) {
    dev::TemporalArgs A;
    A.rgb = cur.rgb; A.noise = cur.noise; A.position = cur.position; A.normal = cur.normal; A.depth = cur.depth; A.mesh = cur.mesh;
    A.p_rgb = prev ? prev->rgb : nullptr; A.p_noise = prev ? prev->noise : nullptr; A.p_length = prev ? prev->length : nullptr;
    A.p_position = prev ? prev->position : nullptr; A.p_normal = prev ? prev->normal : nullptr; A.p_depth = prev ? prev->depth : nullptr;
    A.p_mesh = prev ? prev->mesh : nullptr;
    A.o_rgb = out.rgb; A.o_noise = out.noise; A.o_length = out.length;
    A.tiling = temporal_tiling(p);
    A.k = temporal_consts(p, prev ? prev->view : nullptr);
    RTK_HIP_AS(launch_temporal_accumulate(A, s), "launch k_temporal_accumulate");
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_temporal_accumulate_device(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                                   const rtk_temporal_outputs *out, void *stream) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_check(p, cur, prev, out));
        if (const char *why = temporal_device_refusal(*cur, prev, *out)) return fail(RTK_ERR_INVALID, why);
        RTK_TRY(temporal_need_device());
        return temporal_device_impl(*p, *cur, prev, *out, static_cast<hipStream_t>(stream));
    });
}

int rtk_temporal_accumulate(const rtk_temporal_params *p, const rtk_temporal_frame *cur, const rtk_temporal_history *prev,
                            const rtk_temporal_outputs *out) {
    return abi_guard([&]() -> int {
        RTK_TRY(temporal_check(p, cur, prev, out));
        RTK_TRY(temporal_need_device());
        // the planes one behind the other in one staging buffer of 4-byte words (the mesh ids are words too), the three outputs
        // last; the buffer is the call's own and is freed when it returns
        const size_t n = size_t(p->width) * size_t(p->height);
        const void *const host[13] = {cur->rgb, cur->noise, cur->position, cur->normal, cur->depth, cur->mesh,
                                      prev ? prev->rgb : nullptr, prev ? prev->noise : nullptr, prev ? prev->length : nullptr,
                                      prev ? prev->position : nullptr, prev ? prev->normal : nullptr, prev ? prev->depth : nullptr,
                                      prev ? prev->mesh : nullptr};
        const size_t each[13] = {3, 1, 3, 3, 1, 1, 3, 1, 1, 3, 3, 1, 1};
        size_t off[17] = {0};
        for (int i = 0; i < 13; ++i) off[i + 1] = off[i] + (host[i] ? each[i] * n : 0u);
        off[14] = off[13] + 3u * n;                                    // out rgb at off[13]
        off[15] = off[14] + (out->noise ? n : 0u);                     // out noise at off[14]
        off[16] = off[15] + n;                                         // out length at off[15]
        DevBuf<float> stage;
        RTK_MEM(stage.reserve(off[16]));
        const float *d[13];
        for (int i = 0; i < 13; ++i) {
            d[i] = host[i] ? stage.get() + off[i] : nullptr;
            if (host[i]) RTK_HIP(hipMemcpy(stage.get() + off[i], host[i], each[i] * n * sizeof(float), hipMemcpyHostToDevice));
        }
        rtk_temporal_frame dcur;
        dcur.rgb = d[0]; dcur.noise = d[1]; dcur.position = d[2]; dcur.normal = d[3]; dcur.depth = d[4];
        dcur.mesh = reinterpret_cast<const uint32_t *>(d[5]);
        rtk_temporal_history dprev;
        dprev.rgb = d[6]; dprev.noise = d[7]; dprev.length = d[8]; dprev.position = d[9]; dprev.normal = d[10]; dprev.depth = d[11];
        dprev.mesh = reinterpret_cast<const uint32_t *>(d[12]);
        dprev.view = prev ? prev->view : nullptr;
        rtk_temporal_outputs dout;
        dout.rgb = stage.get() + off[13]; dout.noise = out->noise ? stage.get() + off[14] : nullptr; dout.length = stage.get() + off[15];
        RTK_TRY(temporal_device_impl(*p, dcur, prev ? &dprev : nullptr, dout, nullptr));
        // (a copy on the null stream is behind the kernel and blocks the host)
        RTK_HIP(hipMemcpy(out->rgb, dout.rgb, 3u * n * sizeof(float), hipMemcpyDeviceToHost));
        if (out->noise) RTK_HIP(hipMemcpy(out->noise, dout.noise, n * sizeof(float), hipMemcpyDeviceToHost));
        RTK_HIP(hipMemcpy(out->length, dout.length, n * sizeof(float), hipMemcpyDeviceToHost));
        return RTK_OK;
    });
}

}  // extern "C"
