// C-ABI, rtk_render_motion: where each pixel's surface point was in the previous pose, and on request its screen-space motion,
// from a frame's tri / bary planes, the previous pose's vertices and the accel's live topology tables.  The arithmetic of the
// calls -- refusals, alignment, scalars, grid, the host variant's stage -- is motion_plan.hpp; the arithmetic of a pixel is
// motion_math.hpp; the kernel is motion.hip.  Nothing here touches the accel's camera, its cost tables, its engine verdict or its
// counters.
#include <mutex>

#include "accel.hpp"
#include "motion.hpp"

using namespace rtk;

namespace {

// The one launch of a call, on `s`: device planes that have passed the checks, under a->mu, the accel resident and `s` behind the
// last update.  The topology tables of an accel no update has touched are made here, once (the one step that may block the host).
int motion_device_impl(rtk_accel *a, const rtk_motion_params &p, const uint32_t *tri, const float *bary, const float *verts,
                       const rtk_view *prev_view, const rtk_motion_outputs &out, hipStream_t s) {
    RTK_TRY(ensure_update_static(a));
    dev::MotionArgs A;
    A.tri = tri; A.bary = bary; A.verts = verts;
    A.index = a->topo.index.get();
    A.n_tris = uint32_t(a->scene.n_triangles); A.n_verts = uint32_t(a->scene.n_vertices);
    A.prev_position = out.prev_position; A.motion = out.motion;
    A.tiling = motion_tiling(p);
    A.k = motion_consts(p, out.motion ? prev_view : nullptr);
    RTK_HIP_AS(launch_motion(A, s), "launch k_motion");
    return RTK_OK;
}

}  // namespace

extern "C" {

int rtk_render_motion_device(rtk_accel *a, const rtk_motion_params *p, const uint32_t *d_tri, const float *d_bary, const float *d_prev_vertices,
                             const rtk_view *prev_view, const rtk_motion_outputs *out, void *stream) {
    return abi_guard([&]() -> int {
        if (const char *why = motion_refusal(a, p, d_tri, d_bary, d_prev_vertices, prev_view, out)) return fail(RTK_ERR_INVALID, why);
        if (const char *why = motion_device_refusal(d_tri, d_bary, d_prev_vertices, *out)) return fail(RTK_ERR_INVALID, why);
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a, static_cast<hipStream_t>(stream)));
        return motion_device_impl(a, *p, d_tri, d_bary, d_prev_vertices, prev_view, *out, static_cast<hipStream_t>(stream));
    });
}

int rtk_render_motion(rtk_accel *a, const rtk_motion_params *p, const uint32_t *tri, const float *bary, const float *prev_vertices,
                      const rtk_view *prev_view, const rtk_motion_outputs *out) {
    return abi_guard([&]() -> int {
        if (const char *why = motion_refusal(a, p, tri, bary, prev_vertices, prev_view, out)) return fail(RTK_ERR_INVALID, why);
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        // the two planes and the vertices up, the planes asked for down (plane i of the stage is kMvStage* i)
        const uint64_t n = uint64_t(p->width) * uint64_t(p->height), nv = uint64_t(a->scene.n_vertices);
        const void *const up[3] = {tri, bary, prev_vertices};
        void *const down[2] = {out->prev_position, out->motion};
        HostStage &st = a->stage;
        StageLayout L;
        for (int i = 0; i < kMvStagePlanes; ++i)
            L.add(motion_stage_words(i, n, nv), i < kMvStagePrevPosition || down[i - kMvStagePrevPosition] != nullptr);
        RTK_MEM(st.reserve(L));
        for (int i = 0; i < kMvStagePrevPosition; ++i) RTK_HIP(st.upload(i, up[i]));
        const rtk_motion_outputs d = {st.at<float>(kMvStagePrevPosition), st.at<float>(kMvStageMotion)};
        RTK_TRY(motion_device_impl(a, *p, st.at<uint32_t>(kMvStageTri), st.at<float>(kMvStageBary), st.at<float>(kMvStageVerts), prev_view, d, nullptr));
        // (a copy on the null stream is behind the kernel and blocks the host)
        for (int i = 0; i < 2; ++i) RTK_HIP(st.download(kMvStagePrevPosition + i, down[i]));
        return RTK_OK;
    });
}

}  // extern "C"
