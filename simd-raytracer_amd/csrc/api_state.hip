// C-ABI, the rest of scene<F> on a live accel: rtk_accel_{get,set}_lights, _materials and _background (rtk.h).  The launch paths
// read a->scene and the device tables when they run (api_frame.hip scene_args), so most of this is bookkeeping; the device work
// that a changed set of refractive materials asks for is remake_occluders (api_update.hip, occluders.hip).
#include <algorithm>
#include <cstring>
#include <mutex>

#include "accel.hpp"

using namespace rtk;

namespace {

// Room for n lights in d_lights, of a resident accel whose device is idle.  A larger table is made before the old one goes, so a
// failure leaves the accel as it was.
int reserve_lights(rtk_accel *a, size_t n) {
    if (n <= a->d_lights.capacity()) return RTK_OK;
    DevBuf<DevLight> larger;
    RTK_MEM(larger.reserve(n, grow_lights()));
    a->d_lights.swap(larger);                            // (the old table goes with `larger`)
    return RTK_OK;
}

// every block's cost scales with the number of lights; their positions leave the silhouettes where they are (rtk.h)
void lights_changed(rtk_accel *a, size_t n_before) {
    if (a->scene.lights.size() == n_before) return;
    forget_orders(a, kKeepTrial);
}

}  // namespace

extern "C" {

int rtk_accel_get_lights(const rtk_accel *a, rtk_light *out, int32_t cap, int32_t *n) {
    return abi_guard([&]() -> int {
        if (!a || !n) return fail(RTK_ERR_INVALID, "null accel or count");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        const size_t have = a->scene.lights.size();
        *n = int32_t(have);
        const size_t take = (out && cap > 0) ? std::min(have, size_t(cap)) : 0;
        if (take == 0) return RTK_OK;
        if (a->lights_on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(hipDeviceSynchronize());
            RTK_HIP(hipMemcpy(out, a->d_lights.get(), take * sizeof(rtk_light), hipMemcpyDeviceToHost));
        } else std::memcpy(out, a->scene.lights.data(), take * sizeof(rtk_light));
        return RTK_OK;
    });
}

int rtk_accel_set_lights(rtk_accel *a, const rtk_light *lights, int32_t n) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n < 0 || (n > 0 && !lights)) return fail(RTK_ERR_INVALID, "negative light count or null lights");
        std::lock_guard<std::mutex> lock(a->mu);
        std::vector<DevLight> table(static_cast<size_t>(n));
        if (n > 0) std::memcpy(table.data(), lights, size_t(n) * sizeof(DevLight));
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            // entry: nothing issued earlier on this accel, on whatever stream, may still read the table
            RTK_HIP(a->geom_fence.quiesce());
            RTK_TRY(reserve_lights(a, size_t(n)));
            if (n > 0) RTK_HIP(hipMemcpy(a->d_lights.get(), table.data(), size_t(n) * sizeof(DevLight), hipMemcpyHostToDevice));
        }
        const size_t before = a->scene.lights.size();
        a->scene.lights.swap(table);
        a->lights_on_device = false;
        lights_changed(a, before);
        return RTK_OK;
    });
}

int rtk_accel_set_lights_device(rtk_accel *a, const rtk_light *d_lights, int32_t n, void *hip_stream) {
    return abi_guard([&]() -> int {
        if (!a) return fail(RTK_ERR_INVALID, "null accel");
        if (n < 0 || (n > 0 && !d_lights)) return fail(RTK_ERR_INVALID, "negative light count or null lights");
        std::lock_guard<std::mutex> lock(a->mu);
        hipStream_t s = static_cast<hipStream_t>(hip_stream);
        RTK_TRY(ensure_device(a));
        RTK_HIP(a->geom_fence.quiesce());
        RTK_TRY(reserve_lights(a, size_t(n)));
        std::vector<DevLight> count_only(static_cast<size_t>(n), DevLight{{0.f, 0.f, 0.f}, 0.f});
        if (n > 0) RTK_HIP(hipMemcpyAsync(a->d_lights.get(), d_lights, size_t(n) * sizeof(DevLight), hipMemcpyDeviceToDevice, s));
        RTK_HIP(a->geom_fence.publish(s));
        const size_t before = a->scene.lights.size();
        a->scene.lights.swap(count_only);              // the COUNT every launch path reads; the values live in d_lights
        a->lights_on_device = true;
        lights_changed(a, before);
        return RTK_OK;
    });
}

int rtk_accel_get_materials(const rtk_accel *a, rtk_material *out) {
    return abi_guard([&]() -> int {
        if (!a || !out) return fail(RTK_ERR_INVALID, "null accel or materials");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        if (!a->scene.materials.empty()) std::memcpy(out, a->scene.materials.data(), a->scene.materials.size() * sizeof(rtk_material));
        return RTK_OK;
    });
}

int rtk_accel_set_materials(rtk_accel *a, const rtk_material *materials, int32_t n) {
    return abi_guard([&]() -> int {
        if (!a || !materials) return fail(RTK_ERR_INVALID, "null accel or materials");
        std::lock_guard<std::mutex> lock(a->mu);
        if (n < 0 || size_t(n) != a->scene.materials.size()) return fail(RTK_ERR_INVALID, "the number of materials is fixed when the scene is made");
        // scene.cpp, scene_from_desc
        std::vector<DevMaterial> table(static_cast<size_t>(n));
        for (size_t i = 0; i < table.size(); ++i) {
            DevMaterial &m = table[i];
            std::memcpy(&m, &materials[i], sizeof(m));
            if (m.kind < RTK_MAT_DIFFUSE || m.kind > RTK_MAT_TEXTURE) return fail(RTK_ERR_INVALID, "material type unknown");
            if (m.kind == RTK_MAT_TEXTURE) {
                if (m.texture < 0 || size_t(m.texture) >= a->scene.textures.size()) return fail(RTK_ERR_INVALID, "texture material refers to a texture that does not exist");
            } else m.texture = -1;
            m.pad = 0u;
        }
        if (a->on_device) {
            RTK_HIP(hipSetDevice(a->device));
            RTK_HIP(a->geom_fence.quiesce());
            // the new table goes into the spare one, what follows from it is built beside what is active, and both are swapped in at the end
            RTK_MEM(a->st_materials.reserve(table.size()));             // (once: the number of materials is fixed)
            if (!table.empty()) RTK_HIP(hipMemcpy(a->st_materials.get(), table.data(), table.size() * sizeof(DevMaterial), hipMemcpyHostToDevice));
            RTK_TRY(remake_occluders(a, table, a->st_materials.get(), nullptr));
            a->d_materials.swap(a->st_materials);
        }
        a->scene.materials.swap(table);
        a->has_refractive = any_refractive(a->scene.materials);
        // a scene that starts or stops forking runs other kernels over other block costs, and needs a new verdict
        forget_orders(a);
        return RTK_OK;
    });
}

int rtk_accel_get_background(const rtk_accel *a, float rgb[3]) {
    return abi_guard([&]() -> int {
        if (!a || !rgb) return fail(RTK_ERR_INVALID, "null accel or colour");
        std::lock_guard<std::mutex> lock(const_cast<rtk_accel *>(a)->mu);
        std::memcpy(rgb, a->scene.background, sizeof(a->scene.background));
        return RTK_OK;
    });
}

int rtk_accel_set_background(rtk_accel *a, const float rgb[3]) {
    return abi_guard([&]() -> int {
        if (!a || !rgb) return fail(RTK_ERR_INVALID, "null accel or colour");
        std::lock_guard<std::mutex> lock(a->mu);
        std::memcpy(a->scene.background, rgb, sizeof(a->scene.background));
        return RTK_OK;
    });
}

}  // extern "C"
