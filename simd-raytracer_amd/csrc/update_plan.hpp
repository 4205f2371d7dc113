// What changing a resident accel decides on the host (api_update.hip, api_state.hip, api.hip ensure_device): the capacities a
// device build is tried with, which materials are opaque, the numbering of RTK_TRAVERSAL_FAST's opaque-only occlusion tree and
// the topology tables of a first update.  Plain structs and vectors, no HIP, no accel: the callers ask these, then reserve,
// copy and launch what they say; tests/cpp/update_plan_check.cpp pins them.  A function that can refuse returns its error text,
// nullptr when it did not.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "build_nodes.hpp"
#include "rtk_internal.hpp"

namespace rtk {

// Capacities of the device build.  A tree of depth d has at most 2^(d+1) - 1 nodes; the lists of all levels lie one behind the
// other, a level's lists together are about as long as leaf_refs.  Both are checked on the device; a build that does not fit
// raises a flag and is repeated with more room.  Per attempt: refused()? then request(), the build, then overflowed() if it was.
class BuildCaps {
    size_t max_nodes_, n_tris_, want_nodes_, want_refs_;
    int attempt_ = 0;
public:
    struct Request { size_t nodes, refs; };
    // cap_nodes / cap_refs: what the last update ended with (0: none yet); n_nodes: of the tree the accel holds
    BuildCaps(size_t cap_nodes, size_t cap_refs, size_t n_nodes, size_t n_tris, int max_depth, bool new_topology)
        : max_nodes_((size_t(1) << (max_depth + 1)) - 1), n_tris_(n_tris) {
        const size_t first_refs = std::max<size_t>(4096, 2 * n_tris * size_t(std::min(max_depth, 12) + 2));
        want_nodes_ = cap_nodes ? cap_nodes : std::max<size_t>(1024, 4 * n_nodes);
        want_refs_ = cap_refs ? cap_refs : first_refs;
        if (new_topology && want_refs_ < first_refs) want_refs_ = first_refs;      // more triangles than the capacity was learnt on: no point in trying it
    }
    bool refused() const { return attempt_ > 16 || want_refs_ > 0x7FFFFFF0ull; }   // "tree too large for 32-bit node/triangle indices"
    Request request() {
        if (want_nodes_ > max_nodes_) want_nodes_ = max_nodes_;
        if (want_refs_ < n_tris_) want_refs_ = n_tris_;
        return {want_nodes_, want_refs_};
    }
    // raised: the cleared bits of BuildHdr::ok; need_*: what the level that did not fit needed; cap_*: what the attempt had
    void overflowed(uint32_t raised, size_t need_nodes, size_t need_refs, size_t cap_nodes, size_t cap_refs) {
        if (raised & dev::kBuildNodeOverflow) want_nodes_ = std::max(2 * cap_nodes, 2 * need_nodes);
        if (raised & dev::kBuildRefOverflow) want_refs_ = std::max(2 * cap_refs, 2 * need_refs);
        ++attempt_;
    }
};

// Whether occlusion stops at a triangle of this material: anything but a refractive one, an index past the table included.
inline bool opaque(const std::vector<DevMaterial> &materials, size_t material) {
    return !(material < materials.size() && materials[material].kind == RTK_MAT_REFRACTIVE);
}
// rtk_accel::has_refractive of a material table
inline bool any_refractive(const std::vector<DevMaterial> &materials) {
    for (const DevMaterial &m : materials) if (m.kind == RTK_MAT_REFRACTIVE) return true;
    return false;
}

// Occlusion through transmissive surfaces as ONE query against what is not transmissive (rtk.h, RTK_TRAVERSAL_FAST): the same
// nodes, a leaf's a / b its run in the opaque-only copy of the references; leaves left empty stay nodes and drop out of the leaf
// list, which holds node 0 as a leaf of nothing when no leaf is left.
struct Occluders {
    std::vector<DevNode> nodes, leaves;
    std::vector<uint32_t> dst;         // per leaf, in dev_nodes' order: its first slot in the opaque-only copy
    size_t n_opaque = 0;
};
// counts: opaque references per leaf, in dev_nodes' order
inline const char *number_occluders(const std::vector<DevNode> &dev_nodes, const std::vector<uint32_t> &counts, Occluders &out) {
    out = Occluders{};
    out.nodes = dev_nodes;
    for (DevNode &n : out.nodes) {
        if (n.b == DEV_INNER) continue;
        const size_t li = out.dst.size();
        if (li >= counts.size()) return "internal: a leaf without an opaque count";
        if (counts[li] > n.b) return "internal: a leaf's opaque count exceeds the leaf";
        out.dst.push_back(uint32_t(out.n_opaque));
        n.a = uint32_t(out.n_opaque); n.b = counts[li];
        out.n_opaque += n.b;
        if (n.b != 0u) out.leaves.push_back(n);
    }
    if (out.leaves.empty()) { DevNode n = out.nodes.empty() ? DevNode{} : out.nodes[0]; n.a = 0u; n.b = 0u; out.leaves.push_back(n); }
    return nullptr;
}

// The same from a tree whose references the host still holds, with the copy itself: one triangle (the first reference, if there
// is one) and id 0 when nothing is opaque, so that the pointers stay valid.
struct HostOccluders {
    Occluders tree;
    std::vector<DevTri> tris;
    std::vector<uint32_t> ids;
};
inline const char *host_occluders(const HostTree &t, const std::vector<DevMaterial> &materials, HostOccluders &out) {
    out = HostOccluders{};
    std::vector<uint32_t> counts;
    for (const DevNode &n : t.dev_nodes) {
        if (n.b == DEV_INNER) continue;
        const size_t first = out.tris.size();
        for (uint32_t r = n.a; r < n.a + n.b; ++r) {
            if (!opaque(materials, t.dev_shade[t.dev_tri_ids[r]].material)) continue;
            out.tris.push_back(t.dev_tris[r]); out.ids.push_back(t.dev_tri_ids[r]);
        }
        counts.push_back(uint32_t(out.tris.size() - first));
    }
    if (out.tris.empty()) { out.tris.push_back(t.dev_tris.empty() ? DevTri{} : t.dev_tris[0]); out.ids.push_back(0u); }
    return number_occluders(t.dev_nodes, counts, out.tree);
}

// What an update of the vertices needs of the topology: vertex ids per triangle over the concatenated vertex array, the
// vertex -> (triangle, corner) incidence lists and which triangles are opaque, from the scene an accel was built from.
// mesh_nverts: numbers, an update empties the meshes' vertices.
struct HostTopology {
    std::vector<uint32_t> index, inc_off, inc;
    std::vector<uint8_t> opaque;
};
inline const char *host_topology(const rtk_scene &scene, const std::vector<int32_t> &mesh_nverts, HostTopology &out) {
    const size_t nv = size_t(scene.n_vertices), nt = size_t(scene.n_triangles);
    if (nt * 3 > 0xFFFFFFF0ull || nv > 0xFFFFFFF0ull) return "scene too large for the device build's 32-bit indices";
    out.index.assign(nt * 3, 0u); out.inc_off.assign(nv + 1, 0u); out.inc.assign(nt * 3, 0u); out.opaque.assign(nt, uint8_t(1));
    size_t voff = 0, t = 0;
    for (size_t mi = 0; mi < scene.meshes.size(); ++mi) {
        const HostMesh &m = scene.meshes[mi];
        const uint8_t flag = opaque(scene.materials, size_t(m.material)) ? 1 : 0;
        if (mi >= mesh_nverts.size() || t + m.indices.size() / 3 > nt) return "internal: the accel's scene copy lost its topology";
        for (size_t ti = 0; ti < m.indices.size() / 3; ++ti, ++t) {
            for (size_t k = 0; k < 3; ++k) out.index[t * 3 + k] = uint32_t(voff + m.indices[ti * 3 + k]);
            out.opaque[t] = flag;
        }
        voff += size_t(mesh_nverts[mi]);
    }
    if (voff != nv || t != nt) return "internal: the accel's scene copy lost its topology";
    // Incidence lists by counting sort over (triangle, corner) in ascending order: each vertex's list ascends by triangle and
    // keeps duplicates, which is the order mesh.hpp:36-38 adds the face normals in (build.hip, k_build_normals).
    for (uint32_t v : out.index) {
        if (v >= nv) return "internal: the accel's scene copy lost its topology";
        out.inc_off[size_t(v) + 1] += 1u;
    }
    for (size_t v = 0; v < nv; ++v) out.inc_off[v + 1] += out.inc_off[v];
    std::vector<uint32_t> cur(out.inc_off.begin(), out.inc_off.end() - 1);
    for (size_t e = 0; e < nt * 3; ++e) out.inc[cur[out.index[e]]++] = uint32_t(e);
    return nullptr;
}

}  // namespace rtk
