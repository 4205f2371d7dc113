// C-ABI, dynamic geometry: rtk_accel_update_vertices and rtk_accel_update_geometry rebuild the kd-tree on the device (build.hip,
// for new triangle lists topology.hip first) and swap it in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "accel.hpp"

using namespace rtk;

// What every update needs once: the event later work waits for.  (Buffers that have to grow do so by grow_bytes; freeing
// synchronises the device: this is the "second block" of an update, taken only then.)
int rtk::ensure_update_common(rtk_accel *a) {
    RTK_MEM(a->geom_ready.ensure());
    return RTK_OK;
}

namespace {

// What an update of the vertices needs of the topology: vertex ids per triangle over the concatenated vertex array, the
// vertex -> (triangle, corner) incidence lists and which triangles are opaque.  Made here, on the host, from the scene the accel
// was built from, on its first update; rtk_accel_update_geometry replaces them by what topology.hip makes of its triangle lists.
int ensure_update_static(rtk_accel *a) {
    RTK_TRY(ensure_update_common(a));
    if (a->up_static) return RTK_OK;
    const size_t nv = size_t(a->scene.n_vertices), nt = size_t(a->scene.n_triangles);
    if (nt * 3 > 0xFFFFFFF0ull || nv > 0xFFFFFFF0ull) return fail(RTK_ERR_INVALID, "scene too large for the device build's 32-bit indices");
    std::vector<uint32_t> index(nt * 3), off(nv + 1, 0u), inc(nt * 3);
    std::vector<uint8_t> opaque(nt, uint8_t(1));
    size_t voff = 0, t = 0;
    for (size_t mi = 0; mi < a->scene.meshes.size(); ++mi) {
        const HostMesh &m = a->scene.meshes[mi];
        const bool refr = size_t(m.material) < a->scene.materials.size() && a->scene.materials[size_t(m.material)].kind == RTK_MAT_REFRACTIVE;
        for (size_t ti = 0; ti < m.indices.size() / 3; ++ti, ++t) {
            for (size_t k = 0; k < 3; ++k) index[t * 3 + k] = uint32_t(voff + m.indices[ti * 3 + k]);
            opaque[t] = refr ? 0 : 1;
        }
        voff += size_t(a->mesh_nverts[mi]);                                  // (a number: an update empties m.vertices)
    }
    if (voff != nv || t != nt) return fail(RTK_ERR_INVALID, "internal: the accel's scene copy lost its topology");
    // Incidence lists by counting sort over (triangle, corner) in ascending order: each vertex's list ascends by triangle and
    // keeps duplicates, which is the order mesh.hpp:36-38 adds the face normals in (build.hip, k_build_normals).
    for (uint32_t v : index) off[size_t(v) + 1] += 1u;
    for (size_t v = 0; v < nv; ++v) off[v + 1] += off[v];
    std::vector<uint32_t> cur(off.begin(), off.end() - 1);
    for (size_t e = 0; e < nt * 3; ++e) inc[cur[index[e]]++] = uint32_t(e);
    // (a call that failed half way left what it had made: made once, never twice; a failed upload leaves its buffer empty)
    TopoBufs &A = a->topo;
    if (!A.index.get()) RTK_TRY(upload(index, A.index));
    if (!A.inc_off.get()) RTK_TRY(upload(off, A.inc_off));
    if (!A.inc.get()) RTK_TRY(upload(inc, A.inc));
    if (!A.opaque.get()) RTK_TRY(upload(opaque, A.opaque));
    a->up_static = true;
    return RTK_OK;
}

// New triangle lists for an update (null: the vertices alone moved).
struct NewTopology {
    const uint32_t *d_indices;      // device, mesh-local, not validated
    const int32_t *mesh_ntris;      // host, validated by check_counts
    uint32_t n_tris;
};

// Everything topology.hip needs beside the caller's arrays: room for its tables in the spare set, its scratch, the per-vertex uvs
// (once) and the per-mesh rows of this call, sent off on `s` through the pinned stage.
int prepare_topology(rtk_accel *a, const NewTopology &N, hipStream_t s, dev::TopoArgs &T) {
    const size_t nv = size_t(a->scene.n_vertices), nt = N.n_tris, nm = a->mesh_nverts.size();
    const bool textured = !a->scene.textures.empty();
    TopoBufs &sp = a->topo_spare;
    RTK_MEM(sp.index.reserve(nt * 3, grow_bytes()));
    RTK_MEM(sp.inc_off.reserve(nv + 1, grow_bytes()));
    RTK_MEM(sp.inc.reserve(nt * 3, grow_bytes()));
    RTK_MEM(sp.opaque.reserve(nt, grow_bytes()));
    if (textured) RTK_MEM(sp.tri_uv.reserve(nt, grow_bytes()));
    size_t temp_bytes = 0;
    RTK_MEM(a->topo_keys.reserve(nt * 3, grow_bytes()));
    RTK_HIP_AS(topology_temp_bytes(uint32_t(nt), uint32_t(nv), &temp_bytes), "size the incidence sort");
    RTK_MEM(a->topo_temp.reserve(temp_bytes, grow_bytes()));
    RTK_MEM(a->topo_meshes.reserve(nm + 1));                                // (once: the number of meshes is fixed)
    if (textured && !a->topo_vert_uv.get()) {                                     // kdtree.cpp:283-: a mesh without uvs has zeros
        std::vector<float> uv(std::max<size_t>(1, nv) * 2, 0.0f);
        size_t voff = 0;
        for (size_t mi = 0; mi < nm; ++mi) {
            const std::vector<float> &mu = a->scene.meshes[mi].uvs;
            const size_t n = std::min(mu.size(), size_t(a->mesh_nverts[mi]) * 2);
            if (n > 0) std::memcpy(uv.data() + voff * 2, mu.data(), n * sizeof(float));
            voff += size_t(a->mesh_nverts[mi]);
        }
        RTK_TRY(upload(uv, a->topo_vert_uv));
    }
    RTK_MEM(a->up_stage.reserve((nm + 1) * sizeof(dev::TopoMesh), grow_bytes()));
    dev::TopoMesh *rows = reinterpret_cast<dev::TopoMesh *>(a->up_stage.get());
    uint32_t tri = 0u, vert = 0u;
    for (size_t mi = 0; mi <= nm; ++mi) {
        dev::TopoMesh r{};
        r.tri_begin = tri; r.vert_begin = vert;
        if (mi < nm) {
            const int32_t mat = a->scene.meshes[mi].material;
            r.n_verts = uint32_t(a->mesh_nverts[mi]);
            r.material = uint32_t(mat);
            r.opaque = (size_t(mat) < a->scene.materials.size() && a->scene.materials[size_t(mat)].kind == RTK_MAT_REFRACTIVE) ? 0u : 1u;
            tri += uint32_t(N.mesh_ntris[mi]); vert += r.n_verts;
        }
        rows[mi] = r;
    }
    RTK_HIP(hipMemcpyAsync(a->topo_meshes.get(), rows, (nm + 1) * sizeof(dev::TopoMesh), hipMemcpyHostToDevice, s));
    T.indices = N.d_indices; T.meshes = a->topo_meshes.get();
    T.n_meshes = uint32_t(nm); T.n_tris = uint32_t(nt); T.n_verts = uint32_t(nv);
    T.vert_uv = textured ? a->topo_vert_uv.get() : nullptr;
    T.index = sp.index.get(); T.inc_off = sp.inc_off.get(); T.inc = sp.inc.get();
    T.opaque = sp.opaque.get();
    T.shade = a->geom_spare.shade.get();
    T.tri_uv = textured ? sp.tri_uv.get() : nullptr;
    T.keys = a->topo_keys.get(); T.temp = a->topo_temp.get(); T.temp_bytes = temp_bytes;
    T.hdr = nullptr;                                                        // (the caller's: the table may still be allocated)
    return RTK_OK;
}

// The one path of both updates.  `topo` null: the vertices moved and the active topology tables describe the triangles.  Else the
// tables are made first, into the spare set, and become the active ones where the geometry does: at the very end.
int update_impl(rtk_accel *a, const float *d_verts, const NewTopology *topo, hipStream_t s) {
    if (topo) RTK_TRY(ensure_update_common(a));
    else RTK_TRY(ensure_update_static(a));
    const uint32_t nv = uint32_t(a->scene.n_vertices), nt = topo ? topo->n_tris : uint32_t(a->scene.n_triangles);
    const bool occl = a->occl_on;
    // per-triangle scratch and the new shading records
    GeomBufs &sp = a->geom_spare;
    RTK_MEM(a->up_tris.reserve(nt, grow_bytes()));
    RTK_MEM(a->up_tbox.reserve(size_t(nt) * 6, grow_bytes()));
    RTK_MEM(sp.shade.reserve(nt, grow_bytes()));
    dev::TopoArgs TA{};
    if (topo) RTK_TRY(prepare_topology(a, *topo, s, TA));
    const uint32_t *t_index = topo ? TA.index : a->topo.index.get(), *t_inc_off = topo ? TA.inc_off : a->topo.inc_off.get(), *t_inc = topo ? TA.inc : a->topo.inc.get();
    const uint8_t *t_opaque = topo ? TA.opaque : a->topo.opaque.get();
    // Capacities of the build: a tree of depth d has at most 2^(d+1) - 1 nodes; the lists of all levels lie one behind the
    // other, a level's lists together are about as long as leaf_refs.  Both are checked on the device; a build that does not fit
    // raises a flag, and is repeated with more room.
    const size_t max_nodes = (size_t(1) << (a->params.max_depth + 1)) - 1;
    // (the table and the reference lists are sized exactly: their capacities are the build's, cap_nodes behind the header)
    auto table_bytes = [](size_t nodes) { return sizeof(dev::BuildHdr) + nodes * sizeof(dev::BuildNode); };
    auto cap_nodes = [&] { return a->up_table.get() ? (a->up_table.capacity() - sizeof(dev::BuildHdr)) / sizeof(dev::BuildNode) : size_t(0); };
    auto cap_refs = [&] { return a->up_ref_node.capacity(); };
    size_t want_nodes = cap_nodes() ? cap_nodes() : std::max<size_t>(1024, 4 * a->tree.dev_nodes.size());
    const size_t first_refs = std::max<size_t>(4096, 2 * size_t(nt) * size_t(std::min(a->params.max_depth, 12) + 2));
    size_t want_refs = cap_refs() ? cap_refs() : first_refs;
    if (topo && want_refs < first_refs) want_refs = first_refs;             // more triangles than the capacity was learnt on: no point in trying it
    dev::BuildHdr hdr;
    for (int attempt = 0;; ++attempt) {
        if (want_nodes > max_nodes) want_nodes = max_nodes;
        if (attempt > 16 || want_refs > 0x7FFFFFF0ull) return fail(RTK_ERR_INVALID, "tree too large for 32-bit node/triangle indices");
        if (want_refs < nt) want_refs = nt;
        RTK_MEM(a->up_table.reserve(table_bytes(want_nodes), set_exactly()));
        RTK_MEM(a->up_table_host.reserve(table_bytes(want_nodes), set_exactly()));
        RTK_MEM(a->up_ref_id.reserve(want_refs, set_exactly()));
        RTK_MEM(a->up_ref_node.reserve(want_refs, set_exactly()));
        dev::BuildArgs B;
        B.verts = d_verts; B.n_verts = nv; B.n_tris = nt;
        B.index = t_index; B.inc_off = t_inc_off; B.inc = t_inc;
        B.opaque = occl ? t_opaque : nullptr;
        B.shade = sp.shade.get();
        B.shade_old = topo ? B.shade : a->geom.shade.get();                          // (topology.hip wrote mesh / material into the new records)
        B.tris = a->up_tris.get(); B.tbox = a->up_tbox.get();
        B.ref_id = a->up_ref_id.get(); B.ref_node = a->up_ref_node.get();
        B.cap_refs = uint32_t(cap_refs()); B.cap_nodes = uint32_t(cap_nodes());
        B.max_depth = a->params.max_depth; B.max_leaf = a->params.max_leaf_size;
        B.hdr = reinterpret_cast<dev::BuildHdr *>(a->up_table.get());
        B.nodes = reinterpret_cast<dev::BuildNode *>(a->up_table.get() + sizeof(dev::BuildHdr));
        TA.hdr = B.hdr;
        // (the topology tables do not depend on the capacities: a repeat keeps them.  Their flag is read after the first attempt.)
        RTK_HIP_AS(launch_build(B, topo && attempt == 0 ? &TA : nullptr, s), "launch device build");
        // the one place an update blocks the host: flags, sizes and the node table
        RTK_HIP(hipMemcpyAsync(a->up_table_host.get(), a->up_table.get(), table_bytes(cap_nodes()), hipMemcpyDeviceToHost, s));
        RTK_HIP(hipStreamSynchronize(s));
        std::memcpy(&hdr, a->up_table_host.get(), sizeof(hdr));
        const uint32_t raised = ~hdr.ok;
        if (raised & dev::kBuildNonFinite) return fail(RTK_ERR_INVALID, "vertices must be finite");
        if (raised & dev::kBuildBadIndex) return fail(RTK_ERR_INVALID, "an index is not a vertex of its mesh");
        if ((raised & (dev::kBuildRefOverflow | dev::kBuildNodeOverflow)) == 0u) break;
        if (raised & dev::kBuildNodeOverflow) want_nodes = std::max<size_t>(2 * cap_nodes(), 2 * size_t(hdr.need_nodes));
        if (raised & dev::kBuildRefOverflow) want_refs = std::max<size_t>(2 * cap_refs(), 2 * size_t(hdr.need_refs));
    }
    // numbering on the host (kdtree.cpp): reference order, traversal order with skip links, leaf offsets in both, FAST orders
    const dev::BuildNode *bn = reinterpret_cast<const dev::BuildNode *>(a->up_table_host.get() + sizeof(dev::BuildHdr));
    HostTree T;
    std::vector<dev::GatherLeaf> gather;
    tree_from_build_nodes(bn, T, gather);
    if (T.nodes.size() != hdr.n_nodes) return fail(RTK_ERR_INVALID, "internal: the device build's node table is not a tree");
    if (a->fast_traversal) build_fast_leaf_orders(T);
    size_t n_refs = 0;
    for (const dev::GatherLeaf &g : gather) n_refs += g.count;
    if (n_refs > 0x7FFFFFFFull) return fail(RTK_ERR_INVALID, "tree too large for 32-bit node/triangle indices");
    std::vector<DevNode> onodes, oleaves;
    size_t n_opaque = 0;
    if (occl) {                                                         // as ensure_device: the same nodes, their leaves without the transmissive triangles
        onodes = T.dev_nodes;
        size_t li = 0;
        for (DevNode &n : onodes) {
            if (n.b == DEV_INNER) continue;
            dev::GatherLeaf &g = gather[li++];                          // (dev_leaves and gather are both the leaves in dev_nodes' order)
            g.dst_occl = uint32_t(n_opaque);
            n.a = uint32_t(n_opaque); n.b = g.pad[0];
            n_opaque += g.pad[0];
            if (n.b != 0u) oleaves.push_back(n);
        }
        if (oleaves.empty()) { DevNode n = onodes[0]; n.a = 0u; n.b = 0u; oleaves.push_back(n); }
    }
    for (dev::GatherLeaf &g : gather) g.pad[0] = 0u;
    // room in the spare set
    RTK_MEM(sp.nodes.reserve(T.dev_nodes.size(), grow_bytes()));
    RTK_MEM(sp.leaves.reserve(T.dev_leaves.size(), grow_bytes()));
    if (a->fast_traversal) RTK_MEM(sp.leaves_fast.reserve(T.dev_leaves_fast.size(), grow_bytes()));
    RTK_MEM(sp.tris.reserve(n_refs, grow_bytes()));
    RTK_MEM(sp.tri_ids.reserve(n_refs, grow_bytes()));
    RTK_MEM(sp.leaf_refs.reserve(n_refs, grow_bytes()));
    if (occl) {
        RTK_MEM(sp.occl_nodes.reserve(onodes.size(), grow_bytes()));
        RTK_MEM(sp.occl_leaves.reserve(oleaves.size(), grow_bytes()));
        RTK_MEM(sp.occl_tris.reserve(std::max<size_t>(1, n_opaque), grow_bytes()));
        RTK_MEM(sp.occl_ids.reserve(std::max<size_t>(1, n_opaque), grow_bytes()));
    }
    RTK_MEM(a->up_gather.reserve(gather.size(), grow_bytes()));
    // the small tables go up through one pinned buffer (the copies are stream-ordered and the host does not wait for them)
    struct Up { const void *src; void *dst; size_t bytes; };
    const Up ups[] = {
        {T.dev_nodes.data(), sp.nodes.get(), T.dev_nodes.size() * sizeof(DevNode)},
        {T.dev_leaves.data(), sp.leaves.get(), T.dev_leaves.size() * sizeof(DevNode)},
        {T.dev_leaves_fast.data(), sp.leaves_fast.get(), a->fast_traversal ? T.dev_leaves_fast.size() * sizeof(DevNode) : 0},
        {gather.data(), a->up_gather.get(), gather.size() * sizeof(dev::GatherLeaf)},
        {onodes.data(), sp.occl_nodes.get(), onodes.size() * sizeof(DevNode)},
        {oleaves.data(), sp.occl_leaves.get(), oleaves.size() * sizeof(DevNode)},
    };
    size_t total = 0;
    for (const Up &u : ups) total += (u.bytes + 63) & ~size_t(63);
    RTK_MEM(a->up_stage.reserve(total, grow_bytes()));
    uint8_t *const stage = a->up_stage.get();
    size_t at = 0;
    for (const Up &u : ups) {
        if (u.bytes == 0) continue;
        std::memcpy(stage + at, u.src, u.bytes);
        RTK_HIP(hipMemcpyAsync(u.dst, stage + at, u.bytes, hipMemcpyHostToDevice, s));
        at += (u.bytes + 63) & ~size_t(63);
    }
    dev::GatherArgs G;
    G.leaves = a->up_gather.get(); G.n_leaves = uint32_t(gather.size());
    G.ref_id = a->up_ref_id.get(); G.tris_in = a->up_tris.get(); G.opaque = occl ? t_opaque : nullptr;
    G.tris = sp.tris.get(); G.tri_ids = sp.tri_ids.get(); G.leaf_refs = sp.leaf_refs.get();
    G.occl_tris = sp.occl_tris.get(); G.occl_ids = sp.occl_ids.get();
    RTK_HIP_AS(launch_gather(G, s), "launch k_build_gather");
    if (occl && n_opaque == 0) {                                        // nothing opaque: keep the pointers valid, as ensure_device does
        if (n_refs > 0) RTK_HIP(hipMemcpyAsync(sp.occl_tris.get(), sp.tris.get(), sizeof(DevTri), hipMemcpyDeviceToDevice, s));
        else RTK_HIP(hipMemsetAsync(sp.occl_tris.get(), 0, sizeof(DevTri), s));
        RTK_HIP(hipMemsetAsync(sp.occl_ids.get(), 0, sizeof(uint32_t), s));
    }
    RTK_HIP(hipEventRecord(a->geom_ready.get(), s));
    // ---- nothing below fails: swap the sets and bring the host's picture of the accel up to date
    a->geom.swap(sp, a->fast_traversal, occl);
    if (topo) {
        a->topo.swap(a->topo_spare, TA.tri_uv != nullptr);
        a->up_static = true;
        a->scene.n_triangles = int32_t(nt);
        a->mesh_ntris.assign(topo->mesh_ntris, topo->mesh_ntris + a->mesh_ntris.size());
        // the host's copy of the old lists, and what was derived from them: dropped, as the vertices are below
        for (HostMesh &m : a->scene.meshes) std::vector<uint32_t>().swap(m.indices);
        std::vector<DevTriUv>().swap(a->tree.dev_tri_uv);
    }
    a->geom_pending = true;
    a->occl_n_leaves = occl ? uint32_t(oleaves.size()) : 0u;
    a->tree.nodes = std::move(T.nodes);
    a->tree.dev_nodes = std::move(T.dev_nodes);
    a->tree.dev_leaves = std::move(T.dev_leaves);
    a->tree.dev_leaves_fast = std::move(T.dev_leaves_fast);
    a->tree.depth = T.depth;
    // what the host held per triangle, per reference and per vertex describes the old geometry: dropped, not left to lie
    // (rtk_accel_tree_dump fetches leaf_refs from the device)
    std::vector<HostTriangle>().swap(a->tree.triangles);
    std::vector<int32_t>().swap(a->tree.leaf_refs);
    std::vector<DevTri>().swap(a->tree.dev_tris);
    std::vector<uint32_t>().swap(a->tree.dev_tri_ids);
    std::vector<DevShade>().swap(a->tree.dev_shade);
    for (HostMesh &m : a->scene.meshes) { std::vector<Vec3>().swap(m.vertices); std::vector<Vec3>().swap(m.vertex_normals); }
    a->refs_on_device = true;
    a->n_leaf_refs_dev = int32_t(n_refs);
    a->coords_small = (~hdr.ok & dev::kBuildCoordsBig) == 0u;
    a->stream_slices_auto = stream_slices_for(a->tree);
    // the launch order learnt from the old silhouette and the engines' trial on it say nothing about the new geometry
    a->fb.forget();
    for (rtk_cost_feedback &f : a->fb_views) f.forget();
    for (rtk_cost_feedback &f : a->fb_regions) f.forget();
    a->trial.abandon();
    return RTK_OK;
}

bool any_triangles(const rtk_accel *a, const int32_t *mesh_ntris) {
    for (size_t mi = 0; mi < a->mesh_nverts.size(); ++mi) if (mesh_ntris[mi] > 0) return true;
    return false;
}

// The counts of an update_geometry call, before anything is sized by them.
int check_counts(const rtk_accel *a, const int32_t *mesh_ntris, uint32_t &total) {
    uint64_t sum = 0;
    for (size_t mi = 0; mi < a->mesh_nverts.size(); ++mi) {
        if (mesh_ntris[mi] < 0) return fail(RTK_ERR_INVALID, "a negative triangle count");
        if (mesh_ntris[mi] > 0 && a->mesh_nverts[mi] <= 0) return fail(RTK_ERR_INVALID, "triangles on a mesh without vertices");
        sum += uint64_t(mesh_ntris[mi]);
    }
    if (sum * 3 > 0xFFFFFFF0ull || sum > 0x7FFFFFFFull) return fail(RTK_ERR_INVALID, "too many triangles for the device build's 32-bit indices");
    total = uint32_t(sum);
    return RTK_OK;
}

}  // namespace

int rtk::remake_occluders(rtk_accel *a, const std::vector<DevMaterial> &materials, const DevMaterial *d_materials, hipStream_t s) {
    auto refractive = [](const DevMaterial &m) { return m.kind == RTK_MAT_REFRACTIVE; };
    bool any = false, set_changed = false;
    for (size_t i = 0; i < materials.size(); ++i) {
        any = any || refractive(materials[i]);
        if (refractive(materials[i]) != refractive(a->scene.materials[i])) set_changed = true;
    }
    const bool tree = a->fast_traversal && a->knobs.fast_occluders && set_changed;
    if (!tree && !(a->topo.opaque.get() && set_changed)) return RTK_OK;
    RTK_TRY(ensure_update_common(a));
    dev::OcclArgs O{};
    O.materials = d_materials; O.n_materials = uint32_t(materials.size());
    O.shade = a->geom.shade.get(); O.n_tris = uint32_t(a->scene.n_triangles);
    if (tree && any) {
        // the leaves of the active tree, in dev_nodes' order: as ensure_device and update_impl walk them
        const std::vector<DevNode> &nodes = a->tree.dev_nodes;
        std::vector<dev::OcclLeaf> leaves;
        for (const DevNode &n : nodes) if (n.b != DEV_INNER) leaves.push_back(dev::OcclLeaf{n.a, n.b, 0u, 0u});
        const size_t n_refs = a->refs_on_device ? size_t(a->n_leaf_refs_dev) : a->tree.dev_tris.size();
        for (const dev::OcclLeaf &l : leaves)
            if (size_t(l.first) + l.count > n_refs) return fail(RTK_ERR_INVALID, "internal: a leaf runs past the accel's references");
        const size_t nl = leaves.size();
        RTK_MEM(a->st_leaves.reserve(nl, grow_bytes()));
        RTK_MEM(a->st_counts.reserve(nl, grow_bytes()));
        O.leaves = a->st_leaves.get(); O.n_leaves = uint32_t(nl); O.n_refs = uint32_t(n_refs);
        O.tris = a->geom.tris.get(); O.tri_ids = a->geom.tri_ids.get(); O.counts = a->st_counts.get();
        std::vector<uint32_t> counts(nl, 0u);
        if (nl > 0) {
            RTK_HIP(hipMemcpyAsync(a->st_leaves.get(), leaves.data(), nl * sizeof(dev::OcclLeaf), hipMemcpyHostToDevice, s));
            RTK_HIP_AS(launch_occl_count(O, s), "launch k_occl_count");
            // the one place the call blocks after entry: one count per leaf
            RTK_HIP(hipMemcpyAsync(counts.data(), a->st_counts.get(), nl * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
            RTK_HIP(hipStreamSynchronize(s));
        }
        // as ensure_device / update_impl: the same nodes, a leaf's a / b its run in the opaque copy, empty leaves kept as nodes
        // and dropped from the leaf list
        std::vector<DevNode> onodes = nodes, oleaves;
        size_t n_opaque = 0, li = 0;
        for (DevNode &n : onodes) {
            if (n.b == DEV_INNER) continue;
            const uint32_t c = counts[li];
            if (c > leaves[li].count) return fail(RTK_ERR_INVALID, "internal: a leaf's opaque count exceeds the leaf");
            leaves[li++].dst = uint32_t(n_opaque);
            n.a = uint32_t(n_opaque); n.b = c;
            n_opaque += c;
            if (n.b != 0u) oleaves.push_back(n);
        }
        if (oleaves.empty()) { DevNode n = onodes.empty() ? DevNode{} : onodes[0]; n.a = 0u; n.b = 0u; oleaves.push_back(n); }
        GeomBufs &sp = a->geom_spare;
        RTK_MEM(sp.occl_nodes.reserve(onodes.size(), grow_bytes()));
        RTK_MEM(sp.occl_leaves.reserve(oleaves.size(), grow_bytes()));
        RTK_MEM(sp.occl_tris.reserve(std::max<size_t>(1, n_opaque), grow_bytes()));
        RTK_MEM(sp.occl_ids.reserve(std::max<size_t>(1, n_opaque), grow_bytes()));
        // (pageable sources: these copies return when the data has left the host vectors)
        if (!onodes.empty()) RTK_HIP(hipMemcpyAsync(sp.occl_nodes.get(), onodes.data(), onodes.size() * sizeof(DevNode), hipMemcpyHostToDevice, s));
        RTK_HIP(hipMemcpyAsync(sp.occl_leaves.get(), oleaves.data(), oleaves.size() * sizeof(DevNode), hipMemcpyHostToDevice, s));
        if (nl > 0) RTK_HIP(hipMemcpyAsync(a->st_leaves.get(), leaves.data(), nl * sizeof(dev::OcclLeaf), hipMemcpyHostToDevice, s));
        O.occl_tris = sp.occl_tris.get(); O.occl_ids = sp.occl_ids.get(); O.cap = uint32_t(n_opaque);
        if (n_opaque > 0) RTK_HIP_AS(launch_occl_gather(O, s), "launch k_occl_gather");
        else {                                                              // nothing opaque: keep the pointers valid, as ensure_device does
            if (n_refs > 0) RTK_HIP(hipMemcpyAsync(sp.occl_tris.get(), a->geom.tris.get(), sizeof(DevTri), hipMemcpyDeviceToDevice, s));
            else RTK_HIP(hipMemsetAsync(sp.occl_tris.get(), 0, sizeof(DevTri), s));
            RTK_HIP(hipMemsetAsync(sp.occl_ids.get(), 0, sizeof(uint32_t), s));
        }
        if (a->topo.opaque.get()) { O.opaque = a->topo.opaque.get(); RTK_HIP_AS(launch_occl_flags(O, s), "launch k_occl_flags"); }
        RTK_HIP(hipStreamSynchronize(s));                                   // (the host vectors above go out of scope)
        RTK_HIP(hipEventRecord(a->geom_ready.get(), s));
        // ---- nothing below fails
        a->geom.swap_occl(sp);
        a->occl_n_leaves = uint32_t(oleaves.size());
        a->occl_on = true;
        a->geom_pending = true;
        return RTK_OK;
    }
    // the flags alone; a FAST accel that lost its last refractive material keeps the buffers for the next time
    if (a->topo.opaque.get()) {
        O.opaque = a->topo.opaque.get();
        RTK_HIP_AS(launch_occl_flags(O, s), "launch k_occl_flags");
        RTK_HIP(hipEventRecord(a->geom_ready.get(), s));
        a->geom_pending = true;
    }
    if (tree) { a->occl_on = false; a->occl_n_leaves = 0u; }
    return RTK_OK;
}

int rtk_accel_update_vertices_device(rtk_accel *a, const float *d_vertices, void *hip_stream) {
    if (!a || !d_vertices) return fail(RTK_ERR_INVALID, "null accel or vertices");
    std::lock_guard<std::mutex> lock(a->mu);
    try {
        RTK_TRY(ensure_device(a));
        // entry: nothing issued earlier on this accel, on whatever stream, may still read a buffer the update rewrites
        RTK_HIP(hipDeviceSynchronize());
        a->geom_pending = false;
        return update_impl(a, d_vertices, nullptr, static_cast<hipStream_t>(hip_stream));
    } catch (const std::exception &e) { return fail(RTK_ERR_INVALID, e.what()); }
}

int rtk_accel_update_vertices(rtk_accel *a, const float *vertices) {
    if (!a || !vertices) return fail(RTK_ERR_INVALID, "null accel or vertices");
    std::lock_guard<std::mutex> lock(a->mu);
    try {
        RTK_TRY(ensure_device(a));
        const size_t n = size_t(a->scene.n_vertices) * 3;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(vertices[i])) return fail(RTK_ERR_INVALID, "vertices must be finite");
        RTK_HIP(hipDeviceSynchronize());
        a->geom_pending = false;
        RTK_MEM(a->up_verts.reserve(n));                                    // (once: the vertex count never changes)
        if (n > 0) RTK_HIP(hipMemcpy(a->up_verts.get(), vertices, n * sizeof(float), hipMemcpyHostToDevice));
        return update_impl(a, a->up_verts.get(), nullptr, nullptr);
    } catch (const std::exception &e) { return fail(RTK_ERR_INVALID, e.what()); }
}

int rtk_accel_update_geometry_device(rtk_accel *a, const float *d_vertices, const uint32_t *d_indices, const int32_t *mesh_ntris, void *hip_stream) {
    if (!a || !d_vertices || !mesh_ntris) return fail(RTK_ERR_INVALID, "null accel, vertices or mesh_ntris");
    std::lock_guard<std::mutex> lock(a->mu);
    try {
        if (!d_indices && any_triangles(a, mesh_ntris)) return fail(RTK_ERR_INVALID, "null indices");
        RTK_TRY(ensure_device(a));
        NewTopology N{d_indices, mesh_ntris, 0u};
        RTK_TRY(check_counts(a, mesh_ntris, N.n_tris));
        RTK_HIP(hipDeviceSynchronize());
        a->geom_pending = false;
        return update_impl(a, d_vertices, &N, static_cast<hipStream_t>(hip_stream));
    } catch (const std::exception &e) { return fail(RTK_ERR_INVALID, e.what()); }
}

// validate + stage + the device path
int rtk_accel_update_geometry(rtk_accel *a, const float *vertices, const uint32_t *indices, const int32_t *mesh_ntris) {
    if (!a || !vertices || !mesh_ntris) return fail(RTK_ERR_INVALID, "null accel, vertices or mesh_ntris");
    std::lock_guard<std::mutex> lock(a->mu);
    try {
        if (!indices && any_triangles(a, mesh_ntris)) return fail(RTK_ERR_INVALID, "null indices");
        RTK_TRY(ensure_device(a));
        NewTopology N{nullptr, mesh_ntris, 0u};
        RTK_TRY(check_counts(a, mesh_ntris, N.n_tris));
        const size_t n = size_t(a->scene.n_vertices) * 3;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(vertices[i])) return fail(RTK_ERR_INVALID, "vertices must be finite");
        size_t t = 0;
        for (size_t mi = 0; mi < a->mesh_nverts.size(); ++mi) {
            const uint32_t limit = uint32_t(a->mesh_nverts[mi]);
            for (size_t e = t * 3, end = (t + size_t(mesh_ntris[mi])) * 3; e < end; ++e)
                if (indices[e] >= limit) return fail(RTK_ERR_INVALID, "an index is not a vertex of its mesh");
            t += size_t(mesh_ntris[mi]);
        }
        RTK_HIP(hipDeviceSynchronize());
        a->geom_pending = false;
        RTK_MEM(a->up_verts.reserve(n));
        if (n > 0) RTK_HIP(hipMemcpy(a->up_verts.get(), vertices, n * sizeof(float), hipMemcpyHostToDevice));
        RTK_MEM(a->up_idx_stage.reserve(size_t(N.n_tris) * 3, grow_bytes()));
        if (N.n_tris > 0u) RTK_HIP(hipMemcpy(a->up_idx_stage.get(), indices, size_t(N.n_tris) * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
        N.d_indices = a->up_idx_stage.get();
        return update_impl(a, a->up_verts.get(), &N, nullptr);
    } catch (const std::exception &e) { return fail(RTK_ERR_INVALID, e.what()); }
}
