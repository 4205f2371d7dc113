// C-ABI, dynamic geometry: rtk_accel_update_vertices and rtk_accel_update_geometry rebuild the kd-tree on the device (build.hip,
// for new triangle lists topology.hip first) and swap it in.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <mutex>

#include "accel.hpp"

using namespace rtk;

// (Buffers that have to grow do so by grow_bytes; freeing synchronises the device: this is the "second block" of an update, taken
// only then.)
// The topology tables of an update of the vertices (update_plan.hpp, host_topology): made on the host from the scene the accel
// was built from, on its first update; rtk_accel_update_geometry replaces them by what topology.hip makes of its triangle lists.
int rtk::ensure_update_static(rtk_accel *a) {
    if (a->up_static) return RTK_OK;
    HostTopology H;
    if (const char *why = host_topology(a->scene, a->mesh_nverts, H)) return fail(RTK_ERR_INVALID, why);
    // (a call that failed half way left what it had made: made once, never twice; a failed upload leaves its buffer empty)
    TopoBufs &A = a->topo;
    if (!A.index.get()) RTK_TRY(upload(H.index, A.index));
    if (!A.inc_off.get()) RTK_TRY(upload(H.inc_off, A.inc_off));
    if (!A.inc.get()) RTK_TRY(upload(H.inc, A.inc));
    if (!A.opaque.get()) RTK_TRY(upload(H.opaque, A.opaque));
    a->up_static = true;
    return RTK_OK;
}

namespace {

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
    if (textured) RTK_TRY(ensure_vert_uv_dev(a));                           // the CURRENT per-vertex uvs (rtk_accel_set_uvs)
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
            r.opaque = opaque(a->scene.materials, size_t(mat)) ? 1u : 0u;
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

// Nothing opaque: the opaque-only copy in `sp` holds one triangle (the first reference, if there is one) and id 0, as
// host_occluders makes it, so that the pointers stay valid.
int occl_placeholder(GeomBufs &sp, const DevTri *tris, size_t n_refs, hipStream_t s) {
    if (n_refs > 0) RTK_HIP(hipMemcpyAsync(sp.occl_tris.get(), tris, sizeof(DevTri), hipMemcpyDeviceToDevice, s));
    else RTK_HIP(hipMemsetAsync(sp.occl_tris.get(), 0, sizeof(DevTri), s));
    RTK_HIP(hipMemsetAsync(sp.occl_ids.get(), 0, sizeof(uint32_t), s));
    return RTK_OK;
}

int reserve_occluders(GeomBufs &sp, const Occluders &o) {
    RTK_MEM(sp.occl_nodes.reserve(o.nodes.size(), grow_bytes()));
    RTK_MEM(sp.occl_leaves.reserve(o.leaves.size(), grow_bytes()));
    RTK_MEM(sp.occl_tris.reserve(std::max<size_t>(1, o.n_opaque), grow_bytes()));
    RTK_MEM(sp.occl_ids.reserve(std::max<size_t>(1, o.n_opaque), grow_bytes()));
    return RTK_OK;
}

// One update on its way through the steps of update_impl.  `topo` null: the vertices moved and the active topology tables
// describe the triangles.  Else the tables are made first, into the spare set, and become the active ones where the geometry
// does: at the very end.
struct Update {
    rtk_accel *a;
    const float *d_verts;
    const NewTopology *topo;
    hipStream_t s;
    uint32_t nt;                        // triangles of the new geometry
    const TopoBufs &tables;             // the topology the build reads
    dev::TopoArgs TA{};
    dev::BuildHdr hdr{};                // of the build that fitted
    HostTree T;                         // its tree, numbered
    std::vector<dev::GatherLeaf> gather;
    Occluders occl;                     // empty without an opaque-only tree
    size_t n_refs = 0;
    Update(rtk_accel *a_, const float *d_verts_, const NewTopology *topo_, hipStream_t s_)
        : a(a_), d_verts(d_verts_), topo(topo_), s(s_), nt(topo_ ? topo_->n_tris : uint32_t(a_->scene.n_triangles)),
          tables(topo_ ? a_->topo_spare : a_->topo) {}
    // its flags (once prepare_topology has made room for new ones); null: the accel keeps no opaque-only tree
    const uint8_t *opaque_flags() const { return a->occl_on ? tables.opaque.get() : nullptr; }
};

// 1. The topology tables (with new triangle lists), then the build, repeated with more room while it does not fit (BuildCaps).
int build_with_retries(Update &u) {
    rtk_accel *a = u.a;
    // per-triangle scratch and the new shading records
    RTK_MEM(a->up_tris.reserve(u.nt, grow_bytes()));
    RTK_MEM(a->up_tbox.reserve(size_t(u.nt) * 6, grow_bytes()));
    RTK_MEM(a->geom_spare.shade.reserve(u.nt, grow_bytes()));
    if (u.topo) RTK_TRY(prepare_topology(a, *u.topo, u.s, u.TA));
    // (the table and the reference lists are sized exactly: their capacities are the build's, cap_nodes behind the header)
    auto table_bytes = [](size_t nodes) { return sizeof(dev::BuildHdr) + nodes * sizeof(dev::BuildNode); };
    auto cap_nodes = [&] { return a->up_table.get() ? (a->up_table.capacity() - sizeof(dev::BuildHdr)) / sizeof(dev::BuildNode) : size_t(0); };
    auto cap_refs = [&] { return a->up_ref_node.capacity(); };
    BuildCaps caps(cap_nodes(), cap_refs(), a->tree.dev_nodes.size(), u.nt, a->params.max_depth, u.topo != nullptr);
    for (bool first = true;; first = false) {
        if (caps.refused()) return fail(RTK_ERR_INVALID, "tree too large for 32-bit node/triangle indices");
        const BuildCaps::Request want = caps.request();
        RTK_MEM(a->up_table.reserve(table_bytes(want.nodes), set_exactly()));
        RTK_MEM(a->up_table_host.reserve(table_bytes(want.nodes), set_exactly()));
        RTK_MEM(a->up_ref_id.reserve(want.refs, set_exactly()));
        RTK_MEM(a->up_ref_node.reserve(want.refs, set_exactly()));
        dev::BuildArgs B;
        B.verts = u.d_verts; B.n_verts = uint32_t(a->scene.n_vertices); B.n_tris = u.nt;
        B.index = u.tables.index.get(); B.inc_off = u.tables.inc_off.get(); B.inc = u.tables.inc.get();
        B.opaque = u.opaque_flags();
        B.shade = a->geom_spare.shade.get();
        B.shade_old = u.topo ? B.shade : a->geom.shade.get();                        // (topology.hip wrote mesh / material into the new records)
        B.tris = a->up_tris.get(); B.tbox = a->up_tbox.get();
        B.ref_id = a->up_ref_id.get(); B.ref_node = a->up_ref_node.get();
        B.cap_refs = uint32_t(cap_refs()); B.cap_nodes = uint32_t(cap_nodes());
        B.max_depth = a->params.max_depth; B.max_leaf = a->params.max_leaf_size;
        B.hdr = reinterpret_cast<dev::BuildHdr *>(a->up_table.get());
        B.nodes = reinterpret_cast<dev::BuildNode *>(a->up_table.get() + sizeof(dev::BuildHdr));
        u.TA.hdr = B.hdr;
        // (the topology tables do not depend on the capacities: a repeat keeps them.  Their flag is read after the first attempt.)
        RTK_HIP_AS(launch_build(B, u.topo && first ? &u.TA : nullptr, u.s), "launch device build");
        // the one place an update blocks the host: flags, sizes and the node table
        RTK_HIP(hipMemcpyAsync(a->up_table_host.get(), a->up_table.get(), table_bytes(cap_nodes()), hipMemcpyDeviceToHost, u.s));
        RTK_HIP(hipStreamSynchronize(u.s));
        std::memcpy(&u.hdr, a->up_table_host.get(), sizeof(u.hdr));
        const uint32_t raised = ~u.hdr.ok;
        if (raised & dev::kBuildNonFinite) return fail(RTK_ERR_INVALID, "vertices must be finite");
        if (raised & dev::kBuildBadIndex) return fail(RTK_ERR_INVALID, "an index is not a vertex of its mesh");
        if ((raised & (dev::kBuildRefOverflow | dev::kBuildNodeOverflow)) == 0u) return RTK_OK;
        caps.overflowed(raised, u.hdr.need_nodes, u.hdr.need_refs, cap_nodes(), cap_refs());
    }
}

// 2. Numbering on the host (kdtree.cpp): reference order, traversal order with skip links, leaf offsets in both, FAST orders;
// the opaque-only tree from the counts the build left in the leaves.
int number_on_host(Update &u) {
    const dev::BuildNode *bn = reinterpret_cast<const dev::BuildNode *>(u.a->up_table_host.get() + sizeof(dev::BuildHdr));
    tree_from_build_nodes(bn, u.T, u.gather);
    if (u.T.nodes.size() != u.hdr.n_nodes) return fail(RTK_ERR_INVALID, "internal: the device build's node table is not a tree");
    if (u.a->fast_traversal) build_fast_leaf_orders(u.T);
    for (const dev::GatherLeaf &g : u.gather) u.n_refs += g.count;
    if (u.n_refs > 0x7FFFFFFFull) return fail(RTK_ERR_INVALID, "tree too large for 32-bit node/triangle indices");
    if (u.a->occl_on) {                                                 // (dev_leaves and gather are both the leaves in dev_nodes' order)
        std::vector<uint32_t> counts;
        for (const dev::GatherLeaf &g : u.gather) counts.push_back(g.pad[0]);
        if (const char *why = number_occluders(u.T.dev_nodes, counts, u.occl)) return fail(RTK_ERR_INVALID, why);
        for (size_t li = 0; li < u.occl.dst.size(); ++li) u.gather[li].dst_occl = u.occl.dst[li];
    }
    for (dev::GatherLeaf &g : u.gather) g.pad[0] = 0u;
    return RTK_OK;
}

// 3. Room in the spare set.
int reserve_spare(Update &u) {
    rtk_accel *a = u.a;
    GeomBufs &sp = a->geom_spare;
    RTK_MEM(sp.nodes.reserve(u.T.dev_nodes.size(), grow_bytes()));
    RTK_MEM(sp.leaves.reserve(u.T.dev_leaves.size(), grow_bytes()));
    if (a->fast_traversal) RTK_MEM(sp.leaves_fast.reserve(u.T.dev_leaves_fast.size(), grow_bytes()));
    RTK_MEM(sp.tris.reserve(u.n_refs, grow_bytes()));
    RTK_MEM(sp.tri_ids.reserve(u.n_refs, grow_bytes()));
    RTK_MEM(sp.leaf_refs.reserve(u.n_refs, grow_bytes()));
    if (a->occl_on) RTK_TRY(reserve_occluders(sp, u.occl));
    RTK_MEM(a->up_gather.reserve(u.gather.size(), grow_bytes()));
    return RTK_OK;
}

// 4. The small tables go up through one pinned buffer (the copies are stream-ordered and the host does not wait for them).
int stage_tables(Update &u) {
    rtk_accel *a = u.a;
    const GeomBufs &sp = a->geom_spare;
    struct Up { const void *src; void *dst; size_t bytes; };
    const Up ups[] = {
        {u.T.dev_nodes.data(), sp.nodes.get(), u.T.dev_nodes.size() * sizeof(DevNode)},
        {u.T.dev_leaves.data(), sp.leaves.get(), u.T.dev_leaves.size() * sizeof(DevNode)},
        {u.T.dev_leaves_fast.data(), sp.leaves_fast.get(), a->fast_traversal ? u.T.dev_leaves_fast.size() * sizeof(DevNode) : 0},
        {u.gather.data(), a->up_gather.get(), u.gather.size() * sizeof(dev::GatherLeaf)},
        {u.occl.nodes.data(), sp.occl_nodes.get(), u.occl.nodes.size() * sizeof(DevNode)},
        {u.occl.leaves.data(), sp.occl_leaves.get(), u.occl.leaves.size() * sizeof(DevNode)},
    };
    size_t total = 0;
    for (const Up &up : ups) total += (up.bytes + 63) & ~size_t(63);
    RTK_MEM(a->up_stage.reserve(total, grow_bytes()));
    uint8_t *const stage = a->up_stage.get();
    size_t at = 0;
    for (const Up &up : ups) {
        if (up.bytes == 0) continue;
        std::memcpy(stage + at, up.src, up.bytes);
        RTK_HIP(hipMemcpyAsync(up.dst, stage + at, up.bytes, hipMemcpyHostToDevice, u.s));
        at += (up.bytes + 63) & ~size_t(63);
    }
    return RTK_OK;
}

// 5. The references into the spare set, leaf by leaf, and the fence behind them.
int gather_and_publish(Update &u) {
    rtk_accel *a = u.a;
    GeomBufs &sp = a->geom_spare;
    dev::GatherArgs G;
    G.leaves = a->up_gather.get(); G.n_leaves = uint32_t(u.gather.size());
    G.ref_id = a->up_ref_id.get(); G.tris_in = a->up_tris.get(); G.opaque = u.opaque_flags();
    G.tris = sp.tris.get(); G.tri_ids = sp.tri_ids.get(); G.leaf_refs = sp.leaf_refs.get();
    G.occl_tris = sp.occl_tris.get(); G.occl_ids = sp.occl_ids.get();
    RTK_HIP_AS(launch_gather(G, u.s), "launch k_build_gather");
    if (a->occl_on && u.occl.n_opaque == 0) RTK_TRY(occl_placeholder(sp, sp.tris.get(), u.n_refs, u.s));
    RTK_HIP(a->geom_fence.publish(u.s));
    return RTK_OK;
}

// 6. Nothing here fails: swap the sets and bring the host's picture of the accel up to date.
void adopt(Update &u) {
    rtk_accel *a = u.a;
    const bool occl = a->occl_on;
    a->geom.swap(a->geom_spare, a->fast_traversal, occl);
    if (u.topo) {
        a->topo.swap(a->topo_spare, u.TA.tri_uv != nullptr);
        a->up_static = true;
        a->scene.n_triangles = int32_t(u.nt);
        a->mesh_ntris.assign(u.topo->mesh_ntris, u.topo->mesh_ntris + a->mesh_ntris.size());
        // the host's copy of the old lists, and what was derived from them: dropped, as the vertices are below
        for (HostMesh &m : a->scene.meshes) std::vector<uint32_t>().swap(m.indices);
        std::vector<DevTriUv>().swap(a->tree.dev_tri_uv);
    }
    a->occl_n_leaves = occl ? uint32_t(u.occl.leaves.size()) : 0u;
    a->tree.nodes = std::move(u.T.nodes);
    a->tree.dev_nodes = std::move(u.T.dev_nodes);
    a->tree.dev_leaves = std::move(u.T.dev_leaves);
    a->tree.dev_leaves_fast = std::move(u.T.dev_leaves_fast);
    a->tree.depth = u.T.depth;
    // what the host held per triangle, per reference and per vertex describes the old geometry: dropped, not left to lie
    // (rtk_accel_tree_dump fetches leaf_refs from the device)
    std::vector<HostTriangle>().swap(a->tree.triangles);
    std::vector<int32_t>().swap(a->tree.leaf_refs);
    std::vector<DevTri>().swap(a->tree.dev_tris);
    std::vector<uint32_t>().swap(a->tree.dev_tri_ids);
    std::vector<DevShade>().swap(a->tree.dev_shade);
    for (HostMesh &m : a->scene.meshes) { std::vector<Vec3>().swap(m.vertices); std::vector<Vec3>().swap(m.vertex_normals); }
    a->refs_on_device = true;
    a->n_leaf_refs_dev = int32_t(u.n_refs);
    a->coords_small = (~u.hdr.ok & dev::kBuildCoordsBig) == 0u;
    a->stream_slices_auto = stream_slices_for(a->tree);
    // the launch order learnt from the old silhouette and the engines' trial on it say nothing about the new geometry
    forget_orders(a);
}

// The one path of both updates.
int update_impl(rtk_accel *a, const float *d_verts, const NewTopology *topo, hipStream_t s) {
    if (!topo) RTK_TRY(ensure_update_static(a));
    Update u(a, d_verts, topo, s);
    RTK_TRY(build_with_retries(u));
    RTK_TRY(number_on_host(u));
    RTK_TRY(reserve_spare(u));
    RTK_TRY(stage_tables(u));
    RTK_TRY(gather_and_publish(u));
    adopt(u);
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
    const bool any = any_refractive(materials);
    bool set_changed = false;
    for (size_t i = 0; i < materials.size(); ++i) if (opaque(materials, i) != opaque(a->scene.materials, i)) set_changed = true;
    const bool tree = a->fast_traversal && a->knobs.fast_occluders && set_changed;
    if (!tree && !(a->topo.opaque.get() && set_changed)) return RTK_OK;
    dev::OcclArgs O{};
    O.materials = d_materials; O.n_materials = uint32_t(materials.size());
    O.shade = a->geom.shade.get(); O.n_tris = uint32_t(a->scene.n_triangles);
    if (tree && any) {
        // the leaves of the active tree, in dev_nodes' order: as number_occluders walks them
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
        Occluders o;
        if (const char *why = number_occluders(nodes, counts, o)) return fail(RTK_ERR_INVALID, why);
        for (size_t li = 0; li < nl; ++li) leaves[li].dst = o.dst[li];
        GeomBufs &sp = a->geom_spare;
        RTK_TRY(reserve_occluders(sp, o));
        // (pageable sources: these copies return when the data has left the host vectors)
        if (!o.nodes.empty()) RTK_HIP(hipMemcpyAsync(sp.occl_nodes.get(), o.nodes.data(), o.nodes.size() * sizeof(DevNode), hipMemcpyHostToDevice, s));
        RTK_HIP(hipMemcpyAsync(sp.occl_leaves.get(), o.leaves.data(), o.leaves.size() * sizeof(DevNode), hipMemcpyHostToDevice, s));
        if (nl > 0) RTK_HIP(hipMemcpyAsync(a->st_leaves.get(), leaves.data(), nl * sizeof(dev::OcclLeaf), hipMemcpyHostToDevice, s));
        O.occl_tris = sp.occl_tris.get(); O.occl_ids = sp.occl_ids.get(); O.cap = uint32_t(o.n_opaque);
        if (o.n_opaque > 0) RTK_HIP_AS(launch_occl_gather(O, s), "launch k_occl_gather");
        else RTK_TRY(occl_placeholder(sp, a->geom.tris.get(), n_refs, s));
        if (a->topo.opaque.get()) { O.opaque = a->topo.opaque.get(); RTK_HIP_AS(launch_occl_flags(O, s), "launch k_occl_flags"); }
        RTK_HIP(hipStreamSynchronize(s));                                   // (the host vectors above go out of scope)
        RTK_HIP(a->geom_fence.publish(s));
        // ---- nothing below fails
        a->geom.swap_occl(sp);
        a->occl_n_leaves = uint32_t(o.leaves.size());
        a->occl_on = true;
        return RTK_OK;
    }
    // the flags alone; a FAST accel that lost its last refractive material keeps the buffers for the next time
    if (a->topo.opaque.get()) {
        O.opaque = a->topo.opaque.get();
        RTK_HIP_AS(launch_occl_flags(O, s), "launch k_occl_flags");
        RTK_HIP(a->geom_fence.publish(s));
    }
    if (tree) { a->occl_on = false; a->occl_n_leaves = 0u; }
    return RTK_OK;
}

int rtk_accel_update_vertices_device(rtk_accel *a, const float *d_vertices, void *hip_stream) {
    return abi_guard([&]() -> int {
        if (!a || !d_vertices) return fail(RTK_ERR_INVALID, "null accel or vertices");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        // entry: nothing issued earlier on this accel, on whatever stream, may still read a buffer the update rewrites
        RTK_HIP(a->geom_fence.quiesce());
        return update_impl(a, d_vertices, nullptr, static_cast<hipStream_t>(hip_stream));
    });
}

int rtk_accel_update_vertices(rtk_accel *a, const float *vertices) {
    return abi_guard([&]() -> int {
        if (!a || !vertices) return fail(RTK_ERR_INVALID, "null accel or vertices");
        std::lock_guard<std::mutex> lock(a->mu);
        RTK_TRY(ensure_device(a));
        const size_t n = size_t(a->scene.n_vertices) * 3;
        for (size_t i = 0; i < n; ++i)
            if (!std::isfinite(vertices[i])) return fail(RTK_ERR_INVALID, "vertices must be finite");
        RTK_HIP(a->geom_fence.quiesce());
        RTK_MEM(a->up_verts.reserve(n));                                    // (once: the vertex count never changes)
        if (n > 0) RTK_HIP(hipMemcpy(a->up_verts.get(), vertices, n * sizeof(float), hipMemcpyHostToDevice));
        return update_impl(a, a->up_verts.get(), nullptr, nullptr);
    });
}

int rtk_accel_update_geometry_device(rtk_accel *a, const float *d_vertices, const uint32_t *d_indices, const int32_t *mesh_ntris, void *hip_stream) {
    return abi_guard([&]() -> int {
        if (!a || !d_vertices || !mesh_ntris) return fail(RTK_ERR_INVALID, "null accel, vertices or mesh_ntris");
        std::lock_guard<std::mutex> lock(a->mu);
        if (!d_indices && any_triangles(a, mesh_ntris)) return fail(RTK_ERR_INVALID, "null indices");
        RTK_TRY(ensure_device(a));
        NewTopology N{d_indices, mesh_ntris, 0u};
        RTK_TRY(check_counts(a, mesh_ntris, N.n_tris));
        RTK_HIP(a->geom_fence.quiesce());
        return update_impl(a, d_vertices, &N, static_cast<hipStream_t>(hip_stream));
    });
}

// validate + stage + the device path
int rtk_accel_update_geometry(rtk_accel *a, const float *vertices, const uint32_t *indices, const int32_t *mesh_ntris) {
    return abi_guard([&]() -> int {
        if (!a || !vertices || !mesh_ntris) return fail(RTK_ERR_INVALID, "null accel, vertices or mesh_ntris");
        std::lock_guard<std::mutex> lock(a->mu);
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
        RTK_HIP(a->geom_fence.quiesce());
        RTK_MEM(a->up_verts.reserve(n));
        if (n > 0) RTK_HIP(hipMemcpy(a->up_verts.get(), vertices, n * sizeof(float), hipMemcpyHostToDevice));
        RTK_MEM(a->up_idx_stage.reserve(size_t(N.n_tris) * 3, grow_bytes()));
        if (N.n_tris > 0u) RTK_HIP(hipMemcpy(a->up_idx_stage.get(), indices, size_t(N.n_tris) * 3 * sizeof(uint32_t), hipMemcpyHostToDevice));
        N.d_indices = a->up_idx_stage.get();
        return update_impl(a, a->up_verts.get(), &N, nullptr);
    });
}
