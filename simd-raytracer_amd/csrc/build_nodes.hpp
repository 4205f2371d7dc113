// What the device build (build.hip) hands to the host's numbering (kdtree.cpp): plain structs, no HIP runtime needed.
#pragma once

#include <cstdint>
#include <vector>

#include "rtk_internal.hpp"

namespace rtk {
namespace dev {

// One node of the device build, in the order the build creates nodes: level by level, within a level by parent, child0
// before child1.  The host renumbers (kdtree.cpp, tree_from_build_nodes).
struct BuildNode {
    float lo[3], hi[3];
    int32_t child0, child1;     // build-order ids, -1 = no such child (its list was empty)
    uint32_t start, count;      // the node's triangle ids: ref_id[start, start + count), ascending
    uint32_t c0, c1;            // scratch of the build; in a leaf c0 ends as the number of opaque triangles (when asked for)
    int32_t axis;               // split axis, kBuildLeaf for a leaf
    float mid;
    uint32_t pad[2];
};
static_assert(sizeof(BuildNode) == 64, "BuildNode must be 64 bytes");
constexpr int32_t kBuildLeaf = 3;

// One leaf's copy job, in traversal order of the leaves.
struct GatherLeaf {
    uint32_t src, count;            // ref_id[src, src + count)
    uint32_t dst, dst_ref, dst_occl;   // first slot in tris / tri_ids, in leaf_refs (reference order), in the opaque-only copy
    uint32_t pad[3];
};

// One leaf of the ACTIVE tree when rtk_accel_set_materials re-makes the opaque-only occlusion tree from it (occluders.hip).
struct OcclLeaf {
    uint32_t first, count;          // the leaf's run in the active tris / tri_ids
    uint32_t dst;                   // its first slot in the opaque-only copy (the gather's; the count kernel does not read it)
    uint32_t pad;
};
static_assert(sizeof(OcclLeaf) == 16, "OcclLeaf must be 16 bytes");

// The flags of BuildHdr::ok (build.hpp): a kernel CLEARS a bit to raise one.
constexpr uint32_t kBuildNonFinite = 1u, kBuildCoordsBig = 2u, kBuildRefOverflow = 4u, kBuildNodeOverflow = 8u;
constexpr uint32_t kBuildBadIndex = 16u;     // topology.hip: an index that is not a vertex of its own mesh

}  // namespace dev

// kdtree.cpp: numbering and flattening of a device-built tree (nodes, depth, dev_nodes, dev_leaves of `out`)
void tree_from_build_nodes(const dev::BuildNode *bn, HostTree &out, std::vector<dev::GatherLeaf> &gather);

}  // namespace rtk
