// Device kd-tree build for rtk_accel_update_vertices (build.hip): what the kernels and the host share.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "build_nodes.hpp"

namespace rtk {
namespace dev {

// Header in front of the node table, read back with it.  `ok` starts as all ones and a kernel CLEARS a bit to raise a flag
// (the header is initialised by one memset to 0xFF, which is also the neutral element of the root-box keys).
struct BuildHdr {
    uint32_t ok;
    uint32_t n_nodes, n_refs, depth;
    uint32_t need_nodes, need_refs;      // with kBuildNodeOverflow / kBuildRefOverflow: what the level that did not fit needed
    uint32_t pad[2];
    unsigned long long key[6];           // root box: (ordered value, lowest triangle) minima of lo.xyz, maxima of hi.xyz
    uint32_t pad2[12];
};
static_assert(sizeof(BuildHdr) == 128, "BuildHdr must be 128 bytes");
constexpr uint32_t kBuildNonFinite = 1u, kBuildCoordsBig = 2u, kBuildRefOverflow = 4u, kBuildNodeOverflow = 8u;

struct BuildArgs {
    const float *verts;             // [n_verts][3], the new positions
    uint32_t n_verts, n_tris;
    const uint32_t *index;          // [n_tris][3] vertex ids into verts (all meshes concatenated)
    const uint32_t *inc_off;        // [n_verts + 1] vertex -> incidences
    const uint32_t *inc;            // triangle * 3 + corner, ascending per vertex, duplicates kept
    const uint8_t *opaque;          // [n_tris] 1 = material not refractive; null when no opaque-only tree is kept
    const DevShade *shade_old;      // mesh / material of every triangle (constant topology)
    DevShade *shade;                // out
    DevTri *tris;                   // out, per triangle
    float *tbox;                    // out, [n_tris][6]
    uint32_t *ref_id, *ref_node;    // [cap_refs] the lists of every level, one behind the other
    uint32_t cap_refs, cap_nodes;
    int32_t max_depth, max_leaf;
    BuildHdr *hdr;
    BuildNode *nodes;               // [cap_nodes]
};

struct GatherArgs {
    const GatherLeaf *leaves;
    uint32_t n_leaves;
    const uint32_t *ref_id;
    const DevTri *tris_in;          // per triangle
    const uint8_t *opaque;          // null: no opaque-only copy
    DevTri *tris;
    uint32_t *tri_ids;
    int32_t *leaf_refs;
    DevTri *occl_tris;
    uint32_t *occl_ids;
};

}  // namespace dev

hipError_t launch_build(const dev::BuildArgs &B, hipStream_t s);       // header memset + triangles + vertex normals + tree
hipError_t launch_gather(const dev::GatherArgs &G, hipStream_t s);

}  // namespace rtk
