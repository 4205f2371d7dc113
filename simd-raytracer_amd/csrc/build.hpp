// Device kd-tree build for rtk_accel_update_vertices / _update_geometry (build.hip, topology.hip): what the kernels and the host share.
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

struct BuildArgs {
    const float *verts;             // [n_verts][3], the new positions
    uint32_t n_verts, n_tris;
    const uint32_t *index;          // [n_tris][3] vertex ids into verts (all meshes concatenated)
    const uint32_t *inc_off;        // [n_verts + 1] vertex -> incidences
    const uint32_t *inc;            // triangle * 3 + corner, ascending per vertex, duplicates kept
    const uint8_t *opaque;          // [n_tris] 1 = material not refractive; null when no opaque-only tree is kept
    const DevShade *shade_old;      // mesh / material of every triangle: the active records, or `shade` itself after topology.hip filled them in
    DevShade *shade;                // out
    DevTri *tris;                   // out, per triangle
    float *tbox;                    // out, [n_tris][6]
    uint32_t *ref_id, *ref_node;    // [cap_refs] the lists of every level, one behind the other
    uint32_t cap_refs, cap_nodes;
    int32_t max_depth, max_leaf;
    BuildHdr *hdr;
    BuildNode *nodes;               // [cap_nodes]
};

// rtk_accel_update_geometry: one row per mesh and a last one that holds the totals, from the host.
struct TopoMesh {
    uint32_t tri_begin, vert_begin;     // prefix sums over the meshes
    uint32_t n_verts;
    uint32_t material;
    uint32_t opaque;                    // 0: the material is refractive
    uint32_t pad[3];
};
static_assert(sizeof(TopoMesh) == 32, "TopoMesh must be 32 bytes");

// What topology.hip makes of a caller's triangle lists: every table the build takes from the topology.
struct TopoArgs {
    const uint32_t *indices;        // the caller's: [n_tris][3], mesh-local, NOT validated
    const TopoMesh *meshes;         // [n_meshes + 1]
    uint32_t n_meshes, n_tris, n_verts;
    const float *vert_uv;           // [n_verts][2]; null when the scene has no textures
    uint32_t *index;                // out: BuildArgs::index, validated
    uint32_t *inc_off, *inc;        // out: BuildArgs::inc_off / inc
    uint8_t *opaque;                // out: [n_tris]
    DevShade *shade;                // out: mesh, material and zero padding of [n_tris] records
    DevTriUv *tri_uv;               // out: [n_tris]; null when the scene has no textures
    uint32_t *keys;                 // scratch: [3 n_tris] the vertex ids sorted
    void *temp;                     // scratch of the sort, topology_temp_bytes() long
    size_t temp_bytes;
    BuildHdr *hdr;                  // kBuildBadIndex is raised here
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

// rtk_accel_set_materials (occluders.hip): the opaque-only occlusion tree again, from the ACTIVE tree and a new material table
// (OcclLeaf: build_nodes.hpp).

struct OcclArgs {
    const DevMaterial *materials;
    uint32_t n_materials;
    const DevShade *shade;          // the active per-triangle records: `material`
    uint32_t n_tris;
    const OcclLeaf *leaves;
    uint32_t n_leaves;
    uint32_t n_refs;                // length of tris / tri_ids
    const DevTri *tris;             // the active leaf references
    const uint32_t *tri_ids;
    uint32_t *counts;               // out of the count: [n_leaves] opaque references
    DevTri *occl_tris;              // out of the gather; `cap` slots
    uint32_t *occl_ids;
    uint32_t cap;
    uint8_t *opaque;                // out of the flags: [n_tris]
};

}  // namespace dev

hipError_t launch_occl_flags(const dev::OcclArgs &O, hipStream_t s);
hipError_t launch_occl_count(const dev::OcclArgs &O, hipStream_t s);
hipError_t launch_occl_gather(const dev::OcclArgs &O, hipStream_t s);

// header memset + (with `topo`: the topology tables, topology.hip) + triangles + vertex normals + tree
hipError_t launch_build(const dev::BuildArgs &B, const dev::TopoArgs *topo, hipStream_t s);
hipError_t launch_topology(const dev::TopoArgs &T, hipStream_t s);
// DevTriUv of the n_tris triangles whose vertex ids `index` holds, from the per-vertex uvs
hipError_t launch_tri_uv(const uint32_t *index, const float *vert_uv, uint32_t n_tris, uint32_t n_verts, DevTriUv *tri_uv, hipStream_t s);
hipError_t topology_temp_bytes(uint32_t n_tris, uint32_t n_verts, size_t *bytes);
hipError_t launch_gather(const dev::GatherArgs &G, hipStream_t s);

}  // namespace rtk
