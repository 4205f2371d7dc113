// rtk_accel_update_geometry: a caller's triangle lists become the tables the device build (build.hip) takes from the topology.
//
// What api_update.hip (ensure_update_static), kdtree.cpp (dev_shade's mesh / material, dev_tri_uv) and api.hip (which triangles
// are opaque) make on the host from the build-time topology is made here from `indices` and one small row per mesh:
//
//   k_topo_tris     one thread per triangle: its mesh (a search in the prefix sums), its three vertex ids over the concatenated
//                   vertex array, DevShade::mesh / ::material, the opaque flag, DevTriUv
//   the sort        rocPRIM, stable: the 3 n (vertex, triangle * 3 + corner) pairs by vertex
//   k_topo_offsets  one thread per vertex: where its run begins in the sorted pairs
//   k_tri_uv        one thread per triangle: DevTriUv alone, for new per-vertex uvs on the topology as it is
//
// An index is the caller's and may be anything.  k_topo_tris is the only kernel that sees it raw: it compares it with the vertex
// count of the triangle's own mesh, raises kBuildBadIndex and puts the mesh's first vertex in its place.  Everything behind it --
// the sort, k_build_tris' loads from the vertex array -- reads the table it wrote, so no index leaves a mesh's vertices whether
// the host notices the flag or not (it does, and drops the build).
//
// The incidence lists are the reason for a sort: k_build_normals sums a vertex's face normals in ascending (triangle, corner)
// order with duplicates kept (mesh.hpp:36-38 walks the triangles in index order and float addition does not commute), and the
// pairs enter the sort in exactly that order, so a STABLE sort by vertex leaves every run in it.  Counting with atomics would not.
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>

#include "build.hpp"

namespace rtk {
namespace dev {
namespace {

// triangle::uvs, loader.hpp:199-207 (kdtree.cpp build_tree): the uvs of a triangle's three vertices, by their ids over all meshes
__device__ __forceinline__ DevTriUv gather_tri_uv(const float *vert_uv, const uint32_t (&g)[3]) {
    DevTriUv u;
#pragma unroll
    for (int k = 0; k < 3; ++k) { u.uv[k * 2] = vert_uv[size_t(g[k]) * 2]; u.uv[k * 2 + 1] = vert_uv[size_t(g[k]) * 2 + 1]; }
    return u;
}

__global__ __launch_bounds__(256) void k_topo_tris(const TopoArgs T) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T.n_tris) return;
    // the first mesh whose triangles end behind i: meshes without triangles drop out by themselves
    uint32_t lo = 0u, hi = T.n_meshes;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) / 2u;
        if (T.meshes[mid + 1u].tri_begin <= i) lo = mid + 1u; else hi = mid;
    }
    const uint32_t m = lo < T.n_meshes ? lo : T.n_meshes - 1u;      // (i < the total, so lo is a mesh; the clamp costs nothing)
    const TopoMesh M = T.meshes[m];
    bool bad = false;
    uint32_t g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        uint32_t v = T.indices[size_t(i) * 3 + k];
        if (v >= M.n_verts) { bad = true; v = 0u; }
        v += M.vert_begin;                                          // (a mesh with triangles has a vertex: checked on the host)
        g[k] = v < T.n_verts ? v : T.n_verts - 1u;
        T.index[size_t(i) * 3 + k] = g[k];
    }
    T.opaque[i] = uint8_t(M.opaque);
    DevShade *sh = T.shade + i;                                     // (fn: k_build_tris; n0..n2: k_build_normals, every corner is in one list)
    sh->mesh = m; sh->material = M.material; sh->pad[0] = 0u; sh->pad[1] = 0u;
    if (T.tri_uv != nullptr) T.tri_uv[i] = gather_tri_uv(T.vert_uv, g);
    if (__builtin_amdgcn_ballot_w64(bad) != 0ull && __lane_id() == 0u) atomicAnd(&T.hdr->ok, ~kBuildBadIndex);
}

// rtk_accel_set_uvs / _set_textures: the per-triangle uvs alone, through the vertex ids of the live topology (`index` as
// k_topo_tris or the host wrote it: every id is a vertex; the clamp keeps a table that lies from becoming an address).
__global__ __launch_bounds__(256) void k_tri_uv(const uint32_t *index, const float *vert_uv, uint32_t n_tris, uint32_t n_verts, DevTriUv *tri_uv) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n_tris) return;
    uint32_t g[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { const uint32_t v = index[size_t(i) * 3 + k]; g[k] = v < n_verts ? v : n_verts - 1u; }
    tri_uv[i] = gather_tri_uv(vert_uv, g);
}

// inc_off[v] = the number of pairs whose vertex is below v, for v in [0, n_verts]: vertices no triangle uses get an empty run.
__global__ __launch_bounds__(256) void k_topo_offsets(const TopoArgs T) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v > T.n_verts) return;
    uint32_t lo = 0u, hi = T.n_tris * 3u;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2u;
        if (T.keys[mid] < v) lo = mid + 1u; else hi = mid;
    }
    T.inc_off[v] = lo;
}

// the bits of a vertex id: a radix pass less for every eight the vertex count does not need
unsigned key_bits(uint32_t n_verts) {
    unsigned bits = 1u;
    while (bits < 32u && (uint64_t(1) << bits) < uint64_t(n_verts)) ++bits;
    return bits;
}

}  // namespace
}  // namespace dev

hipError_t topology_temp_bytes(uint32_t n_tris, uint32_t n_verts, size_t *bytes) {
    *bytes = 0;
    if (n_tris == 0u) return hipSuccess;
    uint32_t *nk = nullptr;
    return rocprim::radix_sort_pairs(nullptr, *bytes, nk, nk, rocprim::counting_iterator<uint32_t>(0u), nk, size_t(n_tris) * 3, 0u,
                                     dev::key_bits(n_verts), nullptr);
}

hipError_t launch_tri_uv(const uint32_t *index, const float *vert_uv, uint32_t n_tris, uint32_t n_verts, DevTriUv *tri_uv, hipStream_t s) {
    if (n_tris == 0u || n_verts == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_tri_uv, dim3((n_tris + 255u) / 256u), dim3(256), 0, s, index, vert_uv, n_tris, n_verts, tri_uv);
    return hipGetLastError();
}

hipError_t launch_topology(const dev::TopoArgs &T, hipStream_t s) {
    hipError_t e;
    if (T.n_tris > 0u) {
        hipLaunchKernelGGL(dev::k_topo_tris, dim3((T.n_tris + 255u) / 256u), dim3(256), 0, s, T);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        // key: the vertex id, i.e. `index` as it lies there; value: its position triangle * 3 + corner
        size_t bytes = T.temp_bytes;
        e = rocprim::radix_sort_pairs(T.temp, bytes, T.index, T.keys, rocprim::counting_iterator<uint32_t>(0u), T.inc, size_t(T.n_tris) * 3, 0u,
                                      dev::key_bits(T.n_verts), s);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dev::k_topo_offsets, dim3((T.n_verts + 1u + 255u) / 256u), dim3(256), 0, s, T);
    return hipGetLastError();
}

}  // namespace rtk
