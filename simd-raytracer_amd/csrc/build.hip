// rtk_accel_update_vertices / rtk_accel_update_geometry: the accel of a scene whose vertices moved, rebuilt on the device.
// (A new triangle list first becomes the tables of BuildArgs in topology.hip; from there on the two calls are one.)
//
// Everything per vertex, per triangle and per (node, triangle) reference happens here; the host sees one table of nodes
// (build.hpp) and numbers them (kdtree.cpp).  The result is defined bit for bit by the host build (scene.cpp, kdtree.cpp, i.e.
// mesh.hpp:25-43, triangle.hpp:20-30, aabb3.hpp, kd_tree_simd.hpp:100-185), so every float operation below is the host's, in
// the host's order, and this file is compiled like the rest with -ffp-contract=off.  `1.0f / sqrtf(x)` and `x / 2.0f` are the
// correctly rounded IEEE operations (hipcc's default for float; tests/test_gpu_update.py compares the normals by bits).
//
//   k_build_tris     one thread per triangle (and per vertex, for the finiteness check)
//   k_build_normals  one thread per vertex
//   k_build_tree     ONE workgroup, level by level: at a few thousand triangles the build is bound by launches and
//                    synchronisation, and a workgroup synchronises with a barrier instead of a launch
//   k_build_gather   one wave per leaf
#include <hip/hip_runtime.h>

#include "build.hpp"
#include "trace.hip.hpp"

namespace rtk {
namespace dev {
namespace {

constexpr int kTreeThreads = 1024;
constexpr int kItems = 8;                                    // references per thread and trip of sweep_level
constexpr uint32_t kChunk = uint32_t(kTreeThreads) * uint32_t(kItems);
static_assert(kChunk <= (1u << 14) - 1u, "sweep_level packs a chunk's counts into 14 bits");

__device__ __forceinline__ uint32_t lanes_below(const unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
}

// Order-preserving map float -> uint32 with -0 == +0 (they compare equal in box_grow's `<`, so they must share a key).
__device__ __forceinline__ uint32_t ordered(float v) {
    v = (v == 0.0f) ? 0.0f : v;
    const uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ unsigned long long wave_min(unsigned long long k) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, off), hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), off);
        const unsigned long long o = ((unsigned long long)hi << 32) | lo;
        k = o < k ? o : k;
    }
    return k;
}

// triangle ctor (triangle.hpp:20-30) as kdtree.cpp build_tree does it, plus the triangle's part of the root box.
//
// Boxes keep the FIRST of equal extremes (box_grow is `p < mn ? p : mn`, and -0 == +0): the corners of a triangle are folded
// in order here; the mesh boxes grow over their triangles in index order (scene.cpp:49-52) and the root unites the mesh boxes
// in mesh order (kdtree.cpp:166-174) with the same rule, which together is the fold over all triangles in global order.
// "Least value, then lowest triangle" is that fold as an associative minimum, so it can be reduced in any order: the key is
// (ordered value, triangle) and the winner's own box supplies the bits.  Vertices no triangle uses never enter.
__global__ __launch_bounds__(256) void k_build_tris(const BuildArgs B) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    bool bad = false, big = false;
    if (i < B.n_verts) {
        const float x = B.verts[size_t(i) * 3], y = B.verts[size_t(i) * 3 + 1], z = B.verts[size_t(i) * 3 + 2];
        bad = !(fabsf(x) <= 3.402823466e38f && fabsf(y) <= 3.402823466e38f && fabsf(z) <= 3.402823466e38f);
    }
    unsigned long long key[6];
#pragma unroll
    for (int c = 0; c < 6; ++c) key[c] = ~0ull;
    if (i < B.n_tris) {
        const uint32_t ia = B.index[size_t(i) * 3], ib = B.index[size_t(i) * 3 + 1], ic = B.index[size_t(i) * 3 + 2];
        float v0[3], v1[3], v2[3], e1[3], e2[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            v0[k] = B.verts[size_t(ia) * 3 + k]; v1[k] = B.verts[size_t(ib) * 3 + k]; v2[k] = B.verts[size_t(ic) * 3 + k];
            e1[k] = v1[k] - v0[k]; e2[k] = v2[k] - v0[k];
        }
        // unit(cross(v1 - v0, v2 - v0)), vec3.hpp:104-108 / 124-131
        const float cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
        const float inv_length = 1.0f / sqrtf(cx * cx + cy * cy + cz * cz);
        DevShade sh = B.shade_old[i];                                   // mesh, material: topology (may be B.shade[i] itself)
        sh.fn[0] = cx * inv_length; sh.fn[1] = cy * inv_length; sh.fn[2] = cz * inv_length;
        B.shade[i] = sh;                                                // (n0..n2: k_build_normals)
        DevTri t;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            t.v0[k] = v0[k]; t.e1[k] = e1[k]; t.e2[k] = e2[k];
            // coords_small (api.hip, rtk_accel_build): every triangle is in some leaf, so "every leaf reference" is "every triangle"
            big = big || !(fabsf(v0[k]) <= kBundleLimit && fabsf(e1[k]) <= kBundleLimit && fabsf(e2[k]) <= kBundleLimit);
            float mn = 3.402823466e38f, mx = -3.402823466e38f;          // box_reset, then box_grow with v0, v1, v2
            mn = v0[k] < mn ? v0[k] : mn; mx = mx < v0[k] ? v0[k] : mx;
            mn = v1[k] < mn ? v1[k] : mn; mx = mx < v1[k] ? v1[k] : mx;
            mn = v2[k] < mn ? v2[k] : mn; mx = mx < v2[k] ? v2[k] : mx;
            B.tbox[size_t(i) * 6 + k] = mn; B.tbox[size_t(i) * 6 + 3 + k] = mx;
            key[k] = ((unsigned long long)ordered(mn) << 32) | i;
            key[3 + k] = ((unsigned long long)(~ordered(mx)) << 32) | i;
        }
        B.tris[i] = t;
    }
    const uint32_t lane = __lane_id();
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const unsigned long long k = wave_min(key[c]);
        if (lane == 0u && k != ~0ull) atomicMin(&B.hdr->key[c], k);
    }
    const unsigned long long any_bad = __builtin_amdgcn_ballot_w64(bad), any_big = __builtin_amdgcn_ballot_w64(big);
    if (lane == 0u && (any_bad | any_big) != 0ull)
        atomicAnd(&B.hdr->ok, ~((any_bad ? kBuildNonFinite : 0u) | (any_big ? kBuildCoordsBig : 0u)));
}

// mesh.hpp:36-43 / scene.cpp:53-58.  The reference adds each face normal to its three vertices while it walks the triangles in
// index order, and float addition does not commute across that order: a vertex's incidence list is ascending by triangle and
// keeps duplicates (a triangle [0,0,1] adds twice to vertex 0), and the sum starts from +0 as there.  A vertex no triangle
// uses would become NaN, as there; nothing reads it.
__global__ __launch_bounds__(256) void k_build_normals(const BuildArgs B) {
    const uint32_t v = blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= B.n_verts) return;
    const uint32_t first = B.inc_off[v], last = B.inc_off[v + 1];
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    for (uint32_t e = first; e < last; ++e) {
        const float *fn = B.shade[B.inc[e] / 3u].fn;
        sx = sx + fn[0]; sy = sy + fn[1]; sz = sz + fn[2];
    }
    const float inv_length = 1.0f / sqrtf(sx * sx + sy * sy + sz * sz);
    const float nx = sx * inv_length, ny = sy * inv_length, nz = sz * inv_length;
    for (uint32_t e = first; e < last; ++e) {
        const uint32_t t = B.inc[e] / 3u, corner = B.inc[e] % 3u;
        float *n = corner == 0u ? B.shade[t].n0 : (corner == 1u ? B.shade[t].n1 : B.shade[t].n2);
        n[0] = nx; n[1] = ny; n[2] = nz;
    }
}

// Exclusive scan of two counters over the workgroup; `total` is the same in every thread.
__device__ __forceinline__ uint2 block_scan2(const uint32_t a, const uint32_t b, uint2 *wsum, uint2 &total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t ia = a, ib = b;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ta = __shfl_up(ia, off), tb = __shfl_up(ib, off);
        if (lane >= (uint32_t)off) { ia += ta; ib += tb; }
    }
    if (lane == 63u) wsum[w] = make_uint2(ia, ib);
    __syncthreads();
    uint2 base = make_uint2(0u, 0u), tot = make_uint2(0u, 0u);
    for (uint32_t k = 0; k < uint32_t(kTreeThreads / 64); ++k) {
        const uint2 s = wsum[k];
        if (k < w) { base.x += s.x; base.y += s.y; }
        tot.x += s.x; tot.y += s.y;
    }
    __syncthreads();
    total = tot;
    return make_uint2(base.x + ia - a, base.y + ib - b);
}

// One pass over the references of a level, [ref_begin, ref_end), in chunks of kChunk: every thread takes kItems consecutive
// references, so the dependent loads of a chunk (reference -> node -> box) are in flight kItems deep and a level of a few
// thousand references is one or two trips through the workgroup's barriers.  Every reference of an inner node tests the two
// halves of its node's box (aabb3.hpp:68-72, inclusive on both sides: a triangle on the split plane goes to both children) and
// learns its rank among its node's earlier references that passed the same test: a scan over the chunk minus the scan's value
// at the node's first reference in the chunk, plus -- for the one node that straddles the chunk's start -- what it collected
// before (`carry`).
// WRITE = false counts (c0, c1 become the sizes of the children's lists; for a leaf, c0 its number of opaque triangles);
// WRITE = true places the ids.  The rank keeps the order, the list of the root ascends, so every list ascends by triangle
// index: that is the order of `ids` in Builder::build, i.e. the reference's order within a leaf.
struct SweepLds {
    uint2 wsum[kTreeThreads / 64];
    uint32_t sc[kChunk];            // per reference: exclusive count of f0 (14 bits), of f1 (14 bits), f0, f1, "takes part"
    uint32_t carry[2][2];           // [chunk parity]: what the node open at the chunk's end has collected (f0, f1)
};

template <bool WRITE>
__device__ void sweep_level(const BuildArgs &B, const uint32_t ref_begin, const uint32_t ref_end, SweepLds &L) {
    if (threadIdx.x < 4u) L.carry[threadIdx.x >> 1][threadIdx.x & 1u] = 0u;
    uint32_t parity = 0u;
    for (uint32_t base = ref_begin; base < ref_end; base += kChunk, parity ^= 1u) {
        const uint32_t first = base + threadIdx.x * uint32_t(kItems);
        uint32_t n[kItems], id[kItems], fl[kItems];
        uint32_t s0 = 0u, s1 = 0u;
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            const uint32_t i = first + uint32_t(j);
            n[j] = 0u; id[j] = 0u; fl[j] = 0u;
            if (i < ref_end) {
                n[j] = B.ref_node[i]; id[j] = B.ref_id[i];
                const BuildNode &nd = B.nodes[n[j]];
                const int32_t axis = nd.axis;
                if (axis != kBuildLeaf) {
                    const float mid = nd.mid;
                    const float *tb = B.tbox + size_t(id[j]) * 6;
                    bool in0 = true, in1 = true;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const float lo = nd.lo[k], hi = nd.hi[k], tlo = tb[k], thi = tb[3 + k];
                        const float hi0 = (k == axis) ? mid : hi, lo1 = (k == axis) ? mid : lo;      // child0 = [lo, mid], child1 = [mid, hi]
                        in0 = in0 && (tlo <= hi0 && lo <= thi);
                        in1 = in1 && (tlo <= hi && lo1 <= thi);
                    }
                    fl[j] = 4u | (in0 ? 1u : 0u) | (in1 ? 2u : 0u);
                } else if (!WRITE && B.opaque != nullptr) {
                    fl[j] = 4u | uint32_t(B.opaque[id[j]] != 0u);
                }
            }
            s0 += fl[j] & 1u; s1 += (fl[j] >> 1) & 1u;
        }
        uint2 total;
        const uint2 ex = block_scan2(s0, s1, L.wsum, total);
        {
            uint32_t e0 = ex.x, e1 = ex.y;
#pragma unroll
            for (int j = 0; j < kItems; ++j) {
                L.sc[threadIdx.x * uint32_t(kItems) + uint32_t(j)] = e0 | (e1 << 14) | (fl[j] << 28);
                e0 += fl[j] & 1u; e1 += (fl[j] >> 1) & 1u;
            }
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if ((fl[j] & 4u) == 0u) continue;
            const uint32_t i = first + uint32_t(j);
            const BuildNode &nd = B.nodes[n[j]];
            const uint32_t nstart = nd.start, nend = nd.start + nd.count;
            const uint32_t mine = L.sc[i - base], head = L.sc[nstart > base ? nstart - base : 0u];
            uint32_t r0 = (mine & 0x3FFFu) - (head & 0x3FFFu), r1 = ((mine >> 14) & 0x3FFFu) - ((head >> 14) & 0x3FFFu);
            if (nstart < base) { r0 += L.carry[parity ^ 1u][0]; r1 += L.carry[parity ^ 1u][1]; }
            const uint32_t f0 = fl[j] & 1u, f1 = (fl[j] >> 1) & 1u;
            if (WRITE) {
                if (f0) { const uint32_t d = B.nodes[nd.child0].start + r0; B.ref_id[d] = id[j]; B.ref_node[d] = uint32_t(nd.child0); }
                if (f1) { const uint32_t d = B.nodes[nd.child1].start + r1; B.ref_id[d] = id[j]; B.ref_node[d] = uint32_t(nd.child1); }
            } else if (i + 1u == nend) {
                B.nodes[n[j]].c0 = r0 + f0; B.nodes[n[j]].c1 = r1 + f1;
            }
            if (i + 1u == base + kChunk) { L.carry[parity][0] = r0 + f0; L.carry[parity][1] = r1 + f1; }
        }
        // (the next trip overwrites sc behind block_scan2's barriers, and carry[parity] a whole trip later)
    }
    __syncthreads();
}

// Builder::build (kd_tree_simd.hpp:146-185, kdtree.cpp) breadth first.  The recursion there only decides the numbering of the
// nodes, which the host redoes; what a node holds depends on its box and its list alone.
__global__ __launch_bounds__(kTreeThreads) void k_build_tree(const BuildArgs B) {
    __shared__ SweepLds lds;
    uint2 *wsum = lds.wsum;
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) {
        BuildNode r;
        for (int k = 0; k < 3; ++k) {
            const unsigned long long kl = B.hdr->key[k], kh = B.hdr->key[3 + k];
            r.lo[k] = kl == ~0ull ? 3.402823466e38f : B.tbox[size_t(uint32_t(kl)) * 6 + k];          // no triangle: box_reset's box
            r.hi[k] = kh == ~0ull ? -3.402823466e38f : B.tbox[size_t(uint32_t(kh)) * 6 + 3 + k];
        }
        r.child0 = r.child1 = -1; r.start = 0u; r.count = B.n_tris; r.c0 = r.c1 = 0u; r.axis = kBuildLeaf; r.mid = 0.0f; r.pad[0] = r.pad[1] = 0u;
        B.nodes[0] = r;
    }
    for (uint32_t i = tid; i < B.n_tris; i += uint32_t(kTreeThreads)) { B.ref_id[i] = i; B.ref_node[i] = 0u; }     // `all` ascends
    __syncthreads();
    uint32_t lvl_begin = 0u, lvl_end = 1u, ref_begin = 0u, ref_end = B.n_tris;
    int32_t depth = 0;
    for (;;) {
        // which nodes of this level stop (kdtree.cpp Builder::build / split_box)
        for (uint32_t n = lvl_begin + tid; n < lvl_end; n += uint32_t(kTreeThreads)) {
            BuildNode &nd = B.nodes[n];
            int32_t axis = kBuildLeaf;
            float mid = 0.0f;
            if (!(depth == B.max_depth || int64_t(nd.count) <= int64_t(B.max_leaf))) {
                // aabb3.hpp:43-60: an axis of zero extent hands over to the next one; a point box becomes a leaf
                int32_t ax = depth % 3;
                for (int tries = 0; tries < 3 && nd.lo[ax] == nd.hi[ax]; ++tries) ax = (ax + 1) % 3;
                if (nd.lo[ax] != nd.hi[ax]) { axis = ax; mid = nd.lo[ax] + ((nd.hi[ax] - nd.lo[ax]) / 2.0f); }
            }
            nd.axis = axis; nd.mid = mid; nd.c0 = 0u; nd.c1 = 0u;
        }
        __syncthreads();
        sweep_level<false>(B, ref_begin, ref_end, lds);
        // the children: an empty list gives no node (child = -1), as there
        uint32_t next_id = lvl_end;
        unsigned long long next_ref = ref_end;
        bool overflow = false;
        for (uint32_t chunk = lvl_begin; chunk < lvl_end; chunk += uint32_t(kTreeThreads)) {
            const uint32_t n = chunk + tid;
            const bool valid = n < lvl_end;
            const bool inner = valid && B.nodes[n].axis != kBuildLeaf;
            const uint32_t c0 = inner ? B.nodes[n].c0 : 0u, c1 = inner ? B.nodes[n].c1 : 0u;
            uint2 total;
            const uint2 ex = block_scan2((c0 != 0u ? 1u : 0u) + (c1 != 0u ? 1u : 0u), c0 + c1, wsum, total);
            if ((unsigned long long)next_id + total.x > B.cap_nodes || next_ref + total.y > B.cap_refs) overflow = true;     // (uniform)
            if (inner && !overflow) {
                BuildNode &nd = B.nodes[n];
                uint32_t id = next_id + ex.x;
                const uint32_t st = uint32_t(next_ref) + ex.y;
                nd.child0 = nd.child1 = -1;
                for (int side = 0; side < 2; ++side) {
                    const uint32_t c = side == 0 ? c0 : c1;
                    if (c == 0u) continue;
                    BuildNode ch;
                    for (int k = 0; k < 3; ++k) {                        // aabb3::split: child0 below the plane, child1 above
                        ch.lo[k] = (side == 1 && k == nd.axis) ? nd.mid : nd.lo[k];
                        ch.hi[k] = (side == 0 && k == nd.axis) ? nd.mid : nd.hi[k];
                    }
                    ch.child0 = ch.child1 = -1; ch.start = side == 0 ? st : st + c0; ch.count = c; ch.c0 = ch.c1 = 0u;
                    ch.axis = kBuildLeaf; ch.mid = 0.0f; ch.pad[0] = ch.pad[1] = 0u;
                    B.nodes[id] = ch;
                    if (side == 0) nd.child0 = int32_t(id); else nd.child1 = int32_t(id);
                    id += 1u;
                }
                nd.c0 = 0u; nd.c1 = 0u;
            }
            next_id += total.x; next_ref += total.y;
        }
        if (overflow) {
            if (tid == 0u) {
                B.hdr->need_nodes = next_id; B.hdr->need_refs = next_ref > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(next_ref);
                atomicAnd(&B.hdr->ok, ~((next_id > B.cap_nodes ? kBuildNodeOverflow : 0u) | (next_ref > B.cap_refs ? kBuildRefOverflow : 0u)));
            }
            return;
        }
        __syncthreads();
        if (next_id == lvl_end) break;                                   // no node of this level split
        sweep_level<true>(B, ref_begin, ref_end, lds);
        lvl_begin = lvl_end; lvl_end = next_id; ref_begin = ref_end; ref_end = uint32_t(next_ref);
        depth += 1;
    }
    if (tid == 0u) { B.hdr->n_nodes = lvl_end; B.hdr->n_refs = ref_end; B.hdr->depth = uint32_t(depth); }
}

// The leaves' packets: DevTri / tri_ids in traversal order of the leaves (kdtree.cpp flatten), leaf_refs in reference order
// (HostTree::leaf_refs, rtk_accel_tree_dump), and with `opaque` the leaf without its transmissive triangles (api.hip,
// ensure_device).  One wave per leaf; the opaque copy keeps the order through ballot + mbcnt.
__global__ __launch_bounds__(64) void k_build_gather(const GatherArgs G) {
    const GatherLeaf L = G.leaves[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint32_t kept = 0u;
    for (uint32_t k0 = 0u; k0 < L.count; k0 += 64u) {
        const uint32_t k = k0 + lane;
        const bool valid = k < L.count;
        uint32_t id = 0u;
        DevTri t = {};
        if (valid) {
            id = G.ref_id[L.src + k];
            t = G.tris_in[id];
            G.tris[L.dst + k] = t; G.tri_ids[L.dst + k] = id; G.leaf_refs[L.dst_ref + k] = int32_t(id);
        }
        if (G.opaque != nullptr) {
            const bool keep = valid && G.opaque[id] != 0u;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
            if (keep) { const uint32_t d = L.dst_occl + kept + lanes_below(m); G.occl_tris[d] = t; G.occl_ids[d] = id; }
            kept += uint32_t(__popcll(m));
        }
    }
}

}  // namespace
}  // namespace dev

hipError_t launch_build(const dev::BuildArgs &B, const dev::TopoArgs *topo, hipStream_t s) {
    hipError_t e = hipMemsetAsync(B.hdr, 0xFF, sizeof(dev::BuildHdr), s);
    if (e != hipSuccess) return e;
    if (topo != nullptr && (e = launch_topology(*topo, s)) != hipSuccess) return e;
    const uint32_t n = B.n_verts > B.n_tris ? B.n_verts : B.n_tris;
    if (n > 0u) {
        hipLaunchKernelGGL(dev::k_build_tris, dim3((n + 255u) / 256u), dim3(256), 0, s, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    if (B.n_verts > 0u) {
        hipLaunchKernelGGL(dev::k_build_normals, dim3((B.n_verts + 255u) / 256u), dim3(256), 0, s, B);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(dev::k_build_tree, dim3(1), dim3(dev::kTreeThreads), 0, s, B);
    return hipGetLastError();
}

hipError_t launch_gather(const dev::GatherArgs &G, hipStream_t s) {
    if (G.n_leaves == 0u) return hipSuccess;
    hipLaunchKernelGGL(dev::k_build_gather, dim3(G.n_leaves), dim3(64), 0, s, G);
    return hipGetLastError();
}

}  // namespace rtk
