// tree_from_build_nodes (csrc/kdtree.cpp), the host's numbering of a device-built kd-tree, without a device:
//
//   build_nodes_check <scene.crtscene> <max_depth> <max_leaf> [<max_depth> <max_leaf> ...]
//
// For every pair the host build gives a tree H.  A plain breadth-first walk of H writes the table of BuildNodes the device
// build (csrc/build.hip) would hand over for it -- level by level, within a level by parent, child0 before child1, the lists
// of a level one behind the other and the levels one behind the other -- and tree_from_build_nodes has to get H back from it:
// the nodes in reference order, the flattened nodes and leaves byte for byte, the depth, and one copy job per leaf that
// takes the leaf's list to where H has it.  One line per pair: "... ok" or "... FAIL <what>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "build_nodes.hpp"

namespace rtk {
void set_error(const std::string &) {}          // (api.hip's, which this program does not link)
}

using namespace rtk;

namespace {

bool overlaps(const Box &a, const Box &o) {     // aabb3.hpp:68-72
    return (o.mn.x <= a.mx.x && a.mn.x <= o.mx.x) && (o.mn.y <= a.mx.y && a.mn.y <= o.mx.y) && (o.mn.z <= a.mx.z && a.mn.z <= o.mx.z);
}

float comp(const Vec3 &v, int k) { return k == 0 ? v.x : (k == 1 ? v.y : v.z); }

struct Table {
    std::vector<dev::BuildNode> nodes;          // build order
    std::vector<uint32_t> ref_id;               // every node's list at its `start`
    std::vector<int32_t> host_id;               // build order -> node of H
};

// The device's table for H.  The lists are made again from the boxes (an inner node of H does not keep its list).
std::string table_of(const HostTree &H, Table &t) {
    std::vector<std::vector<int32_t>> lists(1);
    for (size_t i = 0; i < H.triangles.size(); ++i) lists[0].push_back(int32_t(i));
    t.host_id.assign(1, 0);
    size_t lvl_begin = 0, lvl_end = 1;
    while (lvl_begin < lvl_end) {
        for (size_t b = lvl_begin; b < lvl_end; ++b) {                 // the children of this level: the next level
            const HostNode &hn = H.nodes[size_t(t.host_id[b])];
            for (const int32_t c : {hn.child0, hn.child1}) {
                if (c < 0) continue;
                std::vector<int32_t> l;
                for (const int32_t id : lists[b])
                    if (overlaps(H.nodes[size_t(c)].box, H.triangles[size_t(id)].box)) l.push_back(id);
                lists.push_back(l);
                t.host_id.push_back(c);
            }
        }
        lvl_begin = lvl_end;
        lvl_end = t.host_id.size();
    }
    if (t.host_id.size() != H.nodes.size()) return "the walk did not reach every node";
    std::vector<int32_t> build_of(H.nodes.size(), -1);
    for (size_t b = 0; b < t.host_id.size(); ++b) build_of[size_t(t.host_id[b])] = int32_t(b);
    t.nodes.resize(H.nodes.size());
    uint32_t at = 0;
    for (size_t b = 0; b < t.nodes.size(); ++b) {
        const HostNode &hn = H.nodes[size_t(t.host_id[b])];
        dev::BuildNode &n = t.nodes[b];
        std::memset(&n, 0, sizeof(n));
        n.lo[0] = hn.box.mn.x; n.lo[1] = hn.box.mn.y; n.lo[2] = hn.box.mn.z;
        n.hi[0] = hn.box.mx.x; n.hi[1] = hn.box.mx.y; n.hi[2] = hn.box.mx.z;
        n.child0 = hn.child0 < 0 ? -1 : build_of[size_t(hn.child0)];
        n.child1 = hn.child1 < 0 ? -1 : build_of[size_t(hn.child1)];
        n.start = at;
        n.count = uint32_t(lists[b].size());
        n.axis = dev::kBuildLeaf;
        if (hn.leaf_start < 0) {                                       // the plane is where a child's box ends
            const int32_t c = hn.child0 >= 0 ? hn.child0 : hn.child1;
            if (c < 0) return "an inner node without children";
            const Box &cb = H.nodes[size_t(c)].box;
            for (int k = 2; k >= 0; --k) {
                const float plane = hn.child0 >= 0 ? comp(cb.mx, k) : comp(cb.mn, k);
                if (plane != (hn.child0 >= 0 ? comp(hn.box.mx, k) : comp(hn.box.mn, k))) { n.axis = k; n.mid = plane; }
            }
            if (n.axis == dev::kBuildLeaf) n.axis = hn.depth % 3;       // (a plane that rounded onto the box's own side)
        } else {
            if (hn.leaf_count != int32_t(lists[b].size()) ||
                !std::equal(lists[b].begin(), lists[b].end(), H.leaf_refs.begin() + hn.leaf_start))
                return "the walk's list of a leaf is not the host build's";
        }
        for (const int32_t id : lists[b]) t.ref_id.push_back(uint32_t(id));
        at += n.count;
    }
    return "";
}

template <class T>
bool same_bytes(const std::vector<T> &a, const std::vector<T> &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

std::string check(const HostTree &H, const Table &t) {
    HostTree T;
    T.dev_leaves_fast.resize(3);                                       // (must be cleared)
    std::vector<dev::GatherLeaf> jobs(2);
    tree_from_build_nodes(t.nodes.data(), T, jobs);
    if (T.nodes.size() != H.nodes.size()) return "nodes: count";
    for (size_t i = 0; i < H.nodes.size(); ++i) {
        const HostNode &a = T.nodes[i], &b = H.nodes[i];
        const std::string at = " of node " + std::to_string(i);
        if (std::memcmp(&a.box, &b.box, sizeof(Box)) != 0) return "nodes: box" + at;
        if (a.child0 != b.child0 || a.child1 != b.child1) return "nodes: children" + at;
        if (a.depth != b.depth) return "nodes: depth" + at;
        if (a.leaf_start != b.leaf_start || a.leaf_count != b.leaf_count) return "nodes: leaf_start / leaf_count" + at;
    }
    if (!same_bytes(T.dev_nodes, H.dev_nodes)) return "dev_nodes";
    if (!same_bytes(T.dev_leaves, H.dev_leaves)) return "dev_leaves";
    if (!T.dev_leaves_fast.empty()) return "dev_leaves_fast not cleared";
    if (T.depth != H.depth) return "depth";
    if (jobs.size() != H.dev_leaves.size()) return "jobs: count";
    const size_t n_refs = H.leaf_refs.size();
    std::vector<uint8_t> seen_dst(n_refs, 0), seen_ref(n_refs, 0);
    for (size_t j = 0; j < jobs.size(); ++j) {
        const dev::GatherLeaf &g = jobs[j];
        const std::string at = " of job " + std::to_string(j);
        if (g.dst != H.dev_leaves[j].a || g.count != H.dev_leaves[j].b) return "jobs: dst / count is not the leaf's" + at;
        if (g.pad[0] != 0u || g.dst_occl != 0u) return "jobs: opaque count of a table without one" + at;
        if (size_t(g.src) + g.count > t.ref_id.size() || size_t(g.dst) + g.count > n_refs || size_t(g.dst_ref) + g.count > n_refs)
            return "jobs: out of range" + at;
        for (uint32_t k = 0; k < g.count; ++k) {
            const uint32_t id = t.ref_id[g.src + k];
            if (int32_t(id) != H.leaf_refs[g.dst_ref + k]) return "jobs: leaf_refs" + at;
            if (id != H.dev_tri_ids[g.dst + k]) return "jobs: dev_tri_ids" + at;
            if (seen_dst[g.dst + k]++ || seen_ref[g.dst_ref + k]++) return "jobs: overlap" + at;
        }
    }
    for (size_t i = 0; i < n_refs; ++i)
        if (!seen_dst[i] || !seen_ref[i]) return "jobs: gap at " + std::to_string(i);
    return "";
}

}  // namespace

int main(int argc, char **argv) {
    if (argc < 4 || (argc - 2) % 2 != 0) { std::fprintf(stderr, "usage: %s scene max_depth max_leaf [max_depth max_leaf ...]\n", argv[0]); return 2; }
    rtk_scene scene;
    std::string err;
    if (scene_from_crtscene(argv[1], scene, err) != RTK_OK) { std::fprintf(stderr, "%s: %s\n", argv[1], err.c_str()); return 2; }
    int bad = 0;
    for (int i = 2; i + 1 < argc; i += 2) {
        const int max_depth = std::atoi(argv[i]), max_leaf = std::atoi(argv[i + 1]);
        HostTree H;
        if (build_tree(scene, max_depth, max_leaf, H, err) != RTK_OK) { std::fprintf(stderr, "build_tree: %s\n", err.c_str()); return 2; }
        Table t;
        std::string what = table_of(H, t);
        if (what.empty()) what = check(H, t);
        size_t leaves = 0;
        for (const HostNode &n : H.nodes) leaves += n.leaf_start >= 0 ? 1 : 0;
        std::printf("depth %d leaf %d: nodes %zu leaves %zu refs %zu levels %d table_refs %zu %s%s\n", max_depth, max_leaf, H.nodes.size(), leaves,
                    H.leaf_refs.size(), H.depth + 1, t.ref_id.size(), what.empty() ? "ok" : "FAIL ", what.c_str());
        bad += what.empty() ? 0 : 1;
    }
    return bad ? 1 : 0;
}
