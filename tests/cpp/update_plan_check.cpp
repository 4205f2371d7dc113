// update_plan.hpp on the host: what changing a resident accel decides before anything is reserved, copied or launched
// (tests/test_cpp_update_plan.py).  The expected values are literals, worked out by hand from the expressions as they stood inline
// in update_impl, ensure_device, remake_occluders and ensure_update_static.  Plain g++, no HIP.  Prints one "... ok" line per
// group; any failure is reported and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <utility>
#include <vector>

#include "update_plan.hpp"

using namespace rtk;

namespace {

int g_failed = 0;
#define CHECK(cond, ...)                                                     \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s (line %d): ", #cond, __LINE__);           \
            std::printf(__VA_ARGS__);                                        \
            std::printf("\n");                                               \
            if (++g_failed > 20) std::exit(1);                               \
        }                                                                    \
    } while (0)

constexpr uint32_t kNodes = dev::kBuildNodeOverflow, kRefs = dev::kBuildRefOverflow;

// the next attempt of `c`: not refused, and these capacities
void expect(BuildCaps &c, size_t nodes, size_t refs, const char *what) {
    CHECK(!c.refused(), "%s: refused", what);
    const BuildCaps::Request r = c.request();
    CHECK(r.nodes == nodes && r.refs == refs, "%s: {%zu, %zu}, expected {%zu, %zu}", what, r.nodes, r.refs, nodes, refs);
}

void caps() {
    // (cap_nodes, cap_refs, n_nodes, n_tris, max_depth, new_topology)
    { BuildCaps c(0, 0, 1, 0, 8, false); expect(c, 511, 4096, "first update of an empty tree: 1024 clamped to 2^9 - 1, the floor of 4096"); }
    { BuildCaps c(0, 0, 1, 10, 0, false); expect(c, 1, 4096, "depth 0: one node; 2 * 10 * 2 = 40 references are under the floor"); }
    { BuildCaps c(0, 0, 1, 1000, 16, false); expect(c, 1024, 28000, "depth 16: 2 * 1000 * (12 + 2)"); }
    { BuildCaps c(0, 0, 1, 1000, 12, false); expect(c, 1024, 28000, "depth 12: the same multiplier"); }
    { BuildCaps c(0, 0, 1, 1000, 11, false); expect(c, 1024, 26000, "depth 11: 2 * 1000 * 13"); }
    { BuildCaps c(0, 0, 255, 1000, 16, false); expect(c, 1024, 28000, "4 * 255 = 1020 is below 1024"); }
    { BuildCaps c(0, 0, 257, 1000, 16, false); expect(c, 1028, 28000, "4 * 257 = 1028 is above"); }
    { BuildCaps c(2000, 50000, 7, 1000, 16, false); expect(c, 2000, 50000, "kept capacities are the first request of a later update"); }
    { BuildCaps c(2000, 50000, 7, 1000, 16, true); expect(c, 2000, 50000, "new topology that the kept lists have room for"); }
    { BuildCaps c(2000, 50000, 7, 3000, 16, true); expect(c, 2000, 84000, "new topology of 3000 triangles: 2 * 3000 * 14 beats the kept 50000"); }
    { BuildCaps c(2000, 50000, 7, 3000, 16, false); expect(c, 2000, 50000, "the same triangle count without a new topology keeps them"); }
    { BuildCaps c(2000, 100, 7, 500, 16, false); expect(c, 2000, 500, "kept lists shorter than the triangles: raised to one reference each"); }
    { BuildCaps c(4000, 50000, 7, 1000, 8, false); expect(c, 511, 50000, "kept nodes above what the depth allows"); }
    {   // growth: what overflowed, by max(2 * cap, 2 * need); the rest stays
        BuildCaps c(0, 0, 1, 1000, 16, false);
        expect(c, 1024, 28000, "growth, first attempt");
        c.overflowed(kNodes, 600, 999999, 1024, 28000);
        expect(c, 2048, 28000, "nodes alone, 2 * cap beats 2 * need; need_refs is not read");
        c.overflowed(kRefs, 999999, 40000, 2048, 28000);
        expect(c, 2048, 80000, "references alone, 2 * need beats 2 * cap; need_nodes is not read");
        c.overflowed(kNodes | kRefs | dev::kBuildCoordsBig, 3000, 10, 2048, 80000);
        expect(c, 6000, 160000, "both at once: nodes by need, references by cap");
    }
    {   // growth past what the depth allows is clamped again
        BuildCaps c(0, 0, 1, 0, 8, false);
        expect(c, 511, 4096, "clamp, first attempt");
        c.overflowed(kNodes, 400, 0, 511, 4096);
        expect(c, 511, 4096, "max(1022, 800) clamped to 511");
    }
    {   // the first attempt and 16 retries run; the next is refused
        BuildCaps c(0, 0, 1, 0, 16, false);
        for (int attempt = 1; attempt <= 17; ++attempt) {
            CHECK(!c.refused(), "attempt %d is refused", attempt);
            const BuildCaps::Request r = c.request();
            CHECK(r.nodes == (attempt == 1 ? 1024u : 2u) && r.refs == 4096, "attempt %d: {%zu, %zu}", attempt, r.nodes, r.refs);
            c.overflowed(kNodes, 1, 0, 1, 4096);
        }
        CHECK(c.refused(), "the 18th attempt is not refused");
    }
    {   // the 32-bit bound of the reference lists
        BuildCaps at(2000, 0x7FFFFFF0ull, 7, 10, 16, false), past(2000, 0x7FFFFFF1ull, 7, 10, 16, false), grown(2000, 100, 7, 10, 16, false);
        expect(at, 2000, 0x7FFFFFF0ull, "kept lists at the bound");
        CHECK(past.refused(), "one past the bound is not refused");
        expect(grown, 2000, 100, "before the growth past the bound");
        grown.overflowed(kRefs, 0, 0x40000000ull, 2000, 100);
        CHECK(grown.refused(), "2 * 2^30 references are not refused");
    }
    if (!g_failed) std::printf("caps ok\n");
}

DevNode node(float tag, uint32_t a, uint32_t b) { return DevNode{{tag, tag + 1, tag + 2}, {tag + 3, tag + 4, tag + 5}, a, b}; }
bool same(const DevNode &x, const DevNode &y) { return std::memcmp(&x, &y, sizeof(DevNode)) == 0; }
bool same(const std::vector<uint32_t> &x, std::initializer_list<uint32_t> y) { return x == std::vector<uint32_t>(y); }

// node 0 (skip 5) { leaf 1, node 2 (skip 5) { leaf 3, leaf 4 } }: leaves of 4, 7 and 3 references
std::vector<DevNode> three_leaves() { return {node(10, 5, DEV_INNER), node(20, 0, 4), node(30, 5, DEV_INNER), node(40, 4, 7), node(50, 11, 3)}; }

void occluders() {
    Occluders o;
    {   // a root that is a leaf: all opaque, none opaque, empty
        const std::vector<DevNode> root = {node(10, 0, 5)};
        CHECK(number_occluders(root, {5}, o) == nullptr, "all opaque: refused");
        CHECK(o.nodes.size() == 1 && same(o.nodes[0], node(10, 0, 5)) && o.leaves.size() == 1 && same(o.leaves[0], node(10, 0, 5)) && same(o.dst, {0}) && o.n_opaque == 5, "all opaque");
        CHECK(number_occluders(root, {0}, o) == nullptr, "none opaque: refused");
        CHECK(o.nodes.size() == 1 && same(o.nodes[0], node(10, 0, 0)) && o.leaves.size() == 1 && same(o.leaves[0], node(10, 0, 0)) && same(o.dst, {0}) && o.n_opaque == 0, "none opaque: the placeholder");
        CHECK(number_occluders({node(10, 0, 0)}, {0}, o) == nullptr, "empty root: refused");
        CHECK(o.nodes.size() == 1 && same(o.nodes[0], node(10, 0, 0)) && o.leaves.size() == 1 && same(o.leaves[0], node(10, 0, 0)) && same(o.dst, {0}) && o.n_opaque == 0, "empty root");
        CHECK(number_occluders({}, {}, o) == nullptr && o.nodes.empty() && o.leaves.size() == 1 && same(o.leaves[0], DevNode{}) && o.dst.empty() && o.n_opaque == 0, "no nodes at all");
    }
    const std::vector<DevNode> t = three_leaves();
    {   // counts (0, k, all): the first leaf stays a node and leaves the list
        CHECK(number_occluders(t, {0, 3, 3}, o) == nullptr, "(0, 3, 3): refused");
        CHECK(o.nodes.size() == 5 && same(o.nodes[0], t[0]) && same(o.nodes[2], t[2]), "(0, 3, 3): inner nodes are untouched");
        CHECK(same(o.nodes[1], node(20, 0, 0)) && same(o.nodes[3], node(40, 0, 3)) && same(o.nodes[4], node(50, 3, 3)), "(0, 3, 3): runs");
        CHECK(o.leaves.size() == 2 && same(o.leaves[0], node(40, 0, 3)) && same(o.leaves[1], node(50, 3, 3)), "(0, 3, 3): leaf list");
        CHECK(same(o.dst, {0, 0, 3}) && o.n_opaque == 6, "(0, 3, 3): dst, n_opaque %zu", o.n_opaque);
    }
    {   // an empty leaf in the middle: the prefix sum passes through it
        CHECK(number_occluders(t, {2, 0, 3}, o) == nullptr, "(2, 0, 3): refused");
        CHECK(same(o.nodes[1], node(20, 0, 2)) && same(o.nodes[3], node(40, 2, 0)) && same(o.nodes[4], node(50, 2, 3)), "(2, 0, 3): runs");
        CHECK(o.leaves.size() == 2 && same(o.leaves[0], node(20, 0, 2)) && same(o.leaves[1], node(50, 2, 3)) && same(o.dst, {0, 2, 2}) && o.n_opaque == 5, "(2, 0, 3): leaf list, dst");
    }
    {   // every leaf whole
        CHECK(number_occluders(t, {4, 7, 3}, o) == nullptr, "(4, 7, 3): refused");
        CHECK(o.leaves.size() == 3 && same(o.nodes[1], t[1]) && same(o.nodes[3], t[3]) && same(o.nodes[4], t[4]) && same(o.dst, {0, 4, 11}) && o.n_opaque == 14, "(4, 7, 3)");
    }
    {   // nothing opaque anywhere: node 0, here an inner node, as a leaf of nothing
        CHECK(number_occluders(t, {0, 0, 0}, o) == nullptr, "(0, 0, 0): refused");
        CHECK(o.leaves.size() == 1 && same(o.leaves[0], node(10, 0, 0)) && o.n_opaque == 0 && same(o.dst, {0, 0, 0}), "(0, 0, 0): the placeholder leaf");
        CHECK(same(o.nodes[0], t[0]) && same(o.nodes[2], t[2]) && same(o.nodes[1], node(20, 0, 0)) && same(o.nodes[3], node(40, 0, 0)) && same(o.nodes[4], node(50, 0, 0)), "(0, 0, 0): nodes");
    }
    CHECK(number_occluders(t, {0, 8, 3}, o) != nullptr, "a count one above its leaf is accepted");
    CHECK(number_occluders(t, {4, 7, 4}, o) != nullptr, "a count one above the last leaf is accepted");
    CHECK(number_occluders(t, {4, 7}, o) != nullptr, "two counts for three leaves are accepted");

    // host_occluders: node 0 { leaf of references 0-2, leaf of references 3-4 } over four triangles, triangle 2 in both leaves
    HostTree tree;
    tree.dev_nodes = {node(10, 3, DEV_INNER), node(20, 0, 3), node(30, 3, 2)};
    tree.dev_tri_ids = {0, 1, 2, 2, 3};
    for (uint32_t r = 0; r < 5; ++r) { DevTri d{}; d.v0[0] = float(100 + r); tree.dev_tris.push_back(d); }
    for (uint32_t i = 0; i < 4; ++i) { DevShade s{}; s.material = i & 1u; tree.dev_shade.push_back(s); }       // triangles 1 and 3 of material 1
    DevMaterial diffuse{}, glass{};
    diffuse.kind = RTK_MAT_DIFFUSE; glass.kind = RTK_MAT_REFRACTIVE;
    CHECK(opaque({diffuse, glass}, 0) && !opaque({diffuse, glass}, 1) && opaque({diffuse, glass}, 2) && opaque({glass}, size_t(int32_t(-1))) && opaque({}, 0), "the predicate");
    CHECK(any_refractive({diffuse, glass}) && any_refractive({glass}) && !any_refractive({diffuse, diffuse}) && !any_refractive({}), "any_refractive");
    HostOccluders h;
    {   // material 1 refractive: references 0, 2 | 3 stay
        CHECK(host_occluders(tree, {diffuse, glass}, h) == nullptr, "one refractive material: refused");
        CHECK(h.tris.size() == 3 && h.tris[0].v0[0] == 100.f && h.tris[1].v0[0] == 102.f && h.tris[2].v0[0] == 103.f && same(h.ids, {0, 2, 2}), "one refractive material: the copy");
        CHECK(same(h.tree.nodes[0], tree.dev_nodes[0]) && same(h.tree.nodes[1], node(20, 0, 2)) && same(h.tree.nodes[2], node(30, 2, 1)) && h.tree.leaves.size() == 2 &&
              same(h.tree.leaves[0], node(20, 0, 2)) && same(h.tree.leaves[1], node(30, 2, 1)) && same(h.tree.dst, {0, 2}) && h.tree.n_opaque == 3, "one refractive material: the tree");
    }
    {   // a table of one material, refractive: triangles 1 and 3 point past it and count as opaque, references 1 | 4 stay
        CHECK(host_occluders(tree, {glass}, h) == nullptr, "index past the table: refused");
        CHECK(h.tris.size() == 2 && h.tris[0].v0[0] == 101.f && h.tris[1].v0[0] == 104.f && same(h.ids, {1, 3}), "index past the table: the copy");
        CHECK(same(h.tree.nodes[1], node(20, 0, 1)) && same(h.tree.nodes[2], node(30, 1, 1)) && h.tree.leaves.size() == 2 && same(h.tree.dst, {0, 1}) && h.tree.n_opaque == 2, "index past the table: the tree");
    }
    {   // nothing opaque: the first reference and id 0 stand in, the placeholder leaf is node 0
        CHECK(host_occluders(tree, {glass, glass}, h) == nullptr, "nothing opaque: refused");
        CHECK(h.tris.size() == 1 && h.tris[0].v0[0] == 100.f && same(h.ids, {0}) && h.tree.n_opaque == 0, "nothing opaque: one triangle, one id");
        CHECK(h.tree.leaves.size() == 1 && same(h.tree.leaves[0], node(10, 0, 0)) && same(h.tree.nodes[1], node(20, 0, 0)) && same(h.tree.nodes[2], node(30, 0, 0)), "nothing opaque: the tree");
        const DevTri zero{};
        CHECK(host_occluders(HostTree{}, {glass}, h) == nullptr && h.tris.size() == 1 && std::memcmp(&h.tris[0], &zero, sizeof(zero)) == 0 && same(h.ids, {0}) &&
              h.tree.nodes.empty() && h.tree.leaves.size() == 1, "no tree at all");
    }
    if (!g_failed) std::printf("occluders ok\n");
}

HostMesh mesh(int32_t material, std::vector<uint32_t> indices) {
    HostMesh m{};
    m.material = material; m.indices = std::move(indices);
    return m;
}

void topology() {
    DevMaterial diffuse{}, glass{};
    diffuse.kind = RTK_MAT_DIFFUSE; glass.kind = RTK_MAT_REFRACTIVE;
    // mesh 0: 4 vertices (vertex 3 in no triangle), triangles [0,0,1] and [1,2,0]; mesh 1: 2 vertices, no triangle; mesh 2: 3
    // vertices from 6 on, triangle [2,1,0], refractive.  An update has emptied the meshes' vertices: the counts are numbers.
    rtk_scene s{};
    s.materials = {diffuse, glass};
    s.meshes = {mesh(0, {0, 0, 1, 1, 2, 0}), mesh(7, {}), mesh(1, {2, 1, 0})};
    s.n_vertices = 9; s.n_triangles = 3;
    const std::vector<int32_t> nverts = {4, 2, 3};
    HostTopology h;
    CHECK(host_topology(s, nverts, h) == nullptr, "three meshes: refused");
    CHECK(same(h.index, {0, 0, 1, 1, 2, 0, 8, 7, 6}), "index: the vertex offset passes the mesh without triangles");
    CHECK(same(h.inc_off, {0, 3, 5, 6, 6, 6, 6, 7, 8, 9}), "inc_off: vertices 3, 4 and 5 have empty lists");
    CHECK(same(h.inc, {0, 1, 5, 2, 3, 4, 8, 7, 6}), "inc: ascending (triangle, corner), vertex 0 twice from triangle 0");
    CHECK(h.opaque == std::vector<uint8_t>({1, 1, 0}), "opaque flags per mesh");
    s.meshes[2].material = 2;                                                // past the table: opaque
    CHECK(host_topology(s, nverts, h) == nullptr && h.opaque == std::vector<uint8_t>({1, 1, 1}), "a material past the table");
    s.meshes[2].material = 1;
    {   // refusals: the scene copy no longer matches its counts, or is too large for 32-bit indices (asked before anything is sized)
        rtk_scene b = s; b.n_triangles = 4;
        CHECK(host_topology(b, nverts, h) != nullptr, "fewer triangles than counted");
        b = s; b.n_triangles = 2;
        CHECK(host_topology(b, nverts, h) != nullptr, "more triangles than counted");
        b = s; b.n_vertices = 10;
        CHECK(host_topology(b, nverts, h) != nullptr, "fewer vertices than counted");
        CHECK(host_topology(s, {4, 2}, h) != nullptr, "a mesh without a vertex count");
        b = s; b.meshes[2].indices[0] = 5;
        CHECK(host_topology(b, nverts, h) != nullptr, "an index past the last vertex");
        b = rtk_scene{}; b.n_triangles = 1431655761;                         // (3 * 1431655760 = 0xFFFFFFF0 is the last count within the bound)
        CHECK(host_topology(b, {}, h) != nullptr && std::strstr(host_topology(b, {}, h), "32-bit") != nullptr, "3 * 1431655761 indices are accepted");
    }
    rtk_scene none{};
    CHECK(host_topology(none, {}, h) == nullptr && h.index.empty() && same(h.inc_off, {0}) && h.inc.empty() && h.opaque.empty(), "a scene of nothing");
    if (!g_failed) std::printf("topology ok\n");
}

}  // namespace

int main() {
    caps();
    occluders();
    topology();
    if (!g_failed) std::printf("all ok\n");
    return g_failed ? 1 : 0;
}
