// Stand-alone host program over csrc/motion_math.hpp alone (tests/test_motion_model.py): rtk_render_motion, scalar, pixel by pixel,
// on planes read from a file.  Built with the library's float flags, its output must equal tests/motion_model.py in every bit.
//   usage: motion_math_check IN OUT
//   IN:  int32 {width, height, n_triangles, n_vertices, want_prev_position, want_motion, 0, 0}; 20 floats, tp::Consts in its order
//        (cam[3], m[9], th, aspect, wf, hf, then four words that are not read); tri [h][w] (uint32), bary [h][w][2], the global
//        vertex ids [n_triangles][3] (uint32), the previous pose [n_vertices][3]
//   OUT: prev_position [h][w][3] if wanted, then motion [h][w][2] if wanted
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "motion_math.hpp"

using namespace rtk;

namespace {

template <typename T>
bool read_words(std::FILE *f, std::vector<T> &v, size_t n) {
    static_assert(sizeof(T) == 4, "planes are 4-byte words");
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[8];
    float fl[20];
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8 || std::fread(fl, sizeof(float), 20, f) != 20) { std::fprintf(stderr, "short header\n"); return 2; }
    const int32_t W = hd[0], H = hd[1];
    const bool want_position = hd[4] != 0, want_motion = hd[5] != 0;
    if (W < 1 || H < 1 || W > 16384 || H > 16384 || hd[2] < 0 || hd[3] < 0 || (!want_position && !want_motion)) { std::fprintf(stderr, "bad header\n"); return 3; }
    const uint32_t n_tris = uint32_t(hd[2]), n_verts = uint32_t(hd[3]);
    tp::Consts k;
    static_assert(sizeof(tp::Consts) == 20 * sizeof(float), "the header holds tp::Consts");
    std::memcpy(&k, fl, sizeof(k));
    const size_t n = size_t(W) * size_t(H);
    std::vector<uint32_t> tri, index;
    std::vector<float> bary, verts;
    if (!read_words(f, tri, n) || !read_words(f, bary, 2 * n) || !read_words(f, index, 3 * size_t(n_tris)) || !read_words(f, verts, 3 * size_t(n_verts))) {
        std::fprintf(stderr, "short planes\n");
        return 2;
    }
    std::fclose(f);
    for (uint32_t v : index) if (v >= n_verts) { std::fprintf(stderr, "an id that is no vertex\n"); return 3; }

    std::vector<float> o_position(want_position ? 3 * n : 0), o_motion(want_motion ? 2 * n : 0);
    size_t hits = 0;
    for (int32_t y = 0; y < H; ++y)
        for (int32_t x = 0; x < W; ++x) {
            const size_t at = size_t(y) * size_t(W) + size_t(x);
            const uint32_t id = tri[at];
            float P[3] = {0.0f, 0.0f, 0.0f};
            const bool hit = mv::is_hit(id, n_tris);
            if (hit) {
                const uint32_t *const ids = &index[3 * size_t(id)];
                mv::surface_point(&verts[3 * size_t(ids[0])], &verts[3 * size_t(ids[1])], &verts[3 * size_t(ids[2])], bary[2 * at], bary[2 * at + 1], P);
                ++hits;
            }
            if (want_position) for (int i = 0; i < 3; ++i) o_position[3 * at + i] = P[i];
            if (want_motion) {
                float m[2];
                const uint32_t miss[2] = {mv::kMissBits, mv::kMissBits};
                std::memcpy(m, miss, sizeof(m));
                if (hit) (void)mv::motion_of(k, P, uint32_t(x), uint32_t(y), m[0], m[1]);
                std::memcpy(&o_motion[2 * at], m, sizeof(m));
            }
        }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o || (want_position && std::fwrite(o_position.data(), sizeof(float), o_position.size(), o) != o_position.size()) ||
        (want_motion && std::fwrite(o_motion.data(), sizeof(float), o_motion.size(), o) != o_motion.size()) || std::fclose(o) != 0) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("motion of %d x %d, %zu hits\n", W, H, hits);
    return 0;
}
