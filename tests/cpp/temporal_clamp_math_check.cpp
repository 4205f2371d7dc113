// Stand-alone host program over csrc/temporal_clamp_math.hpp (and the temporal_math.hpp it includes) alone
// (tests/test_temporal_clamp_model.py): rtk_temporal_accumulate_clamped, scalar, pixel by pixel, on planes read from a file.  Built
// with the library's float flags, its output must equal tests/temporal_clamp_model.py in every bit.
//   usage: temporal_clamp_math_check IN OUT
//   IN:  int32 {width, height, has_prev, has_noise, has_mesh, radius, 0, 0}; 20 floats, tp::Consts in its order (cam[3], m[9], th,
//        aspect, wf, hf, nmax, alpha_min, plane_tolerance, normal_min_dot); 2 floats gamma, history_keep; the new frame's rgb,
//        position, normal [h][w][3], depth
//        [h][w], then noise [h][w] and mesh [h][w] (uint32) as announced; with has_prev the history's rgb, position, normal, depth,
//        length, and noise and mesh as announced.
//   OUT: rgb [h][w][3], noise [h][w] if has_noise, length [h][w]
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "temporal_clamp_math.hpp"

using namespace rtk;

namespace {

template <typename T>
bool read_words(std::FILE *f, std::vector<T> &v, size_t n) {
    static_assert(sizeof(T) == 4, "planes are 4-byte words");
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

struct Frame {
    std::vector<float> rgb, position, normal, depth, length, noise;
    std::vector<uint32_t> mesh;
    bool read(std::FILE *f, size_t n, bool history, bool has_noise, bool has_mesh) {
        return read_words(f, rgb, 3 * n) && read_words(f, position, 3 * n) && read_words(f, normal, 3 * n) && read_words(f, depth, n) &&
               read_words(f, length, history ? n : 0) && read_words(f, noise, has_noise ? n : 0) && read_words(f, mesh, has_mesh ? n : 0);
    }
};

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[8];
    float fl[20], ck[2];
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8 || std::fread(fl, sizeof(float), 20, f) != 20 || std::fread(ck, sizeof(float), 2, f) != 2) { std::fprintf(stderr, "short header\n"); return 2; }
    const int32_t W = hd[0], H = hd[1];
    const bool has_prev = hd[2] != 0, has_noise = hd[3] != 0, has_mesh = hd[4] != 0;
    const int32_t R = hd[5];
    if (W < 1 || H < 1 || W > 16384 || H > 16384 || R < 1 || R > 3) { std::fprintf(stderr, "bad size or radius\n"); return 3; }
    tp::Consts k;
    static_assert(sizeof(tp::Consts) == 20 * sizeof(float), "the header holds tp::Consts");
    std::memcpy(&k, fl, sizeof(k));
    const size_t n = size_t(W) * size_t(H);
    Frame cur, prev;
    if (!cur.read(f, n, false, has_noise, has_mesh) || (has_prev && !prev.read(f, n, true, has_noise, has_mesh))) { std::fprintf(stderr, "short planes\n"); return 2; }
    std::fclose(f);

    std::vector<float> o_rgb(3 * n), o_noise(has_noise ? n : 0), o_length(n);
    size_t n_clamped = 0;
    for (int32_t y = 0; y < H; ++y)
        for (int32_t x = 0; x < W; ++x) {
            const size_t at = size_t(y) * size_t(W) + size_t(x);
            tp::Pixel p = {};
            for (int i = 0; i < 3; ++i) p.c[i] = cur.rgb[3 * at + i];
            p.var = has_noise ? cur.noise[at] * cur.noise[at] : 1.0f;
            p.depth = cur.depth[at];
            bool blended = false;
            tp::Sums s;
            if (has_prev && tp::is_hit(p.depth)) {
                for (int i = 0; i < 3; ++i) { p.P[i] = cur.position[3 * at + i]; p.n[i] = cur.normal[3 * at + i]; }
                blended = tp::history(k, p, s, [&](int qx, int qy, tp::Tap &q) -> bool {
                    if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
                    const size_t aq = size_t(qy) * size_t(W) + size_t(qx);
                    if (!tp::tap_alive(prev.depth[aq], prev.length[aq])) return false;
                    if (has_mesh && prev.mesh[aq] != cur.mesh[at]) return false;
                    if (!tp::tap_on_surface(k, p, &prev.normal[3 * aq], &prev.position[3 * aq])) return false;
                    for (int i = 0; i < 3; ++i) q.c[i] = prev.rgb[3 * aq + i];
                    q.var = has_noise ? prev.noise[aq] * prev.noise[aq] : 1.0f;
                    q.length = prev.length[aq];
                    return true;
                });
            }
            if (blended) {
                tp::Box box = tp::box_empty();
                for (int32_t dy = -R; dy <= R; ++dy)
                    for (int32_t dx = -R; dx <= R; ++dx) {
                        const int32_t qx = x + dx, qy = y + dy;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) continue;
                        const size_t aq = size_t(qy) * size_t(W) + size_t(qx);
                        if (!tp::is_hit(cur.depth[aq])) continue;
                        if (has_mesh && cur.mesh[aq] != cur.mesh[at]) continue;
                        tp::box_add(box, &cur.rgb[3 * aq], has_noise ? cur.noise[aq] * cur.noise[aq] : 1.0f);
                    }
                bool was = false;
                const tp::Blend b = tp::blend_clamped(k, ck[0], ck[1], p, s, box, &was);
                n_clamped += was ? 1u : 0u;
                for (int i = 0; i < 3; ++i) o_rgb[3 * at + i] = b.c[i];
                if (has_noise) o_noise[at] = b.noise;
                o_length[at] = b.length;
            } else {                                   // the bits pass through (a copy of the words: a signalling NaN stays one)
                std::memcpy(&o_rgb[3 * at], &cur.rgb[3 * at], 3 * sizeof(float));
                if (has_noise) std::memcpy(&o_noise[at], &cur.noise[at], sizeof(float));
                o_length[at] = 1.0f;
            }
        }
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(o_rgb.data(), sizeof(float), o_rgb.size(), o) != o_rgb.size() ||
        (has_noise && std::fwrite(o_noise.data(), sizeof(float), o_noise.size(), o) != o_noise.size()) ||
        std::fwrite(o_length.data(), sizeof(float), o_length.size(), o) != o_length.size() || std::fclose(o) != 0) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 2;
    }
    std::printf("accumulated %d x %d, radius %d, %s, clamped %zu\n", W, H, R, has_prev ? "with a history" : "no history", n_clamped);
    return 0;
}
