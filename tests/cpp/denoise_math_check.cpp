// Stand-alone host program over csrc/denoise_math.hpp and csrc/denoise_plan.hpp (tests/test_denoise_model.py): the filter of
// rtk_denoise_frame, scalar, pixel by pixel in the order the plan's tiles give, on planes read from a file.  Built with the
// library's float flags, its output must equal tests/denoise_model.py in every bit.
//   usage: denoise_math_check IN OUT
//   IN:  int32 {width, height, n_images, iterations, normal_power_log2, has_noise, has_albedo, 0}, float {sigma_luminance,
//        sigma_plane, albedo_floor}, then the planes rgb, normal, position [n][h][w][3], depth [n][h][w], and those of noise
//        [n][h][w] and albedo [n][h][w][3] that the header announces.
//   OUT: rgb_out [n][h][w][3]
#include <cstdint>
#include <cstdio>
#include <vector>

#include "denoise_math.hpp"
#include "denoise_plan.hpp"

using namespace rtk;

namespace {

bool read_floats(std::FILE *f, std::vector<float> &v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(float), n, f) == n;
}

}  // namespace

int main(int argc, char **argv) {
    if (argc != 3) { std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]); return 2; }
    std::FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hd[8];
    float fl[3];
    if (std::fread(hd, sizeof(int32_t), 8, f) != 8 || std::fread(fl, sizeof(float), 3, f) != 3) { std::fprintf(stderr, "short header\n"); return 2; }
    rtk_denoise_params p;
    p.width = hd[0]; p.height = hd[1]; p.iterations = hd[3]; p.normal_power_log2 = hd[4];
    p.sigma_luminance = fl[0]; p.sigma_plane = fl[1]; p.albedo_floor = fl[2]; p.reserved = 0;
    const int32_t n_images = hd[2];
    if (const char *why = denoise_refusal(p, n_images)) { std::fprintf(stderr, "refused: %s\n", why); return 3; }
    const size_t n = size_t(p.width) * size_t(p.height) * size_t(n_images);
    std::vector<float> rgb, normal, position, depth, noise, albedo;
    if (!read_floats(f, rgb, 3 * n) || !read_floats(f, normal, 3 * n) || !read_floats(f, position, 3 * n) || !read_floats(f, depth, n) ||
        !read_floats(f, noise, hd[5] ? n : 0) || !read_floats(f, albedo, hd[6] ? 3 * n : 0)) { std::fprintf(stderr, "short planes\n"); return 2; }
    std::fclose(f);
    const float *const alb = hd[6] ? albedo.data() : nullptr;

    // prologue
    std::vector<dn::Tap> cur(n), next(n);
    std::vector<unsigned char> hit(n);
    for (size_t i = 0; i < n; ++i) {
        hit[i] = dn::is_hit(depth[i]) ? 1 : 0;
        cur[i].c = dn::prologue(&rgb[3 * i], alb ? alb + 3 * i : nullptr, hd[5] ? &noise[i] : nullptr, hit[i] != 0, p.albedo_floor);
        cur[i].g = dn::Guide{normal[3 * i], normal[3 * i + 1], normal[3 * i + 2], position[3 * i], position[3 * i + 1], position[3 * i + 2]};
    }
    next = cur;                                   // (the guides never change)
    // iterations, tile by tile as the kernel's workgroups own the pixels
    const DnTiling tiling = denoise_tiling(uint32_t(p.width), uint32_t(p.height), uint32_t(n_images));
    const float sl2 = p.sigma_luminance * p.sigma_luminance, sp2 = p.sigma_plane * p.sigma_plane;
    const int32_t W = p.width, H = p.height;
    std::vector<unsigned> seen(n);
    for (int k = 0; k < p.iterations; ++k) {
        const int32_t s = int32_t(denoise_step(k));
        for (uint64_t tile = 0; tile < tiling.n_tiles; ++tile) {
            const DnTile T = denoise_tile(tiling, tile);
            const size_t base = size_t(T.image) * size_t(W) * size_t(H);
            for (uint32_t ly = 0; ly < T.h; ++ly)
                for (uint32_t lx = 0; lx < T.w; ++lx) {
                    const int32_t x = int32_t(T.x0 + lx), y = int32_t(T.y0 + ly);
                    const size_t at = base + size_t(y) * size_t(W) + size_t(x);
                    seen[at] += 1;
                    next[at].c = cur[at].c;
                    if (!hit[at]) continue;
                    next[at].c = dn::filter_pixel(cur[at], sl2, sp2, p.normal_power_log2, [&](int dx, int dy, dn::Tap &q) -> bool {
                        const int32_t qx = x + dx * s, qy = y + dy * s;
                        if (qx < 0 || qx >= W || qy < 0 || qy >= H) return false;
                        const size_t qa = base + size_t(qy) * size_t(W) + size_t(qx);
                        if (!hit[qa]) return false;
                        q = cur[qa];
                        return true;
                    });
                }
        }
        cur.swap(next);
    }
    for (size_t i = 0; i < n; ++i)
        if (seen[i] != unsigned(p.iterations)) { std::fprintf(stderr, "pixel %zu was owned %u times in %d iterations\n", i, seen[i], p.iterations); return 4; }
    // epilogue
    std::vector<float> out(3 * n);
    for (size_t i = 0; i < n; ++i) dn::epilogue(cur[i].c, alb ? alb + 3 * i : nullptr, hit[i] != 0, p.albedo_floor, &out[3 * i]);
    std::FILE *o = std::fopen(argv[2], "wb");
    if (!o || std::fwrite(out.data(), sizeof(float), out.size(), o) != out.size() || std::fclose(o) != 0) { std::fprintf(stderr, "cannot write %s\n", argv[2]); return 2; }
    std::printf("filtered %d x %d x %d, %d iterations\n", p.width, p.height, n_images, p.iterations);
    return 0;
}
