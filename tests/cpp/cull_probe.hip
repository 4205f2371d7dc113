// Test-only probe over simd-raytracer_amd/csrc/trace.hip.hpp (tests/test_gpu_cull_probe.py; `make cull_probe`).
// Every kernel runs the product's own functions -- make_bundles, pencil_misses, bundle_misses, bundle_may_hit_box, slab,
// tri_step, test_triangle and the leaf loops -- on ONE WAVE per workgroup and writes down what they return.  Nothing of
// trace.hip.hpp is copied here.  All 64 lanes of a wave are always live (the DPP reductions need them): which rays take
// part is data (`active`), and so is everything else.  Every index is bounded by the arguments of the entry point.
//
// A wave's rays travel as 12 words per lane: o.xyz, d.xyz, apex.xyz (floats), cls, active, cull (uint32).
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "trace.hip.hpp"

using namespace rtk;
using namespace rtk::dev;

namespace {

constexpr int kLaneWords = 12;
constexpr int kImage = kMaxBundles * kBundleFloats;
constexpr uint32_t kUnwritten = 0x7FC0DEADu;   // LDS floats no bundle was written to

struct LaneIn {
    Ray r;
    V3 apex;
    uint32_t cls;
    bool active, cull;
};

__device__ __forceinline__ LaneIn load_lane(const uint32_t *lanes) {
    const uint32_t *p = lanes + ((size_t)blockIdx.x * 64u + threadIdx.x) * kLaneWords;
    LaneIn L;
    L.r = make_ray(mk(__uint_as_float(p[0]), __uint_as_float(p[1]), __uint_as_float(p[2])),
                   mk(__uint_as_float(p[3]), __uint_as_float(p[4]), __uint_as_float(p[5])));
    L.apex = mk(__uint_as_float(p[6]), __uint_as_float(p[7]), __uint_as_float(p[8]));
    L.cls = p[9];
    L.active = p[10] != 0u;
    L.cull = p[11] != 0u;
    return L;
}

// make_bundles on this wave's rays; its return value, the lanes' cidx and the LDS image go out when asked for
__device__ __forceinline__ uint32_t bundles_of(const LaneIn &L, float *lds, uint32_t &cidx, uint32_t *out_n, uint32_t *out_cidx,
                                               uint32_t *out_img) {
    for (int i = (int)threadIdx.x; i < kImage; i += 64) lds[i] = __uint_as_float(kUnwritten);
    __syncthreads();
    const uint32_t n = make_bundles(L.r, L.cull, L.active, L.cls, L.apex, lds, cidx, Probe{});
    __syncthreads();
    if (out_n && threadIdx.x == 0u) out_n[blockIdx.x] = n;
    if (out_cidx) out_cidx[(size_t)blockIdx.x * 64u + threadIdx.x] = cidx;
    if (out_img)
        for (int i = (int)threadIdx.x; i < kImage; i += 64) out_img[(size_t)blockIdx.x * kImage + i] = __float_as_uint(lds[i]);
    return n;
}

__global__ __launch_bounds__(64) void k_bundles(const uint32_t *lanes, uint32_t *out_n, uint32_t *out_cidx, uint32_t *out_img) {
    __shared__ __attribute__((aligned(16))) float lds[kImage];
    const LaneIn L = load_lane(lanes);
    uint32_t cidx;
    bundles_of(L, lds, cidx, out_n, out_cidx, out_img);
}

// per (bundle, triangle): used = what leaf_range_bundle would take, pen = pencil_misses (255: not a pencil), itv = bundle_misses
__global__ __launch_bounds__(64) void k_tri_masks(const uint32_t *lanes, const float *tris, const uint32_t K, const float eps,
                                                  uint32_t *out_n, uint32_t *out_cidx, uint32_t *out_img, uint8_t *used, uint8_t *pen,
                                                  uint8_t *itv) {
    __shared__ __attribute__((aligned(16))) float lds[kImage];
    const LaneIn L = load_lane(lanes);
    uint32_t cidx;
    const uint32_t n = bundles_of(L, lds, cidx, out_n, out_cidx, out_img);
    const uint32_t lane = threadIdx.x;
    const float *wt = tris + (size_t)blockIdx.x * K * 9;
    for (uint32_t base = 0; base < K; base += 64u) {
        const bool have = base + lane < K;
        const F3 *tp = reinterpret_cast<const F3 *>(wt + (size_t)(have ? base + lane : 0u) * 9);
        const F3 v0 = tp[0], e1 = tp[1], e2 = tp[2];
        for (uint32_t k = 0; k < (uint32_t)kMaxBundles; ++k) {
            uint8_t p = 255, i = 255, u = 255;
            if (k < n) {
                const bool is_pencil = (bundle_flags(lds, k) & BUNDLE_PENCIL) != 0u;
                if (is_pencil) {
                    const PencilRegs R = load_pencil(lds, k);
                    p = pencil_misses(R, eps, v0.x, v0.y, v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z) ? 1 : 0;
                }
                const BundleRegs R = load_bundle(lds, k, false);
                i = bundle_misses(R.b, eps, v0.x, v0.y, v0.z, e1.x, e1.y, e1.z, e2.x, e2.y, e2.z) ? 1 : 0;
                u = is_pencil ? p : i;
            }
            if (have) {
                const size_t at = ((size_t)blockIdx.x * kMaxBundles + k) * K + base + lane;
                used[at] = u; pen[at] = p; itv[at] = i;
            }
        }
    }
}

// per (bundle, box): bundle_may_hit_box (255: no such bundle); per (box, ray): slab and its t_min
__global__ __launch_bounds__(64) void k_box_masks(const uint32_t *lanes, const float *boxes, const uint32_t K, uint32_t *out_n,
                                                  uint32_t *out_cidx, uint32_t *out_img, uint8_t *may, uint8_t *hit, uint32_t *tmin) {
    __shared__ __attribute__((aligned(16))) float lds[kImage];
    const LaneIn L = load_lane(lanes);
    uint32_t cidx;
    const uint32_t n = bundles_of(L, lds, cidx, out_n, out_cidx, out_img);
    const uint32_t lane = threadIdx.x;
    const float *wb = boxes + (size_t)blockIdx.x * K * 6;
    for (uint32_t base = 0; base < K; base += 64u) {
        const bool have = base + lane < K;
        const float *b = wb + (size_t)(have ? base + lane : 0u) * 6;
        for (uint32_t k = 0; k < (uint32_t)kMaxBundles; ++k) {
            uint8_t m = 255;
            if (k < n) {
                const BundleRegs R = load_bundle(lds, k, true);
                m = bundle_may_hit_box(R, b[0], b[1], b[2], b[3], b[4], b[5]) ? 1 : 0;
            }
            if (have) may[((size_t)blockIdx.x * kMaxBundles + k) * K + base + lane] = m;
        }
    }
    for (uint32_t j = 0; j < K; ++j) {
        const float *b = wb + (size_t)j * 6;
        float t_min;
        const bool h = slab(b[0], b[1], b[2], b[3], b[4], b[5], L.r, t_min);
        const size_t at = ((size_t)blockIdx.x * K + j) * 64u + lane;
        hit[at] = h ? 1 : 0;
        tmin[at] = __float_as_uint(t_min);
    }
}

// per (triangle, ray): tri_step and test_triangle from best.t = FLT_MAX with every lane passing; out: t, u, v bits, accepted
__global__ __launch_bounds__(64) void k_tri_exact(const uint32_t *lanes, const float *tris, const uint32_t K, const float eps,
                                                  uint32_t *step, uint32_t *test) {
    const LaneIn L = load_lane(lanes);
    const uint32_t lane = threadIdx.x;
    const float *wt = tris + (size_t)blockIdx.x * K * 9;
    for (uint32_t j = 0; j < K; ++j) {
        const TriS cur = load_tri_uniform((cptr_f32)(const void *)wt + (size_t)j * 9);
        Cand a = {kFltMax, 0.0f, 0.0f, kMiss}, b = a;
        tri_step(cur, j, L.r, L.cull, eps, ~0ull, lane, a, Probe{});
        const float *tp = wt + (size_t)j * 9;
        test_triangle(tp[0], tp[1], tp[2], tp[3], tp[4], tp[5], tp[6], tp[7], tp[8], L.r, L.cull, eps, j, true, b);
        const size_t at = (((size_t)blockIdx.x * K + j) * 64u + lane) * 4u;
        step[at] = __float_as_uint(a.t); step[at + 1] = __float_as_uint(a.u); step[at + 2] = __float_as_uint(a.v); step[at + 3] = a.k != kMiss;
        test[at] = __float_as_uint(b.t); test[at + 1] = __float_as_uint(b.u); test[at + 2] = __float_as_uint(b.v); test[at + 3] = b.k != kMiss;
    }
}

// the four routes through leaf references [lo, hi) of the leaf at `first`; out[wave][route][lane] = t, u, v, k
__global__ __launch_bounds__(64) void k_leaf(const uint32_t *lanes, const uint32_t *pass_in, const uint32_t *best_in, const float *exit_in,
                                             const float *tris, const uint32_t first, const uint32_t lo, const uint32_t hi,
                                             const float eps, uint32_t *out_n, uint32_t *out) {
    __shared__ __attribute__((aligned(16))) float lds[kImage];
    const LaneIn L = load_lane(lanes);
    uint32_t cidx;
    const uint32_t n = bundles_of(L, lds, cidx, out_n, nullptr, nullptr);
    const uint32_t lane = threadIdx.x;
    const size_t li = (size_t)blockIdx.x * 64u + lane;
    const bool pass = pass_in[li] != 0u;
    const float exit_t = exit_in[li];
    Cand init;
    init.t = __uint_as_float(best_in[li * 4]); init.u = __uint_as_float(best_in[li * 4 + 1]);
    init.v = __uint_as_float(best_in[li * 4 + 2]); init.k = best_in[li * 4 + 3];
    const BundleSet BS = {lds, n};
    TreeView T = {};
    T.tris = reinterpret_cast<const DevTri *>(tris);
    T.eps = eps;
    for (uint32_t route = 0; route < 4u; ++route) {
        Cand best = init;
        if (route == 0u) {
            leaf_range_wave((cptr_f32)(const void *)tris, first, lo, hi, L.r, L.cull, eps, pass, best);
        } else if (route == 3u) {
            T.scalar_surv = 0;
            leaf_range(T, first, lo, hi, L.r, L.cull, pass, cidx, BS, exit_t, best, Probe{});
        } else if (n != 0u && lo < hi) {            // without bundles there is no culling pass to run: the route keeps `init`
            leaf_range_bundle(tris, first, lo, hi, L.r, L.cull, eps, pass, cidx, BS, route == 2u, exit_t, best, Probe{});
        }
        const size_t at = (((size_t)blockIdx.x * 4u + route) * 64u + lane) * 4u;
        out[at] = __float_as_uint(best.t); out[at + 1] = __float_as_uint(best.u); out[at + 2] = __float_as_uint(best.v); out[at + 3] = best.k;
    }
}

// Host side: device copies of the inputs, outputs copied back, everything freed; the first HIP error is what the call returns.
struct Session {
    hipError_t err = hipSuccess;
    struct Out { void *host, *dev; size_t bytes; };
    std::vector<void *> bufs;
    std::vector<Out> outs;
    template <typename T>
    const T *in(const T *host, const size_t count) {
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, count ? count * sizeof(T) : sizeof(T));
        if (err == hipSuccess) bufs.push_back(d);
        if (err == hipSuccess && count) err = hipMemcpy(d, host, count * sizeof(T), hipMemcpyHostToDevice);
        return static_cast<const T *>(d);
    }
    template <typename T>
    T *out(T *host, const size_t count) {
        if (host == nullptr) return nullptr;
        void *d = nullptr;
        if (err == hipSuccess) err = hipMalloc(&d, count ? count * sizeof(T) : sizeof(T));
        if (err == hipSuccess) { bufs.push_back(d); outs.push_back(Out{host, d, count * sizeof(T)}); }
        if (err == hipSuccess && count) err = hipMemset(d, 0xEE, count * sizeof(T));
        return static_cast<T *>(d);
    }
    int finish() {
        if (err == hipSuccess) err = hipGetLastError();
        if (err == hipSuccess) err = hipDeviceSynchronize();
        for (const Out &o : outs)
            if (err == hipSuccess && o.bytes) err = hipMemcpy(o.host, o.dev, o.bytes, hipMemcpyDeviceToHost);
        for (void *p : bufs) (void)hipFree(p);
        return (int)err;
    }
};

}  // namespace

extern "C" {

int cull_probe_constants(uint32_t *out) {      // what the tests must agree with: kMaxBundles, kBundleFloats, kBundleMinTris, lane words
    out[0] = (uint32_t)kMaxBundles; out[1] = (uint32_t)kBundleFloats; out[2] = kBundleMinTris; out[3] = (uint32_t)kLaneWords;
    return 0;
}

int cull_probe_bundles(uint32_t nw, const uint32_t *lanes, uint32_t *n, uint32_t *cidx, uint32_t *img) {
    if (nw == 0u) return 0;
    Session S;
    const uint32_t *dl = S.in(lanes, (size_t)nw * 64 * kLaneWords);
    uint32_t *dn = S.out(n, nw), *dc = S.out(cidx, (size_t)nw * 64), *di = S.out(img, (size_t)nw * kImage);
    if (S.err == hipSuccess) hipLaunchKernelGGL(k_bundles, dim3(nw), dim3(64), 0, 0, dl, dn, dc, di);
    return S.finish();
}

int cull_probe_tri_masks(uint32_t nw, const uint32_t *lanes, uint32_t K, const float *tris, float eps, uint32_t *n, uint32_t *cidx,
                         uint32_t *img, uint8_t *used, uint8_t *pen, uint8_t *itv) {
    if (nw == 0u) return 0;
    if (used == nullptr || pen == nullptr || itv == nullptr) return (int)hipErrorInvalidValue;
    Session S;
    const uint32_t *dl = S.in(lanes, (size_t)nw * 64 * kLaneWords);
    const float *dt = S.in(tris, (size_t)nw * K * 9);
    uint32_t *dn = S.out(n, nw), *dc = S.out(cidx, (size_t)nw * 64), *di = S.out(img, (size_t)nw * kImage);
    const size_t cells = (size_t)nw * kMaxBundles * K;
    uint8_t *du = S.out(used, cells), *dp = S.out(pen, cells), *dv = S.out(itv, cells);
    if (S.err == hipSuccess) hipLaunchKernelGGL(k_tri_masks, dim3(nw), dim3(64), 0, 0, dl, dt, K, eps, dn, dc, di, du, dp, dv);
    return S.finish();
}

int cull_probe_box_masks(uint32_t nw, const uint32_t *lanes, uint32_t K, const float *boxes, uint32_t *n, uint32_t *cidx, uint32_t *img,
                         uint8_t *may, uint8_t *hit, uint32_t *tmin) {
    if (nw == 0u) return 0;
    if (may == nullptr || hit == nullptr || tmin == nullptr) return (int)hipErrorInvalidValue;
    Session S;
    const uint32_t *dl = S.in(lanes, (size_t)nw * 64 * kLaneWords);
    const float *db = S.in(boxes, (size_t)nw * K * 6);
    uint32_t *dn = S.out(n, nw), *dc = S.out(cidx, (size_t)nw * 64), *di = S.out(img, (size_t)nw * kImage);
    uint8_t *dm = S.out(may, (size_t)nw * kMaxBundles * K), *dh = S.out(hit, (size_t)nw * K * 64);
    uint32_t *dt = S.out(tmin, (size_t)nw * K * 64);
    if (S.err == hipSuccess) hipLaunchKernelGGL(k_box_masks, dim3(nw), dim3(64), 0, 0, dl, db, K, dn, dc, di, dm, dh, dt);
    return S.finish();
}

int cull_probe_tri_exact(uint32_t nw, const uint32_t *lanes, uint32_t K, const float *tris, float eps, uint32_t *step, uint32_t *test) {
    if (nw == 0u) return 0;
    if (step == nullptr || test == nullptr) return (int)hipErrorInvalidValue;
    Session S;
    const uint32_t *dl = S.in(lanes, (size_t)nw * 64 * kLaneWords);
    const float *dt = S.in(tris, (size_t)nw * K * 9);
    uint32_t *ds = S.out(step, (size_t)nw * K * 64 * 4), *de = S.out(test, (size_t)nw * K * 64 * 4);
    if (S.err == hipSuccess) hipLaunchKernelGGL(k_tri_exact, dim3(nw), dim3(64), 0, 0, dl, dt, K, eps, ds, de);
    return S.finish();
}

// every wave walks the same leaf: references [lo, hi) of the leaf at `first` in `tris` (n_tris triangles)
int cull_probe_leaf(uint32_t nw, const uint32_t *lanes, const uint32_t *pass, const uint32_t *best, const float *exit_t, uint32_t n_tris,
                    const float *tris, uint32_t first, uint32_t lo, uint32_t hi, float eps, uint32_t *n, uint32_t *out) {
    if (nw == 0u) return 0;
    if (out == nullptr || lo > hi || (size_t)first + hi > n_tris || n_tris == 0u) return (int)hipErrorInvalidValue;
    Session S;
    const uint32_t *dl = S.in(lanes, (size_t)nw * 64 * kLaneWords);
    const uint32_t *dp = S.in(pass, (size_t)nw * 64), *db = S.in(best, (size_t)nw * 64 * 4);
    const float *dx = S.in(exit_t, (size_t)nw * 64), *dt = S.in(tris, (size_t)n_tris * 9);
    uint32_t *dn = S.out(n, nw), *dout = S.out(out, (size_t)nw * 4 * 64 * 4);
    if (S.err == hipSuccess) hipLaunchKernelGGL(k_leaf, dim3(nw), dim3(64), 0, 0, dl, dp, db, dx, dt, first, lo, hi, eps, dn, dout);
    return S.finish();
}

}  // extern "C"
