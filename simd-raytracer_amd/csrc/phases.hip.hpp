// Phase diagnostic (`make phases`, -DRTK_DEBUG_PHASES, read by tools/phase_times.py): where an owner wave's cycles go
// inside k_render.  Not part of the product.  This is the only file under csrc/ that tests RTK_DEBUG_PHASES: the traversal
// and the kernel call the objects below in both builds, and in the product every one of them is empty.
// The product's device code must not move by an instruction, which decides the shapes: a Probe travels BY
// VALUE, and no product struct gets a probe or tally data member -- not even an empty one.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace rtk {
namespace dev {

// One value per pixel block, written by lane <slot> of the owner wave in place of the pixel's red channel.
// tools/phase_times.py addresses the columns by these names (PH_N_TRACE -> "n_trace"; tests/test_phase_diagnostic.py).
enum PhaseSlot : int {
    PH_TOTAL = 0,                          // cycles from the end of the prologue to the end of the block
    PH_TRACE, PH_N_TRACE,                  // cycles inside trace() with the burst wait, and the number of traces
    PH_STEPS,                              // node steps of the stack walk + candidate leaves of the leaf-list passes
    PH_N_SMALL, PH_T_SMALL, PH_C_SMALL,    // leaves the owner tested alone: how many, their triangles, cycles
    PH_N_BIG, PH_T_BIG, PH_C_BIG,          // leaves sliced over the workgroup
    PH_PROLOGUE, PH_TO_FIRST_TRACE, PH_FIRST_TRACE, PH_AFTER_FIRST_TRACE,   // cycles of a block's stretches
    PH_CHUNKS, PH_SURV, PH_CTRIS,          // owner's bundle culling: 64-triangle passes, survivors, triangles in
    PH_RT0, PH_RT1,                        // s_memrealtime (100 MHz, one clock for all CUs) at entry and end, low 24 bits
    PH_WG,                                 // blockIdx.x
    PH_WAIT,                               // cycles waiting for the helpers of a light burst
    PH_TR0, PH_TR1, PH_TR2, PH_TR3, PH_TR4, PH_TR5,               // cycles of the block's first six traces ...
    PH_KIND0, PH_KIND1, PH_KIND2, PH_KIND3, PH_KIND4, PH_KIND5,   // ... 100 + log2(parts) = light burst, else rays in the root box
    PH_C_BUND, PH_C_LIST,                  // cycles making bundles / culling the leaf list
    PH_OWN,                                // the owner's own trace of the last light burst
    PH_STG_N,                              // tri_step: triangles entered
    PH_STG_W1, PH_STG_L1, PH_STG_W2, PH_STG_L2, PH_STG_W3, PH_STG_L3,   // waves / lanes alive after det + u estimate, after u, after v
    PH_STG_L4,                             // lanes accepted
    PH_SLOTS
};

// RTK_PHASES_ONLY(code): the code in the diagnostic build, nothing in the product.  The types below are written once with it,
// so both builds see the same signatures; in the product they are empty structs with empty methods.
#ifdef RTK_DEBUG_PHASES
constexpr bool kPhases = true;
#define RTK_PHASES_ONLY(...) __VA_ARGS__
#else
constexpr bool kPhases = false;
#define RTK_PHASES_ONLY(...)
#endif

// counts, and cycles modulo 2^32 (a block runs for far less)
struct PhaseTallies { uint32_t v[PH_SLOTS] = {}; };
struct Stamp {
    RTK_PHASES_ONLY(unsigned long long t0;)
    static __device__ __forceinline__ Stamp now() { return Stamp{RTK_PHASES_ONLY(__builtin_readcyclecounter())}; }
};

// Handle to the tallies of the wave that owns the rays; null (helper waves, leaf_range_wave): every method does nothing.
struct Probe {
    RTK_PHASES_ONLY(PhaseTallies *t = nullptr;)
    __device__ __forceinline__ void add(const int slot, const uint32_t n) const { RTK_PHASES_ONLY(if (t) t->v[slot] += n;) }
    __device__ __forceinline__ void since(const Stamp s, const int slot) const { RTK_PHASES_ONLY(add(slot, (uint32_t)(__builtin_readcyclecounter() - s.t0));) }
    // tri_step: a triangle enters; the wave goes on after stage `w` (PH_STG_W1..3) with the lanes of `m`; lanes accepted
    __device__ __forceinline__ void tri() const { add(PH_STG_N, 1u); }
    __device__ __forceinline__ void alive(const int w, const unsigned long long m) const { add(w, 1u); add(w + 1, (uint32_t)__popcll(m)); }
    __device__ __forceinline__ void accepted(const unsigned long long m) const { add(PH_STG_L4, (uint32_t)__popcll(m)); }
    // one 64-triangle pass of the bundle culling
    __device__ __forceinline__ void cull_pass(const unsigned long long surv, const uint32_t tris) const { add(PH_CHUNKS, 1u); add(PH_SURV, (uint32_t)__popcll(surv)); add(PH_CTRIS, tris); }
    __device__ __forceinline__ void node_step() const { add(PH_STEPS, 1u); }
    // one 64-leaf pass of the leaf list, begun at `s`, with candidate leaves `cand`
    __device__ __forceinline__ void list_pass(const unsigned long long cand, const Stamp s) const { add(PH_STEPS, (uint32_t)__popcll(cand)); since(s, PH_C_LIST); }
    // process_leaf() of `tris` triangles, begun at `s`; sliced = the workgroup shared it
    __device__ __forceinline__ void leaf(const bool sliced, const uint32_t tris, const Stamp s) const {
        since(s, sliced ? PH_C_BIG : PH_C_SMALL); add(sliced ? PH_N_BIG : PH_N_SMALL, 1u); add(sliced ? PH_T_BIG : PH_T_SMALL, tris);
    }
};
// SliceCtx's tallies and probe().  The member exists in the diagnostic build only, comes last and has an initialiser, so the
// brace initialisers of SliceCtx are the same in both builds.
#define RTK_PHASE_TALLIES_OF_SLICECTX                   \
    RTK_PHASES_ONLY(PhaseTallies phase_tallies = {};)   \
    __device__ __forceinline__ Probe probe() { return Probe{RTK_PHASES_ONLY(&phase_tallies)}; }

// k_render's side: the stretches of a block's life and its first traces.  `p` is the owner's probe (never null).
struct FrameProbe {
    RTK_PHASES_ONLY(unsigned long long entry, rt0, begin = 0, first_trace = 0, after_first = 0, tr0 = 0, w0 = 0;)
    static __device__ __forceinline__ FrameProbe enter() { return FrameProbe{RTK_PHASES_ONLY(__builtin_readcyclecounter(), __builtin_amdgcn_s_memrealtime())}; }
    __device__ __forceinline__ void prologue_done() { RTK_PHASES_ONLY(begin = __builtin_readcyclecounter();) }
    __device__ __forceinline__ void trace_begins() { RTK_PHASES_ONLY(tr0 = __builtin_readcyclecounter(); if (first_trace == 0) first_trace = tr0;) }
    __device__ __forceinline__ void trace_returned() { RTK_PHASES_ONLY(w0 = __builtin_readcyclecounter();) }
    // after the burst's second barrier.  burst_plog = log2(parts) of a light burst, in_root = this lane's ray entered the root box
    __device__ __forceinline__ void trace_done(const Probe p, const bool burst, const bool sliced, const uint32_t burst_plog, const bool in_root) {
        RTK_PHASES_ONLY(
        p.since(Stamp{w0}, PH_WAIT);
        if (burst && sliced) p.t->v[PH_OWN] = (uint32_t)(w0 - tr0);
        for (int i = 0; i < 6; ++i) if (p.t->v[PH_N_TRACE] == (uint32_t)i) {
            p.t->v[PH_TR0 + i] = (uint32_t)(__builtin_readcyclecounter() - tr0);
            p.t->v[PH_KIND0 + i] = burst ? 100u + burst_plog : (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in_root));
        }
        p.since(Stamp{tr0}, PH_TRACE); p.add(PH_N_TRACE, 1u);
        if (after_first == 0) after_first = __builtin_readcyclecounter();)
    }
    // lane <slot> writes its value to o[0]
    __device__ __forceinline__ void write(const Probe p, const uint32_t lane, float *o) const {
        RTK_PHASES_ONLY(
        const unsigned long long now = __builtin_readcyclecounter(), rt1 = __builtin_amdgcn_s_memrealtime();
        float vals[PH_SLOTS];
        for (int i = 0; i < PH_SLOTS; ++i) vals[i] = (float)p.t->v[i];
        vals[PH_TOTAL] = (float)(now - begin);
        vals[PH_PROLOGUE] = (float)(begin - entry);
        vals[PH_TO_FIRST_TRACE] = (float)(first_trace - begin);
        vals[PH_FIRST_TRACE] = (float)(after_first - first_trace);
        vals[PH_AFTER_FIRST_TRACE] = (float)(now - after_first);
        vals[PH_RT0] = (float)(rt0 & 0xFFFFFFull);
        vals[PH_RT1] = (float)(rt1 & 0xFFFFFFull);
        vals[PH_WG] = (float)blockIdx.x;
        float v = 0.f;
        for (int i = 0; i < PH_SLOTS; ++i) v = (lane == (uint32_t)i) ? vals[i] : v;
        o[0] = v; o[1] = 0.f; o[2] = 0.f;)
    }
};

}  // namespace dev
}  // namespace rtk
