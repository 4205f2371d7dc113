// Queue sizing of the streaming pipeline's two clients (api_stream.hip, api_radiance.hip): a frame's samples in batches, a radiance call's rays in
// chunks, and how many of either are in flight.  Plain integers, no HIP, no accel: tests/cpp/stream_plan_check.cpp runs it.
#pragma once

#include <cstdint>

namespace rtk {

constexpr uint64_t kStreamNodeBound = 0xF0000000ull;           // a launch's ray-tree nodes have 32-bit ids
// Rays of one radiance chunk at most: a chunk's ray tree goes through one lane's queues (32-bit node ids, ~120 B per node).
constexpr uint64_t kRadianceChunkRays = uint64_t(1) << 22;

// What a ray-tree node costs in a lane's queues (ensure_stream_ws), from the sizeof of dev::RayRec, dev::NodeRes, dev::HitRec, float2.
inline uint64_t stream_bytes_per_node(uint64_t ray_rec, uint64_t node_res, uint64_t hit_rec, uint64_t contrib, uint64_t n_lights) {
    return ray_rec + node_res + sizeof(uint32_t) + (hit_rec + sizeof(uint32_t) + contrib * (n_lights == 0 ? 1 : n_lights)) / 2 + 1;
}

struct FramePlan { int batch, n_launch, lanes; };              // samples per launch, launches of the pass, launches in flight at once
struct RadiancePlan { uint64_t chunk, nodes, n_chunks; int lanes; };   // rays per chunk, queue nodes of a chunk, chunks, chunks in flight

// Samples per launch (stream.hpp "batch") and batches in flight.  A batch's queues cost ~120 B per ray-tree node: the
// batch is as large as the pass, the knob and the memory budget allow (288 GB of HBM is what this design spends).
// Measured (hw15/scene2 and hw11/scene8 at the BASELINE sizes): four batches in flight, each a
// quarter of the pass, beat both more, smaller launches and fewer, larger ones (1920x1920, 16 samples, no helpers:
// 53.1 ms one sample per launch, 47.6 four, 61.6 eight in two lanes; 960x960, 8 samples: 14.4 -> 9.5 ms).
inline FramePlan plan_frame_batches(int n_pass, uint64_t nodes_per_sample, uint64_t bytes_per_node, uint64_t budget_bytes,
                                    int lanes_knob, int batch_knob) {
    const int even = (n_pass + lanes_knob - 1) / lanes_knob;
    const int want = batch_knob > 0 ? batch_knob : even;
    FramePlan f;
    f.batch = n_pass < want ? n_pass : want;
    while (f.batch > 1 && (nodes_per_sample * uint64_t(f.batch) > kStreamNodeBound ||
                           nodes_per_sample * uint64_t(f.batch) * bytes_per_node > budget_bytes)) f.batch -= 1;
    f.n_launch = (n_pass + f.batch - 1) / f.batch;
    f.lanes = f.n_launch < lanes_knob ? f.n_launch : lanes_knob;     // batches in flight at once (stream.hpp)
    while (f.lanes > 1 && nodes_per_sample * uint64_t(f.batch) * bytes_per_node * uint64_t(f.lanes) > budget_bytes) f.lanes -= 1;
    return f;
}

// Chunk size and lanes: the rule of STREAM frames with a chunk in the place of a sample, but for the cut below.
inline RadiancePlan plan_radiance_chunks(uint64_t n, uint64_t factor, uint64_t bytes_per_node, uint64_t budget_bytes, int lanes_knob) {
    auto fits = [&](uint64_t c, uint64_t l) {
        return c * factor + 4096 <= kStreamNodeBound && (c * factor + 4096) * bytes_per_node * l <= budget_bytes;
    };
    const uint64_t n64 = (n + 63) / 64 * 64;
    RadiancePlan r;
    r.chunk = n64 < kRadianceChunkRays ? n64 : kRadianceChunkRays;
    // a batch that has to be cut for the budget is cut so that every lane gets queues: the chunks then overlap as a frame's samples do
    if (!fits(r.chunk, 1)) while (r.chunk > 64 && !fits(r.chunk, uint64_t(lanes_knob))) r.chunk = (r.chunk / 2 + 63) / 64 * 64;
    r.nodes = r.chunk * factor + 4096;
    r.n_chunks = (n + r.chunk - 1) / r.chunk;
    r.lanes = r.n_chunks < uint64_t(lanes_knob) ? int(r.n_chunks) : lanes_knob;
    while (r.lanes > 1 && !fits(r.chunk, uint64_t(r.lanes))) r.lanes -= 1;
    return r;
}

}  // namespace rtk
