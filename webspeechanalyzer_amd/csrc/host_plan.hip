// host_plan.hip — the part of host_plan.hpp that launches a kernel: the level-3 raw-track gather of batches (wsa_batch_copy_tracks) and streams (wsa_stream_collect).
#include "host_plan.hpp"

namespace wsa {
// level 3, batch and streams: the segments' raw-track pieces out of the pools into one staging buffer in the order the host hands them out.
// desc per segment: {first pool entry (absolute), the base of its pool region, points, ranked ids, points / ranked ids of the segments in front};
// a stream's pool is a ring of `region` entries (a batch's is not: region = 2^63)
__global__ __launch_bounds__(256) void gather_tracks_kernel(const uint64_t* desc, uint64_t region, const int4* pts, const int32_t* rank, int4* out_pts, int32_t* out_rank) {
    const uint64_t* d = desc + 6 * (size_t)blockIdx.x;
    const uint64_t pool0 = d[0], base = d[1], n_pt = d[2], nq = d[3], np = d[4], nr = d[5];
    const uint64_t off0 = pool0 - base;
    for (uint64_t i = threadIdx.x; i < 2 * n_pt; i += 256) out_pts[2 * np + i] = pts[2 * (base + (off0 + (i >> 1)) % region) + (i & 1)];
    for (uint64_t i = threadIdx.x; i < nq; i += 256) out_rank[nr + i] = rank[base + (off0 + i) % region];
}
static void launch_gather_tracks(const uint64_t* desc, uint32_t n_segments, uint64_t region, const int4* pts, const int32_t* rank, int4* out_pts, int32_t* out_rank, hipStream_t s) {
    if (n_segments) hipLaunchKernelGGL(gather_tracks_kernel, dim3(n_segments), dim3(256), 0, s, desc, region, pts, rank, out_pts, out_rank);
}

wsa_status TrackGather::run(wsa_ctx* ctx, uint64_t region, const int4* pts, const int32_t* rank, int32_t* points, int32_t* ranked, hipStream_t s) {
    if (!(n_points + n_ranked)) return WSA_OK;
    const size_t desc_bytes = desc.size() * sizeof(uint64_t);
    const size_t o_pts = (desc_bytes + 255) & ~(size_t)255, o_rank = o_pts + (size_t)n_points * 8 * sizeof(int32_t), need = o_rank + (size_t)n_ranked * sizeof(int32_t);
    if (need > stage_cap) {
        if (d_stage) { (void)hipFree(d_stage); d_stage = nullptr; stage_cap = 0; }
        if (hipMalloc(reinterpret_cast<void**>(&d_stage), need + need / 4) != hipSuccess) { (void)hipGetLastError(); return wsa_api::fail(ctx, WSA_ERR_HIP, "no device memory for the raw-track staging buffer"); }
        stage_cap = need + need / 4;
    }
    HIP_TRY(ctx, hipMemcpyAsync(d_stage, desc.data(), desc_bytes, hipMemcpyHostToDevice, s));
    launch_gather_tracks(reinterpret_cast<const uint64_t*>(d_stage), segments(), region, pts, rank, reinterpret_cast<int4*>(d_stage + o_pts), reinterpret_cast<int32_t*>(d_stage + o_rank), s);
    HIP_TRY(ctx, hipGetLastError());
    if (n_points) HIP_TRY(ctx, hipMemcpyAsync(points, d_stage + o_pts, (size_t)n_points * 8 * sizeof(int32_t), hipMemcpyDefault, s));
    if (n_ranked) HIP_TRY(ctx, hipMemcpyAsync(ranked, d_stage + o_rank, (size_t)n_ranked * sizeof(int32_t), hipMemcpyDefault, s));
    return WSA_OK;
}
}  // namespace wsa
