// featdb_keep.hpp — the storing rules of specifications FD-1 and FD-2 as the one workgroup of FD_WG threads evaluates them,
// FD_WG source rows per step of its walk: K10's keep kernel (featdb.hip, a batch's run) and the stream step's plan kernel
// (stream_featdb.hip) both call these, so that the level-12 rule is written once.  Device code only; every function here is called by
// ALL threads of the workgroup (they hold barriers).
#pragma once
#include "wsa_internal.hpp"
#include "wave_ops.hpp"

namespace wsa_fd {

constexpr int FD_WAVE = 64;                               // source rows one wave ballots
constexpr int FD_WAVES = 16;
constexpr int FD_WG = FD_WAVE * FD_WAVES;                 // source rows per step of the walk
constexpr int FD_MARK_SLOT = 23;                          // level 12: the slot that marks a thrown uncmin

struct KeepShared { uint32_t cnt[FD_WAVES], head[FD_WAVES], tail[FD_WAVES]; };

// Level 12: is source row r kept?  Row r is kept iff no row r' <= r of its callback has a slot 23 other than +-0 (NaN among it: the JS
// `!== 0`).  A callback is a RUN of rows with one (meta[0], meta[1]), which is what a compacted row table holds.  `carry` is uniform over
// the workgroup: whether the callback that is open at the end of the previous step of the walk has been marked.
__device__ __forceinline__ bool keep_l12(const int32_t* __restrict__ meta, const uint64_t* __restrict__ feat, uint32_t stride, uint64_t r, bool valid, bool& carry,
                                         KeepShared& sh) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool mark = false, head = false;
    if (valid) {
        const uint64_t bits = feat[r * (uint64_t)stride + FD_MARK_SLOT];
        mark = (bits << 1) != 0;                                          // anything but +0 and -0
        head = r == 0 || meta[r * 8] != meta[(r - 1) * 8] || meta[r * 8 + 1] != meta[(r - 1) * 8 + 1];
    }
    const uint64_t mm = __ballot(mark), hm = __ballot(head);
    const uint64_t le = wsa::lanemask_lt(lane) | (1ull << lane);
    const uint64_t h = hm & le;                                           // the callbacks that start in this wave at or before this row
    const uint64_t from = h ? (~0ull << (63 - __clzll((long long)h))) : ~0ull;
    const bool local = (mm & le & from) != 0;                             // a mark between the row's callback start (or the wave's) and the row
    if (lane == 0) {
        const uint64_t tail = hm ? (~0ull << (63 - __clzll((long long)hm))) : ~0ull;
        sh.head[wave] = hm != 0; sh.tail[wave] = (mm & tail) != 0;
    }
    __syncthreads();
    bool c = carry, cend = carry;
    for (int w = 0; w < FD_WAVES; w++) {
        cend = sh.head[w] ? sh.tail[w] != 0 : (cend || sh.tail[w] != 0);
        if (w + 1 == wave) c = cend;
    }
    if (wave == 0) c = carry;
    carry = cend;
    return valid && !(local || (h == 0 && c));
}

// The exclusive scan of one step of the walk: *before = the kept rows of this step in front of this thread's, *total = all of them.
// Ends on a barrier, so the shared words may be rewritten right after it.
__device__ __forceinline__ void scan_step(bool keep, KeepShared& sh, uint32_t* before, uint32_t* total) {
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t km = __ballot(keep);
    if (lane == 0) sh.cnt[wave] = (uint32_t)__popcll(km);
    __syncthreads();
    uint32_t b = 0, tot = 0;
    for (int w = 0; w < FD_WAVES; w++) { if (w < wave) b += sh.cnt[w]; tot += sh.cnt[w]; }
    *before = b + (uint32_t)__popcll(km & wsa::lanemask_lt(lane)); *total = tot;
    __syncthreads();
}

}  // namespace wsa_fd
