// regress_fold.hpp — specification RG-1, the device code that the batch fold (regress_fold_kernel) and the stream-step
// fold (regress_step_kernel), both in regress_fold.hip, share: one V / A / D value per callback and a running one per clip or stream,
// each row weighted as the app weights every per-syllable result, by sqrt(duration) (ref src/prediction.js:93).  The reference
// application's own attempt sums fields a regression result does not have (ref src/prediction.js:96-101), so the definition is ours;
// it is written once, here.  Device only; every translation unit that includes it gets its own copy.
#pragma once
#include "classify_fold.hpp"

namespace {

constexpr int RG_HEADS = WSA_REGRESS_GROUP_MAX;
constexpr int RG_ROW = 65;                       // doubles from one head's 64 staged terms to the next: the lanes' reads fall on distinct banks, and slot 64 takes the look-ahead read
constexpr int RG_LDS = RG_HEADS * RG_ROW;        // doubles of LDS one wave stages its terms in

// lane j's x for every lane, j the same in the whole wave (two scalar lane reads: no LDS round trip in the chain)
__device__ __forceinline__ double lane_value(double x, int j) {
    const int lo = __builtin_amdgcn_readlane(__double2loint(x), j), hi = __builtin_amdgcn_readlane(__double2hiint(x), j);
    return __hiloint2double(hi, lo);
}
__device__ __forceinline__ bool finite_d(double v) { return ((unsigned long long)__double_as_longlong(v) & 0x7ff0000000000000ull) != 0x7ff0000000000000ull; }
__device__ __forceinline__ double nan_d() { return __longlong_as_double(0x7ff8000000000000ll); }
// v w, rounded before anything is added to it (JavaScript has no fused multiply-add; as unnormalise_value of classify.hip)
__device__ __forceinline__ double weighted_term(double v, double w) {
#pragma clang fp contract(off)
    const double t = v * w;
    return t;
}

// The rows r0 .. r1 - 1 of one clip or stream, one wave (a workgroup of 64 threads), lane h < H owning head h's sums.
// Blocks of 64 rows: lane j takes row q0 + j and computes what rows do not share — d = fixed3((len + 1) step_s), w = sqrt(d), whether
// the row starts a callback, and per head whether v_h is finite and t = v_h w, staged in LDS (s, RG_LDS doubles) — then every lane walks
// the block's rows in order: the additions are chains in row order, so the bits do not depend on where the 64-row blocks fall.
// A callback's terms go to copies of the running sums A, B, which replace them when the callback closes with seg_weight > 0: a skipped
// callback leaves them untouched.  close(first row, rows, index among this walk's callbacks, skipped, cb_value, cb_weight) is called by
// all lanes; value / weight are the calling lane's head's.  t_n (batches, else NULL): [row] cleared where no callback starts.
// Returns the number of callbacks.
template <typename Close>
__device__ __forceinline__ uint32_t regress_walk(const int32_t* meta, const double* const* value, uint32_t H, double step_s, int lane, uint32_t r0, uint32_t r1,
                                                 double* s, int32_t* t_n, double& A, double& B, const Close& close) {
    const bool head = (uint32_t)lane < H;
    double S = 0.0, W = 0.0, TA = A, TB = B, seg_weight = 0.0;
    uint32_t first = r0, ncb = 0;
    bool open = false;
    const auto finish = [&](uint32_t end) {
        const bool skipped = !(seg_weight > 0.0);
        if (!skipped) { A = TA; B = TB; }
        close(first, end - first, ncb, skipped, (skipped || W == 0.0) ? nan_d() : S / W, skipped ? 0.0 : W);
        ncb++;
    };
    for (uint32_t q0 = r0; q0 < r1; q0 += 64) {
        const uint32_t q = q0 + lane;
        const bool valid = q < r1;
        double d = 0.0, w = 0.0;
        bool start = false;
        if (valid) {
            d = fixed3((double)(meta[(size_t)q * 8 + 3] + 1) * step_s);
            w = __dsqrt_rn(d);                                     // the app's ph_weight
            start = q == r0 || meta[(size_t)q * 8 + 1] != meta[(size_t)(q - 1) * 8 + 1];
            if (t_n && !start) t_n[q] = 0;
        }
        unsigned long long usable = 0;                             // lane h: the block's rows whose v_h is finite
        for (uint32_t h = 0; h < H; h++) {
            const double v = valid ? value[h][q] : 0.0;
            s[h * RG_ROW + lane] = weighted_term(v, w);
            const unsigned long long m = __ballot(valid && finite_d(v));
            if ((uint32_t)lane == h) usable = m;
        }
        const unsigned long long starts = __ballot(start);
        __syncthreads();
        const int n = (int)(r1 - q0 < 64u ? r1 - q0 : 64u);
        const double* mine = s + (head ? lane : 0) * RG_ROW;
        double t_next = mine[0];
        for (int j = 0; j < n; j++) {
            const double t = t_next;
            t_next = mine[j + 1];                                  // (slot 64 at the block's end: read, never used)
            if ((starts >> j) & 1ull) {
                if (open) finish(q0 + j);
                open = true; first = q0 + j; S = 0.0; W = 0.0; seg_weight = 0.0; TA = A; TB = B;
            }
            seg_weight += lane_value(d, j);
            const double wj = lane_value(w, j);
            if ((usable >> j) & 1ull) { S += t; W += wj; TA += t; TB += wj; }
        }
        __syncthreads();
    }
    if (open) finish(r1);
    return ncb;
}

}  // namespace
