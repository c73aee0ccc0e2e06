// debug_units.hip — test entries of libwsa that are NOT part of include/wsa.h, for device functions no kernel of their own exposes: the four test kernels
// below run jsmath_device.hpp's Math ports, tracker_score.hpp's match_score, gate_floor.hpp's floor law and tracker_features.hpp's 53-feature reduction
// (the very functions the gate and tracker kernels inline); wsa_debug_fe_choice names the K1 instantiation (fe_r8.hip, fe_rx.hip, fe_r3.hip) a geometry selects.
#include <cstring>
#include "api_internal.hpp"
#include "debug_internal.hpp"
#include "jsmath_device.hpp"
#include "gate_floor.hpp"
#include "tracker_score.hpp"
#include "tracker_features.hpp"

namespace wsa {
// fn 0: jsm::log10(x[i]); fn 1: jsm::pow_pos(x[i], y[i]) — the V8 Math.log10 / Math.pow ports the noise gate's
// `parseInt(Math.pow(10, t - 3) / 20)` steps depend on (ref dist/main.js:2 @B28615)
__global__ void debug_jsmath_kernel(int fn, const double* x, const double* y, double* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = fn == 0 ? jsm::log10(x[i]) : (fn == 2 ? jsm::log10_fin(x[i]) : jsm::pow_pos(x[i], y[i]));      // fn 2: the branch-free log10 of the feature reductions (positive normal arguments)
}
// rows of 8 doubles {gap, dist, track length, track bin, peak bin, track amp, peak amp, velocity} -> match_score (ref dist/main.js:2 @B37340)
__global__ void debug_score_kernel(const double* a, double* out, uint32_t n) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* r = a + 8 * (size_t)i;
    out[i] = match_score((int)r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7]);
}

// the gate's integer floor law against its f64 evaluation for every y in [lo, hi): out[0] = number of y where they differ, out[1] = the
// smallest such y, out[2] = number of y that took the f64 route inside floor_law
__global__ void debug_floor_law_kernel(uint64_t lo, uint64_t hi, unsigned long long* out) {
    unsigned long long bad = 0, first = ~0ull, exact = 0;
    for (uint64_t y = lo + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; y < hi; y += (uint64_t)gridDim.x * blockDim.x) {
        uint32_t v;
        if (floor_law_needs_exact((uint32_t)y, v)) exact++;
        if (floor_law((uint32_t)y) != floor_law_exact((uint32_t)y)) { bad++; if (y < first) first = y; }
    }
    if (bad) { atomicAdd(&out[0], bad); atomicMin(&out[1], first); }
    if (exact) atomicAdd(&out[2], exact);
}

// the 53-feature reduction on its own: ONE wavefront over n frames of nine floats.  SEL 0: formant_features_wave (frames and the event list in global
// memory); 1: formant_features_lds, frames in LDS, walking events; 2: the same with block events (no_walk); 3: block events with the frames read from
// global memory (as the generic finalize calls it for spans that do not fit its LDS block); 4: the packed form.  Writes x[5 .. 52] like the tracker's calls.
constexpr int DBG_FEAT_LDS_FRAMES = 1024;           // frames the test kernel holds in LDS (36 KB; the tracker's own blocks hold up to 288)
static_assert(DBG_FEAT_LDS_FRAMES <= FEAT_LDS_MAX, "selector 2 stays inside formant_features_lds's domain");
template <int SEL>
__global__ __launch_bounds__(64) void debug_features_kernel(const float* fr_g, int n, double ctx_max, double* x, double* aev) {
    constexpr int LDSF = SEL == 2 ? DBG_FEAT_LDS_FRAMES : (SEL == 1 ? 128 : (SEL == 4 ? 16 : 1));
    __shared__ __attribute__((aligned(16))) float s_fr[LDSF * 9];
    __shared__ __attribute__((aligned(16))) double s_red[FEAT_SCRATCH];
    const int lane = threadIdx.x;
    if (SEL == 0) { formant_features_wave(fr_g, n, ctx_max, x, aev, n + 2, lane); return; }
    const float* fr = fr_g;
    if (SEL != 3) {
        for (int q = lane; q < 9 * n && q < 9 * LDSF; q += 64) s_fr[q] = fr_g[q];
        wsync();
        fr = s_fr;
    }
    formant_features_lds(fr, n, ctx_max, x, lane, s_red, SEL == 4, SEL == 2 || SEL == 3);
}
}  // namespace wsa

using namespace wsa_debug;

extern "C" int wsa_debug_score(int32_t device, const double* args8, double* out, uint32_t n) {
    if (!args8 || !out) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; double *da = nullptr, *dout = nullptr;
    bool ok = up(A, &da, args8, (size_t)n * 8) && A.alloc(&dout, n);
    if (ok && n) {
        hipLaunchKernelGGL(wsa::debug_score_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, da, dout, n);
        ok = ran() && down(out, dout, n);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

extern "C" int wsa_debug_floor_law(int32_t device, uint64_t lo, uint64_t hi, uint64_t* out3) {
    if (!out3 || hi > (1ull << 32) || lo > hi) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; unsigned long long* d = nullptr;
    unsigned long long init[3] = {0ull, ~0ull, 0ull};
    bool ok = up(A, &d, init, 3);
    if (ok) {
        hipLaunchKernelGGL(wsa::debug_floor_law_kernel, dim3(256 * 32), dim3(256), 0, nullptr, lo, hi, d);
        ok = ran() && down(init, d, 3);
    }
    out3[0] = init[0]; out3[1] = init[1]; out3[2] = init[2];
    return ok ? WSA_OK : WSA_ERR_HIP;
}

extern "C" int wsa_debug_jsmath(int32_t device, int32_t fn, const double* x, const double* y, double* out, uint32_t n) {
    if (!x || !out || (fn == 1 && !y) || fn < 0 || fn > 2) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; double *dx = nullptr, *dy = nullptr, *dout = nullptr;
    bool ok = up(A, &dx, x, n) && A.alloc(&dy, n) && A.alloc(&dout, n);
    if (ok && y) ok = put(dy, y, n);
    if (ok && n) {
        hipLaunchKernelGGL(wsa::debug_jsmath_kernel, dim3((n + 255) / 256), dim3(256), 0, nullptr, fn, dx, dy, dout, n);
        ok = ran() && down(out, dout, n);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// selector: see debug_features_kernel; a selector outside its variant's domain (1: n <= 128, 2: n <= DBG_FEAT_LDS_FRAMES, 3: n <= FEAT_LDS_MAX, 4: n <= 15) is refused, never run.
// frames9 = n x [bin, energy, width] x 3 (host), out53 (host): [5 .. 52] are what the device function writes, [0 .. 4] (the caller's in the tracker) stay 0
extern "C" int wsa_debug_features(int32_t device, const float* frames9, uint32_t n, double ctx_max, int32_t selector, double* out53) {
    if (!frames9 || !out53 || n < 1 || n > (1u << 24) || selector < 0 || selector > 4) return WSA_ERR_INVALID;
    if ((selector == 1 && n > 128) || (selector == 2 && n > (uint32_t)wsa::DBG_FEAT_LDS_FRAMES) || (selector == 3 && n > (uint32_t)wsa::FEAT_LDS_MAX) || (selector == 4 && n > 15)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; float* dfr = nullptr; double *dx = nullptr, *daev = nullptr;
    bool ok = up(A, &dfr, frames9, (size_t)n * 9) && zeros(A, &dx, 53) && zeros(A, &daev, (size_t)3 * (n + 2));
    if (ok) {
        const int a = (int)n;
        switch (selector) {
        case 0: hipLaunchKernelGGL(wsa::debug_features_kernel<0>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 1: hipLaunchKernelGGL(wsa::debug_features_kernel<1>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 2: hipLaunchKernelGGL(wsa::debug_features_kernel<2>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        case 3: hipLaunchKernelGGL(wsa::debug_features_kernel<3>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        default: hipLaunchKernelGGL(wsa::debug_features_kernel<4>, dim3(1), dim3(64), 0, nullptr, dfr, a, ctx_max, dx, daev); break;
        }
        ok = ran() && down(out53, dx, 53);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// which K1 instantiation a geometry runs (csrc/fe_r8.hip, fe_rx.hip, fe_r3.hip fe_select_*): its name as profiles/frontend_split.md writes it, e.g.
// "fe_kernel_r8<4,5,8,true,4,3>", into buf (n bytes, zero terminated).  Plans on the host, launches nothing.
extern "C" int wsa_debug_fe_choice(wsa_ctx* ctx, double fs, char* buf, uint32_t n) {
    if (!ctx || !buf || n < 1) return WSA_ERR_INVALID;
    wsa::FePlanHost P; std::string err;
    if (!wsa::build_fe_plan(ctx->cfg, fs, P, err)) return WSA_ERR_INVALID;
    const char* name = wsa::fe_choice_name(P, wsa::Tuning::from_env().fe_fat);
    if (std::strlen(name) + 1 > n) return WSA_ERR_INVALID;
    std::strcpy(buf, name);
    return WSA_OK;
}
