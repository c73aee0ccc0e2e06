// tracker_features.hpp — formant_features (ref dist/main.js:2 @B32369): the 53-feature reduction of the tracker's finalize, in its three device forms
// (formant_features_wave, formant_features_lds with its two event implementations, formant_columns_packed).  A header of its own so that the test entry
// wsa_debug_features (debug_units.hip, tests/test_gpu_units.py) runs the very functions the tracker kernels inline.
#pragma once
#include "wsa_internal.hpp"
#include "jsmath_device.hpp"
#include "wave_ops.hpp"

namespace wsa {

// formant_features (ref @B32369) for all three formant columns, executed by the whole wave.
// Per-frame quantities (validity, dB = 20 log10 E, the products, neighbour differences, run starts)
// are computed with lane = frame and reduced with wave sums (a fixed tree instead of the reference's
// left-to-right order: differences of a few ulp, far inside the 1e-4 feature tolerance); only the
// energy peak-then-halve state machine (L, S) is inherently sequential and runs on lanes 0..2
// (lane = formant).  Writes x[5 .. 52]; the caller writes x[0 .. 4].
__device__ __forceinline__ void formant_features_wave(const float* fr, int a, double ctx_max, double* x, double* Aev, int aev_stride, int lane) {
    double res[16];
#pragma unroll 1
    for (int n = 0; n < 3; n++) {
        double sc = 0, sw = 0, sM = 0, sT = 0, sK = 0, sKpos = 0, up = 0, dn = 0;
        uint32_t cnt = 0, runs = 0, nKpos = 0;
        int carry_valid = 0; float carry_r = 0.f;
        for (int base = 0; base < a; base += 64) {
            const int t = base + lane;
            float rf = 0.f, Ef = 0.f, wf = 0.f;
            if (t < a) { rf = fr[9 * t + 3 * n]; Ef = fr[9 * t + 3 * n + 1]; wf = fr[9 * t + 3 * n + 2]; }
            const bool valid = t < a && rf > 0.f && Ef > 0.f;
            int pv = __shfl_up((int)valid, 1, 64); float pr = __shfl_up(rf, 1, 64);
            if (lane == 0) { pv = carry_valid; pr = carry_r; }
            carry_valid = read_lane_i32((int)valid, 63); carry_r = __builtin_bit_cast(float, read_lane_i32(__builtin_bit_cast(int, rf), 63));
            if (valid) {
                const double r = rf, E = Ef, wd = wf, dB = 20 * jsm::log10(E);
                sc += r * dB; sw += r; sM += wd * dB; sT += E; sK += dB;
                if (dB > 0) { sKpos += dB; nKpos++; }
                cnt++;
                if (pv) { const double dl = r - (double)pr; if (dl > 1) up += dl; else if (dl < -1) dn += -1 * dl; }
                else runs++;
            }
        }
        { double r8[8] = {sc, sw, sM, sT, sK, sKpos, up, dn}; wave_sums_f64(r8); sc = r8[0]; sw = r8[1]; sM = r8[2]; sT = r8[3]; sK = r8[4]; sKpos = r8[5]; up = r8[6]; dn = r8[7]; }
        const double m = wave_sum_u32(cnt), nruns = wave_sum_u32(runs), nkp = wave_sum_u32(nKpos);
#pragma unroll
        for (int q = 0; q < 16; q++) res[q] = 0;
        if (nruns > 0) {
            const double mw = sw / m, mk = sKpos / nkp;
            double vw = 0, vk = 0;
            for (int base = 0; base < a; base += 64) {
                const int t = base + lane;
                if (t < a) {
                    const float rf = fr[9 * t + 3 * n], Ef = fr[9 * t + 3 * n + 1];
                    if (rf > 0.f && Ef > 0.f) {
                        const double d1 = (double)rf - mw, d2 = 20 * jsm::log10((double)Ef) - mk;
                        vw += d1 * d1; vk += d2 * d2;
                    }
                }
            }
            { double r2[2] = {vw, vk}; wave_sums_f64(r2); vw = r2[0]; vk = r2[1]; }
            res[4] = sT / a * 100 / ctx_max; res[5] = sT / m * 100 / ctx_max;
            res[0] = sc / sK; res[1] = sqrt(vw / m); res[6] = sM / sK; res[2] = mk; res[3] = sqrt(vk / m);
        }
        res[7] = m; res[8] = nruns; res[9] = up; res[10] = dn; res[15] = 100 * m / a;
        // keep sK / m for the event statistics of this column
        const double meanK = sK / m;
        if (lane == n) {
            // energy peak-then-halve events (sequential in the frame order)
            double* A = Aev + (size_t)n * aev_stride;
            bool prev = false; double S = 0, L = 0; int nA = 0;
            for (int t = 0; t < a; t++) {
                const float rf = fr[9 * t + 3 * n], Ef = fr[9 * t + 3 * n + 1];
                if (rf > 0.f && Ef > 0.f) {
                    const double E = Ef;
                    if (prev) {
                        if (E > L) { L = E; S = 1; }
                        else if (S == 1 && E < L / 2) { if (L > 10) A[nA++] = 20 * jsm::log10(E); L = 0; S = -1; }
                    }
                    prev = true;
                } else { prev = false; S = 0; L = 0; }
            }
            res[11] = nA;
            if (nA > 0 && nruns > 0) {
                double sa = 0, na = 0;
                for (int q = 0; q < nA; q++) if (A[q] > 0) { sa += A[q]; na += 1; }
                const double ma = sa / na;
                double va = 0;
                for (int q = 0; q < nA; q++) { const double d = A[q] - ma; va += d * d; }
                res[12] = ma; res[13] = sqrt(va / nA); res[14] = 100 * (ma / meanK - 1);
            }
            if (!(nruns > 0)) res[11] = 0;
#pragma unroll
            for (int q = 0; q < 16; q++) x[5 + 16 * n + q] = res[q];
        }
    }
}


// Energy peak-then-halve events (ref @B32369: `E > L ? (L = E, S = 1) : S == 1 && E < L / 2 && (L > 10 && events.push(...), L = 0, S = -1)`,
// state cleared by every invalid frame) of one 64-frame block, lane = frame.  The reference walks the frames one by one; here the walk
// advances per RUN of valid frames and per EVENT: inside a run the state is a running maximum L (S == 1 exactly when L > 0: valid frames
// have E > 0), so the next event is the first frame whose energy is below half the maximum of the frames before it — an exclusive
// prefix-max scan, a compare and a ballot.  Energies are fp32 values, so the scan and the compares run in fp32 (max, x 0.5 and the
// comparisons are exact there).  vm = valid frames, Ef = this lane's energy, Ep = the previous lane's, run_on = frame 0 continues a run of
// the block before, L = its running maximum (in: carried, out: state behind frame 63).  Returns the mask of event frames.
__device__ __forceinline__ uint64_t energy_events_block(uint64_t vm, float Ef, float Ep, bool run_on, float& L, int lane) {
    uint64_t ev = 0ull;
    int c = 0;
    bool cont = run_on;
    for (;;) {
        const uint64_t rest = c >= 64 ? 0ull : (vm >> c) << c;
        if (!rest) break;
        const int j0 = __ffsll((long long)rest) - 1;                       // first valid frame at or after c
        int s;                                                             // first frame that is compared
        if (j0 == c && cont) s = j0;                                       // the run comes over from the block before
        else { s = j0 + 1; L = 0.f; }                                      // a run starts: its first frame only clears the state
        const uint64_t inv = j0 >= 63 ? 0ull : (~vm >> (j0 + 1)) << (j0 + 1);
        const int e = inv ? __ffsll((long long)inv) - 1 : 64;              // the run is [j0, e)
        while (s < e) {
            // X = max of the run's energies in [s, lane): inclusive max-scan of the previous lane's energy over lanes (s, e]
            const uint32_t src = (lane > s && lane <= e) ? __builtin_bit_cast(uint32_t, Ep) : 0u;
            const float X = __builtin_bit_cast(float, wave_incl_scan_max_u32(src));
            const float before = X > L ? X : L;
            const uint64_t hm = __ballot(lane >= s && lane < e && Ef < before * 0.5f);
            if (!hm) {
                // no event: the run's maximum becomes the state
                const int last = e - 1;
                const float bl = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, before), last));
                const float el = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, Ef), last));
                L = el > bl ? el : bl;
                break;
            }
            const int jh = __ffsll((long long)hm) - 1;
            const float bh = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, before), jh));
            if (bh > 10.f) ev |= 1ull << jh;
            L = 0.f; s = jh + 1;
        }
        if (e >= 64) break;
        c = e; cont = false; L = 0.f;
    }
    return ev;
}

constexpr int FEAT_FX = 18;                          // per column: 15 sums / counts, a zero and a one for the lanes without a quotient
// ---- the same features for inputs of at most 15 frames (the syllables of level 13: 15 frames on average), ALL THREE formant columns at once: lane 16 n + t = frame t
// of column n.  Lanes 16 n + 15 and 48 .. 63 hold no frame, so a run of valid frames never crosses into the next column and energy_events_block walks the three
// columns' runs in one call.  Every sum keeps the tree it has in formant_features_lds, where a column's frames sit in lanes 0 .. 14: the f64 sums that go through
// the LDS transposition are two octet sums added (the other six octets only contribute exact zeros there), the event sum is the in-row Kogge-Stone scan (rows
// 1 .. 3 are zeros there), the counts are integers — so the rows are bit-identical to the one-column-at-a-time form (tests: WSA_DBG bit 65536 switches this off).
template <int CTRL>
__device__ __forceinline__ uint32_t dpp_row_u32(uint32_t v) { return (uint32_t)__builtin_amdgcn_mov_dpp((int)v, CTRL, 0xf, 0xf, true); }
__device__ __forceinline__ uint32_t row_allsum_u32(uint32_t v) {          // every lane of a row of 16 receives the row's sum
    v += dpp_row_u32<0x128>(v); v += dpp_row_u32<0x124>(v); v += dpp_row_u32<0x122>(v); v += dpp_row_u32<0x121>(v);
    return v;
}
// (a function of its own — called, not inlined: inlined into the finalize loop it cost the kernel 21 spilled vector registers —, so the two LDS pointers arrive as
//  generic ones and are cast back to the LDS address space: ds_ instructions, not flat ones)
typedef __attribute__((address_space(3))) const float lds_cf;
typedef __attribute__((address_space(3))) double lds_d;
__device__ __attribute__((noinline)) void formant_columns_packed(const float* fr_g, int a, int lane, double* red_g) {
    lds_cf* const fr = (lds_cf*)fr_g;
    lds_d* const red = (lds_d*)red_g;
    lds_d* const fx = red + 8 * 64;
    lds_d* const col = red + 5 * 64;                     // [3][8]: the columns' f64 totals (rows 5 .. 7 of the reduction scratch are free)
    const int n = lane >> 4, t = lane & 15;
    const bool in = n < 3 && t < a;
    float rf = 0.f, Ef = 0.f, wf = 0.f;
    if (in) { rf = fr[9 * t + 3 * n]; Ef = fr[9 * t + 3 * n + 1]; wf = fr[9 * t + 3 * n + 2]; }
    const bool valid = in && rf > 0.f && Ef > 0.f;
    int pv = __shfl_up((int)valid, 1, 64); float pr = __shfl_up(rf, 1, 64);
    if (lane == 0) { pv = 0; pr = 0.f; }                 // (a column's first lane looks at the frameless lane in front of it: not valid)
    const uint64_t vm = __ballot(valid);
    const float Ep = __shfl_up(Ef, 1, 64);
    float evL = 0.f;
    const uint64_t ev = energy_events_block(vm, Ef, Ep, false, evL, lane);
    const bool my_event = ((ev >> lane) & 1ull) != 0ull;
    const int nA = __popcll(ev & (0xffffull << (lane & 48)));
    double sc = 0, sM = 0, sT = 0, sK = 0, sKpos = 0, sa = 0, dB = 0;
    uint32_t cnt = 0, runs = 0, nKpos = 0, na = 0, swi = 0, upi = 0, dni = 0;
    if (valid) {
        const double r = rf, E = Ef, wd = wf;
        dB = 20 * jsm::log10_fin(E);
        sc += r * dB; swi += (uint32_t)rf; sM += wd * dB; sT += E; sK += dB;
        if (dB > 0) { sKpos += dB; nKpos++; }
        cnt++;
        if (pv) { const int dl = (int)rf - (int)pr; if (dl > 1) upi += (uint32_t)dl; else if (dl < -1) dni += (uint32_t)(-dl); }
        else runs++;
        if (my_event && dB > 0) { sa += dB; na++; }
    }
    // ---- the column's sums.  f64 through the LDS transposition: lane (k = lane >> 3, h = lane & 7) adds octet h of row k, lane ^ 1 completes a column
    red[0 * 64 + lane] = sc; red[1 * 64 + lane] = sM; red[2 * 64 + lane] = sT; red[3 * 64 + lane] = sK; red[4 * 64 + lane] = sKpos;
    wsync();
    {
        double s = 0;
        if ((lane >> 3) < 5) {
            const lds_d* r = red + (lane >> 3) * 64 + (lane & 7) * 8;
            s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        }
        s += dpp_f64_perm<0xB1>(s);
        // the event sum: inclusive scan inside the row of 16 (the row's last lane holds the column's sum)
        sa += dpp_f64_row<0x111>(sa); sa += dpp_f64_row<0x112>(sa); sa += dpp_f64_row<0x114>(sa); sa += dpp_f64_row<0x118>(sa);
        wsync();
        if ((lane >> 3) < 5 && (lane & 7) < 6 && !(lane & 1)) col[((lane & 7) >> 1) * 8 + (lane >> 3)] = s;
        if (t == 15 && n < 3) col[n * 8 + 5] = sa;
    }
    const double sw = row_allsum_u32(swi), up = row_allsum_u32(upi), dn = row_allsum_u32(dni);
    const double m = row_allsum_u32(cnt), nruns = row_allsum_u32(runs), nkp = row_allsum_u32(nKpos);
    const uint32_t na_t = row_allsum_u32(na);
    wsync();
    const int nc = n < 3 ? n : 0;
    const double c_sKpos = col[nc * 8 + 4], c_sa = col[nc * 8 + 5];
    double ma = 0, mk = 0, vw = 0, vk = 0, va = 0;
    const bool on = nruns > 0;
    if (on) {
        const double mw = sw / m;
        mk = c_sKpos / nkp;
        if (nA > 0) ma = c_sa / (double)na_t;
        if (valid) {
            const double d1 = (double)rf - mw, d2 = dB - mk;
            vw += d1 * d1; vk += d2 * d2;
            if (my_event) { const double d3 = dB - ma; va += d3 * d3; }
        }
    }
    wsync();
    red[0 * 64 + lane] = vw; red[1 * 64 + lane] = vk; red[2 * 64 + lane] = va;
    wsync();
    {
        double s = 0;
        if ((lane >> 3) < 3) {
            const lds_d* r = red + (lane >> 3) * 64 + (lane & 7) * 8;
            s = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        }
        s += dpp_f64_perm<0xB1>(s);
        wsync();
        if ((lane >> 3) < 3 && (lane & 7) < 6 && !(lane & 1)) col[((lane & 7) >> 1) * 8 + 5 + (lane >> 3)] = s;      // [n][5 .. 7] = vw, vk, va (the event sum has been read)
    }
    wsync();
    if (t == 0 && n < 3) {
        lds_d* f = fx + n * FEAT_FX;
        const lds_d* c = col + n * 8;
        f[0] = c[0]; f[1] = c[3]; f[2] = on ? c[5] : 0.0; f[3] = m; f[4] = on ? c[6] : 0.0; f[5] = c[2]; f[6] = c[1]; f[7] = ma; f[8] = on ? c[7] : 0.0; f[9] = (double)nA; f[10] = nruns;
        f[11] = up; f[12] = dn; f[13] = mk; f[14] = (double)a; f[15] = 0.0; f[16] = 1.0;
    }
}

// The same feature computation for frames that live in LDS (the usual case; `fr` must be derived from a __shared__
// array so that the compiler emits ds_ reads).  Differences from the version above: the energy peak-then-halve state
// machine does not re-read the frames one by one through memory — lane t already holds frame t's energy, so the wave
// walks the valid frames of a 64-frame block with v_readlane and each lane notes whether its frame is an event
// (bit b of the 32-bit `myev` for block b) — and the event statistics are wave sums over those lanes.
// DOMAIN: at most FEAT_LDS_MAX = 2048 frames (32 blocks).  Block b + 32 would share block b's event bit, and the bin-jump sums below are sized for 32
// blocks; every caller keeps longer inputs away from this function (formant_features_wave has no limit).
// `red` = an LDS scratch of FEAT_SCRATCH doubles: the f64 reductions go through it (wave_sums_f64_lds) and the sixteen results of ALL THREE columns are
// evaluated together at the end — lane 16 n + q takes result q of column n: one division, one dependent division and one square root for the 48 of them
// instead of that block once per column; every value is the same IEEE operation on the same operands either way.
constexpr int FEAT_SCRATCH = 8 * 64 + 3 * FEAT_FX;   // doubles
constexpr int FEAT_LDS_MAX = 2048;                   // frames formant_features_lds takes
__device__ __forceinline__ void formant_features_lds(const float* fr, int a, double ctx_max, double* x, int lane, double* red, bool packed = false, bool no_walk = false) {
    double* const fx = red + 8 * 64;
    // ---- energy peak-then-halve events of inputs of at most 128 frames (every segment finalize_lds takes, every syllable): lanes 0 .. 2 walk the frames of
    //      columns 0 .. 2 one after the other — the reference's own walk, three columns at a time, ~16 instructions per frame for all of them — and keep the event
    //      frames as bit masks (evw0: frames 0 .. 63, evw1: 64 .. 127).  energy_events_block (a max-scan, a ballot and a branch per run and per event of ONE
    //      column: ~1 400 instructions for the three columns of a 48-frame segment against ~800 here) serves the longer ones.  Same fp32 comparisons, same events.
    uint32_t evq0 = 0, evq1 = 0, evq2 = 0, evq3 = 0;
    const bool walk = a <= 128 && !packed && !no_walk;          // (no_walk: WSA_DBG bit 131072, the equivalence test of the two event implementations)
    if (walk && lane < 3) {
        const float* c = fr + 3 * lane;
        bool prev = false; float L = 0.f;
        auto group = [&](int t0) __attribute__((always_inline)) -> uint32_t {      // frames t0 .. t0 + 31, four at a time: the reads of four frames ahead of their updates
            uint32_t bits = 0;
            const int lim = min(32, a - t0);
            auto four = [&](int q0, bool tail) __attribute__((always_inline)) {
                float r_[4], e_[4];
#pragma unroll
                for (int k = 0; k < 4; k++) { const int t = tail ? min(t0 + q0 + k, a - 1) : t0 + q0 + k; r_[k] = c[9 * t]; e_[k] = c[9 * t + 1]; }
                uint32_t b4 = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const bool valid = (!tail || q0 + k < lim) && r_[k] > 0.f && e_[k] > 0.f;
                    const bool eff = valid && prev;                              // the run's first frame only opens it (ref `if (prev) {...} prev = true`)
                    const bool ev = eff && e_[k] < L * 0.5f;                     // S == 1 exactly when L > 0, and then E < L / 2 excludes E > L
                    if (ev && L > 10.f) b4 |= 1u << k;
                    float mx; asm("v_max_f32 %0, %1, %2" : "=v"(mx) : "v"(L), "v"(e_[k]));      // (fmaxf would quiet both operands first: neither can be a NaN here)
                    L = (eff && !ev) ? mx : 0.f;                                 // (a frame that opens a run finds L == 0 and leaves it there)
                    prev = valid;
                }
                bits |= b4 << q0;
            };
            int q0 = 0;
#pragma unroll 1
            for (; q0 + 4 <= lim; q0 += 4) four(q0, false);
            if (q0 < lim) four(q0, true);
            return bits;
        };
        evq0 = group(0);
        if (a > 32) evq1 = group(32);
        if (a > 64) evq2 = group(64);
        if (a > 96) evq3 = group(96);
    }
    if (packed) formant_columns_packed(fr, a, lane, red);
    else
#pragma unroll 1
    for (int n = 0; n < 3; n++) {
        double sc = 0, sM = 0, sT = 0, sK = 0, sKpos = 0, sa = 0;
        uint32_t myev = 0;
        uint32_t swi = 0, udi = 0;                           // sums of bins; of upward | downward << 16 bin differences: a jump is at most 254 (bins 1 .. 255), so a lane's share of either stays below 254 x 32 < 2^13 over 32 blocks
        int cnt = 0, runs = 0, nKpos = 0, na = 0;            // counts of lanes: ballots and scalar popcounts, not wave sums
        int carry_valid = 0, nA = 0; float carry_r = 0.f;
        float evL = 0.f;                                     // running maximum L of the reference's scan (uniform across the wave)
        double dB_first = 0;                                 // dB of this lane's frame in the first block: the second pass reuses it (most segments are one block)
#pragma unroll 1
        for (int base = 0, b = 0; base < a; base += 64, b++) {
            const int t = base + lane;
            float rf = 0.f, Ef = 0.f, wf = 0.f;
            if (t < a) { rf = fr[9 * t + 3 * n]; Ef = fr[9 * t + 3 * n + 1]; wf = fr[9 * t + 3 * n + 2]; }
            const bool valid = t < a && rf > 0.f && Ef > 0.f;
            const uint64_t vm = __ballot(valid);
            // the lane before (DPP wave_shr:1; lane 0: the block before)
            int pv = (int)((vm << 1) >> lane) & 1;
            float pr = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, rf), 0x138, 0xf, 0xf, false));
            if (lane == 0) { pv = carry_valid; pr = carry_r; }
            // ---- energy peak-then-halve events of this block
            uint64_t ev;
            if (walk) {
                const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(b == 0 ? evq0 : evq2), n), hi = (uint32_t)__builtin_amdgcn_readlane((int)(b == 0 ? evq1 : evq3), n);
                ev = ((uint64_t)hi << 32) | lo;
            } else {
                const float Ep = __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, Ef), 0x138, 0xf, 0xf, false));
                ev = energy_events_block(vm, Ef, Ep, carry_valid != 0, evL, lane);
            }
            nA += __popcll(ev);
            const bool my_event = ((ev >> lane) & 1ull) != 0ull;
            if (my_event) myev |= 1u << (b & 31);
            carry_valid = (int)(vm >> 63); carry_r = __builtin_bit_cast(float, read_lane_i32(__builtin_bit_cast(int, rf), 63));
            bool kpos = false, run0 = false, evpos = false;
            if (valid) {
                const double r = rf, E = Ef, wd = wf, dB = 20 * jsm::log10_fin(E);      // (valid: an fp32 energy above zero — positive, finite, normal as a double)
                if (b == 0) dB_first = dB;
                sc += r * dB; swi += (uint32_t)rf; sM += wd * dB; sT += E; sK += dB;
                kpos = dB > 0;
                if (kpos) sKpos += dB;
                if (pv) { const int dl = (int)rf - (int)pr; if (dl > 1) udi += (uint32_t)dl; else if (dl < -1) udi += (uint32_t)(-dl) << 16; }
                else run0 = true;
                evpos = my_event && kpos;
                if (evpos) sa += dB;
            }
            cnt += __popcll(vm); runs += __popcll(__ballot(run0)); nKpos += __popcll(__ballot(kpos)); na += __popcll(__ballot(evpos));
        }
        // the two integer sums ride along with the five f64 sums through the LDS transposition (integers far below 2^53: exact in any order); the wave's
        // upward jumps stay below 254 x 2048 < 2^20, so the lanes' two 16-bit fields are spread to up + dn x 2^20 before they are added
        double sw, up, dn;
        {
            double r7[7] = {sc, sM, sT, sK, sKpos, (double)swi, (double)(udi & 0xffffu) + (double)(udi >> 16) * 1048576.0};
            wave_sums_f64_lds(r7, red, lane);
            sc = r7[0]; sM = r7[1]; sT = r7[2]; sK = r7[3]; sKpos = r7[4]; sw = r7[5];
            const unsigned long long ud = (unsigned long long)r7[6];
            up = (double)(uint32_t)(ud & 0xfffffull); dn = (double)(uint32_t)(ud >> 20);
        }
        const double m = cnt, nruns = runs, nkp = nKpos;
        // lane q < 16 collects result q of this column (one coalesced store at the end).  The column's nine quotients and three square
        // roots are not evaluated one after the other by the whole wave: lane q takes the operands of ITS result, and one division,
        // one dependent division (the two-step results 4, 5, 14) and one square root serve all of them — each value is the same
        // IEEE operation on the same operands as before.
        double ma = 0, vw = 0, vk = 0, va = 0;
        double mk = 0;
        if (nruns > 0) {
            const double mw = sw / m;
            mk = sKpos / nkp;
            if (nA > 0) { sa = wave_sum_f64(sa); ma = sa / (double)na; }
#pragma unroll 1
            for (int base = 0, b = 0; base < a; base += 64, b++) {
                const int t = base + lane;
                if (t < a) {
                    const float rf = fr[9 * t + 3 * n], Ef = fr[9 * t + 3 * n + 1];
                    if (rf > 0.f && Ef > 0.f) {
                        double dB = dB_first;
                        if (b != 0) dB = 20 * jsm::log10_fin((double)Ef);
                        const double d1 = (double)rf - mw, d2 = dB - mk;
                        vw += d1 * d1; vk += d2 * d2;
                        if ((myev >> (b & 31)) & 1u) { const double d3 = dB - ma; va += d3 * d3; }
                    }
                }
            }
            { double r3[3] = {vw, vk, va}; wave_sums_f64_lds(r3, red, lane); vw = r3[0]; vk = r3[1]; va = r3[2]; }      // (va = 0 without events)
        }
        {
            // the column's operands wait in LDS for the common evaluation below
            if (lane == 0) {
                double* f = fx + n * FEAT_FX;
                f[0] = sc; f[1] = sK; f[2] = vw; f[3] = m; f[4] = vk; f[5] = sT; f[6] = sM; f[7] = ma; f[8] = va; f[9] = (double)nA; f[10] = nruns; f[11] = up; f[12] = dn; f[13] = mk;
                f[14] = (double)a; f[15] = 0.0; f[16] = 1.0;
            }
        }
    }
    {
        wsync();
        const int n = lane >> 4, q = lane & 15;
        if (n < 3) {
            const double* f = fx + n * FEAT_FX;
            // numerator / denominator slot of result q (15: zero, 16: one)
            const int ni = (q == 0 ? 0 : q == 1 ? 2 : q == 3 ? 4 : (q == 4 || q == 5) ? 5 : q == 6 ? 6 : q == 13 ? 8 : q == 14 ? 1 : q == 15 ? 3 : 15);
            const int di = q == 0 ? 1 : (q == 1 || q == 3 || q == 5 || q == 14) ? 3 : (q == 4 || q == 15) ? 14 : q == 6 ? 1 : q == 13 ? 9 : 16;
            const double nruns = f[10], nA = f[9], m = f[3], ma = f[7], mk = f[13];
            const bool on = nruns > 0, ev_on = on && nA > 0;
            double num = f[ni], den = f[di];
            if (q == 15) num = 100 * num;                                                    // 100 m / a
            if ((!on && q != 15) || (!ev_on && (q == 13 || q == 14))) { num = 0; den = 1; }   // what the per-column form leaves at 0 / 1
            const double q1 = num / den;
            double num2 = 0, den2 = 1;
            if (q == 4 || q == 5) { num2 = q1 * 100; den2 = ctx_max; }                        // sT / a * 100 / ctx_max, sT / m * 100 / ctx_max
            if (q == 14) { num2 = ma; den2 = q1; }                                            // ma / (sK / m)
            const double q2 = num2 / den2;
            const double sq = sqrt(q1);
            double mine = 0;
            if (q == 0 || q == 6) mine = on ? q1 : 0.0;
            if (q == 1 || q == 3) mine = on ? sq : 0.0;
            if (q == 2) mine = on ? mk : 0.0;
            if (q == 4 || q == 5) mine = on ? q2 : 0.0;
            if (q == 7) mine = m;
            if (q == 8) mine = nruns;
            if (q == 9) mine = f[11];
            if (q == 10) mine = f[12];
            if (q == 11) mine = on ? nA : 0.0;
            if (q == 12) mine = ev_on ? ma : 0.0;
            if (q == 13) mine = ev_on ? sq : 0.0;
            if (q == 14) mine = ev_on ? 100 * (q2 - 1) : 0.0;
            if (q == 15) mine = q1;
            x[5 + lane] = mine;
        }
        wsync();
    }
}

}  // namespace wsa
