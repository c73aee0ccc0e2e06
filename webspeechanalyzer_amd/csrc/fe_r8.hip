// fe_r8.hip — K1, the 1024-point family (16 kHz at the default settings): fe_kernel_r8 and the choice of its instantiation.
//
// Mapping: ONE WAVEFRONT PER FRAME, everything in registers except two LDS transposes.
//   N2 = 512 packed complex points = 64 lanes x 8 points.  DIF radices [8, 8, 8]:
//   pass 1  lane m holds z[64a + m], a = 0..7           (only a < AZ are non-zero: window <= 128 AZ samples)
//   X1      LDS transpose: lane (a', c) gets b = 0..7 of sub-FFT a'      (row stride 72: conflict-free)
//   pass 2  radix 8 over b, twiddle W_64^{c b'}
//   X2      LDS transpose inside 8-lane groups: lane (a', b') gets c = 0..7  (row stride 9)
//   pass 3  radix 8 over c  ->  lane holds Z[k0 + 64 c'], k0 = a' + 8 b'
//   split   real-FFT recombination with the partner lane (k0 <-> 64 - k0) through ds_bpermute
//   mel     4|X|^2 to LDS, each lane sums its bands (fmaf chain, ascending bin), u32 store (coalesced)
// Twiddles, the window and the split factors are loop-invariant per lane and live in VGPRs for all
// frames a wave processes.  PCM is read exactly once with 512-byte-per-instruction coalesced loads.
#include "fe_stages.hpp"
#include <algorithm>

namespace wsa {

// where power bin k of the 1024-point kernel sits in its LDS row: the split's lanes hold k0 = (lane >> 3) + 8 (lane & 7), so lanes l and l + 4 of a half-wave
// would store to the same bank (k0 mod 32); swapping bit 2 where bit 5 is set spreads the 32 lanes of a half-wave over the 32 banks.  The readers' tap
// addresses are loop-invariant registers either way.
struct FePsw { __device__ __forceinline__ int operator()(int k) const { return k ^ ((k >> 3) & 4); } };

// NR = rows of 64 bins the split produces (kmax / 64 + 1 <= NR), MW = mel taps per band kept in registers (wider bands take the LDS loop),
// T1L = inter-pass twiddles W_512^{m a'} read from LDS instead of 14 registers: <4, 5, 8, true> is the BASELINE geometry (16 kHz, 128 mel bands
// up to 4 kHz) at 4 waves per SIMD
// MWL = taps kept for the lane's LOWER band (bands 0..63 of a mel bank are the narrow ones: 4 taps at the baseline geometry, 8 for the upper half)
// AF = leading 64-point blocks of packed input that lie inside the window for every lane (win >= 128 AF): their samples need no select
// (the lean instantiations are held to 128 VGPRs = 4 waves per SIMD: what does not fit are three addresses of the general split path, which the
//  baseline geometry never runs)
template <int AZ, int NR, int MW, bool T1L, int MWL = MW, int AF = 0>
__global__ __launch_bounds__(256, (T1L && MWL == 4) ? 4 : 1) void fe_kernel_r8(FeParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    // (the wave number through v_readfirstlane: the compiler then knows the frame counter, the frame's addresses and the loop tests are uniform — scalar code)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    __shared__ uint32_t s_next[2];
    const FePsw psw;
    const FeTables T = fe_tables(smem, p);
    const FeLdsR8 L = fe_lds_r8(p.mel_total, p.bands);
    // (power rows: whole rows of 64 bins — the split stores every lane's row entry, no test against kmax)
    v2f* X = reinterpret_cast<v2f*>(smem + L.wave0) + (size_t)wave * XBUF;
    // the power rows share the wave's exchange buffer: they are written behind the last read of the second transpose and read before the next frame's first store
    // (5 KB less per workgroup: beside two of them a CU then holds five 20 KB peak-scan waves of the other batches instead of four)
    float* P = reinterpret_cast<float*>(X);
    static_assert(XBUF * 8 >= 64 * 9 * 4, "the power rows fit the exchange buffer");
    v2f* s_tw1 = reinterpret_cast<v2f*>(smem + L.tw1);                                                                          // [7][64]
    if (T1L) fe_fill_twiddle_rows(s_tw1, p.tw_n2, 7);
    // BASE: the baseline geometry's own instantiation (AF == 3: 16 kHz, 400-sample window, 128 mel bands up to 4 kHz).  fe_select_r8 picks it only when
    // the split has exactly five rows, all 128 bands exist and every band's taps fit the registers, so the loop-invariant tests of the frame loop
    // (rows, mel_fast, all_bands: a scalar compare + branch each, ~20 instructions per frame) are compile-time constants there
    constexpr bool BASE = AF == 3 && NR == 5 && T1L;
    // (the baseline geometry's pipelined loop keeps the power taps of the frame before in registers across the head of the next frame: the split's five twiddles
    //  W_1024^k of the lane make room — read from this table beside the partner values, same round trip)
    v2f* s_tws = reinterpret_cast<v2f*>(smem + L.tws);                                                                          // [5][64]
    if (BASE) for (int i = threadIdx.x; i < 5 * 64; i += 256) { const int l = i & 63, k = (l >> 3) + 8 * (l & 7) + 64 * (i >> 6); s_tws[i] = to_v2f(k <= p.kmax ? p.tw_nfft[k] : make_float2(0.f, 0.f)); }
    const int zslot = (int)(reinterpret_cast<float*>(smem + L.zero) - P);                                                      // the zero word, as an index into this wave's power rows
    if (threadIdx.x == 0) *reinterpret_cast<float*>(smem + L.zero) = 0.f;
    fe_tables_fill(T, p);
    // without a queue chunk = blockIdx.x; the barrier also stands between the tables' fill and their first read
    uint32_t nxt = 0; int phase = 0;
    fe_queue_ask_first(p, s_next);
    __syncthreads();
    uint32_t chunk = fe_queue_first(p, s_next, blockIdx.x);

    // ---- loop-invariant per-lane constants (registers)
    v2f tw1[8], tw2[8];
#pragma unroll
    for (int k = 1; k < 8; k++) if (!T1L) tw1[k] = to_v2f(p.tw_n2[lane * k]);
    fe_tail_twiddles(tw2, p, lane);
    v2f wn[AZ];
#pragma unroll
    for (int a = 0; a < AZ; a++) wn[a] = fe_window_pair(p, 2 * (64 * a + lane));
    const v2f ss = fe_both(FE_SQRT_HALF);
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const int k0 = hi3 + 8 * lo3;                         // this lane ends up holding Z[k0 + 64 c']
    const int k0p = (64 - k0) & 63;
    const int partner = ((k0p & 7) << 3) | (k0p >> 3);    // lane holding Z[k0p + 64 c']
    const int nrow = BASE ? 5 : p.kmax / 64 + 1;          // rows c' with some k <= kmax (<= NR)
    v2f tws[NR];
#pragma unroll
    for (int c = 0; c < NR; c++) {
        const int k = k0 + 64 * c;
        tws[c] = to_v2f((k <= p.kmax) ? p.tw_nfft[k] : make_float2(0.f, 0.f));       // (dead in the BASE instantiation: its loop reads s_tws)
    }

    // mel taps of this lane's two bands (m = lane, lane + 64): loop invariant, zero padded.  A padded tap multiplies the zero word, not a power
    // bin (fe_mel_taps: 0 * P is not 0 when P overflowed to Inf), so the fixed-length chain equals the FE-1 chain whatever the power rows hold.
    float mw[2][MW]; int mk[2], mn[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int m = lane + 64 * q;
        mk[q] = 0; mn[q] = 0;
#pragma unroll
        for (int j = 0; j < MW; j++) mw[q][j] = 0.f;
        if (p.spec_type == 1 && m < p.bands) {
            mk[q] = T.k0[m]; mn[q] = T.cnt[m];
#pragma unroll
            for (int j = 0; j < MW; j++) if (j < mn[q]) mw[q][j] = T.melw[T.off[m] + j];
        }
    }
    const bool mel_fast = BASE || (p.spec_type == 1 && p.bands <= 128 && __all(mn[0] <= MWL && mn[1] <= MW));
    // emphasis factors of the lane's two bands: loop invariant (two registers instead of two LDS reads per frame)
    float emph_r[2];
#pragma unroll
    for (int q = 0; q < 2; q++) { const int m = lane + 64 * q; emph_r[q] = T.emph[m < p.bands ? m : 0]; }
    const bool all_bands = BASE || p.bands == 128;              // both of a lane's bands exist: the stores need no lane test

    // PCM of frame f+1 is requested before frame f is transformed
    uint32_t ld_idx[AZ]; FeWinPred<true> ld_w[AZ];
#pragma unroll
    for (int a = 0; a < AZ; a++) {
        const int n = 2 * (64 * a + lane);
        ld_idx[a] = fe_pair_offset(n, p.win);
        ld_w[a] = fe_win_pred<true>(n, p.win);
    }
    // the loaded pairs stay untouched until the next iteration consumes them (anything computed from them here
    // would make the loop wait for the loads at once and lose the prefetch)
    for (; chunk < p.n_chunks;) {
    const FeChunk ck = fe_chunk(p, chunk, p.chunks_per_clip, wave);
    const uint32_t f_begin = ck.f_begin, f_end = ck.f_end;
    const __amdgpu_buffer_rsrc_t r_in = fe_buffer(ck.pcm + (uint64_t)f_begin * (uint32_t)p.hop);
    const __amdgpu_buffer_rsrc_t r_out = fe_buffer(ck.out + (uint64_t)f_begin * (uint32_t)p.bands);
    if (f_begin < f_end) {
    v2f xin[AZ];
    fe_load_pairs<AZ>(r_in, ld_idx, 0u, xin);
    fe_queue_ask(p, nxt);

    v2f v[8]; float pv[2][MW];
    // ---- the pieces of a frame, the same for the pipelined and the plain loop
    // window (F1-F3), the next frame's samples requested, pass 1: radix 8 over a, twiddle W_512^{m a'}
    auto head = [&](uint32_t f) __attribute__((always_inline)) {
#pragma unroll
        for (int a = 0; a < 8; a++) { v[a].x = 0.f; v[a].y = 0.f; }
#pragma unroll
        for (int a = 0; a < AZ; a++) v[a] = pk_mul(a >= AF ? fe_win_select(xin[a], ld_w[a]) : xin[a], wn[a]);
        fe_load_pairs<AZ>(r_in, ld_idx, (min(f + 1, f_end - 1) - f_begin) * (uint32_t)p.hop * 4u, xin);          // (the last frame is requested twice: no branch)
        if (T1L) {
#pragma unroll
            for (int k = 1; k < 8; k++) tw1[k] = s_tw1[(k - 1) * 64 + lane];
        }
        radix8_pk<AZ>(v, ss);
        pk_cmul7(v, tw1);
    };
    // partner value Z[512 - k] of row c: general lanes: partner lane's register 7 - c; the k0 == 0 lane pairs with itself: register (8 - c) & 7
    auto partner_value = [&](int c) __attribute__((always_inline)) {
        v2f zb;
        if (c < 8) zb = fe_shfl(v[7 - c], partner); else { zb.x = 0.f; zb.y = 0.f; }
        if (k0 == 0) zb = v[(8 - c) & 7];
        return zb;
    };
    // real-FFT split + 4x power (F4) of the baseline geometry's five rows in one block (pk_split5): partner values first, then the five chains interleaved
    auto split5 = [&](auto tw_of) __attribute__((always_inline)) {
        v2f za[5], zb[5], tw5[5]; float pw[5];
#pragma unroll
        for (int c = 0; c < 5; c++) { zb[c] = partner_value(c); za[c] = v[c]; tw5[c] = tw_of(c); }
        pk_split5(za, zb, tw5, pw);
#pragma unroll
        for (int c = 0; c < 5; c++) P[psw(k0) + 64 * c] = pw[c];          // (psw only looks at bits 2 and 5)
    };
    // the power values of BOTH bands are requested before the first multiply-add: one LDS round trip per frame for the taps instead of one per band
    // (the two bands' chains are independent)
    auto request_taps = [&]() __attribute__((always_inline)) {
#pragma unroll
        for (int q = 0; q < 2; q++) fe_mel_taps<MW>(pv[q], P, mk[q], mn[q], q == 1 ? MW : MWL, zslot, psw);
        wave_lds_sync();
    };
    auto band_value = [&](int q) __attribute__((always_inline)) { return fe_mel_chain<MW>(mw[q], pv[q], q == 1 ? MW : MWL, emph_r[q], p.gain); };
    auto store_band = [&](uint32_t f, int m, float e) __attribute__((always_inline)) {
        __builtin_amdgcn_raw_buffer_store_b32(to_u32(e), r_out, (uint32_t)m * 4u, (f - f_begin) * (uint32_t)p.bands * 4u, 0);
    };

    if constexpr (BASE) {
        // ---- the baseline geometry's loop, software-pipelined by one stage.  A wave issues nothing while it waits for an LDS read, and a frame has five such
        //      round trips one after the other (two transposes, the split's partner values, the power taps, the twiddles); here the END of frame f — power taps
        //      -> mel sums -> store — is taken apart: its reads are requested right behind the power rows' stores, then the HEAD of frame f + 1 (window, first
        //      radix-8 pass, twiddles) runs while they are on their way, the first transpose of f + 1 is issued, and only then the mel sums of f are formed —
        //      while that transpose is on ITS way.  Two of the round trips are covered by the other frame's arithmetic.  The power rows share the exchange buffer
        //      (P aliases X): the taps of f are READ before the transpose of f + 1 is WRITTEN, and a wave's LDS instructions execute in order.  Same operations
        //      on the same operands as the plain loop below: bit-identical frames.  The first transpose is the one in registers.
        auto tail = [&](uint32_t fp, int q) __attribute__((always_inline)) { store_band(fp, lane + 64 * q, band_value(q)); };
        head(f_begin);
        for (uint32_t f = f_begin; f < f_end; f++) {
            fe_tail64<true, 8, true>(v, X, tw2, ss, lane,
                [&]() __attribute__((always_inline)) { if (f > f_begin) tail(f - 1, 1); },     // the upper band's mel sum and store of the frame before, behind this frame's first transpose
                [&]() __attribute__((always_inline)) { if (f > f_begin) tail(f - 1, 0); });    // ... the lower band's behind the second
            split5([&](int c) __attribute__((always_inline)) { return s_tws[c * 64 + lane]; });
            wave_lds_sync();
            // the power taps of frame f are requested ...
            request_taps();
            // ... and the head of frame f + 1 runs while they arrive (behind the last frame: the same frame's samples once more, nobody looks at the result)
            head(f + 1);
        }
        tail(f_end - 1, 1); tail(f_end - 1, 0);
    } else
    for (uint32_t f = f_begin; f < f_end; f++) {
        head(f);
        fe_tail64<false, 8, true>(v, X, tw2, ss, lane);               // -> v[c'] = Z[k0 + 64 c']
        // ---- real-FFT split + 4x power (F4): X[k] from Z[k] and conj(Z[512 - k])
        if (NR == 5 && nrow == 5) split5([&](int c) __attribute__((always_inline)) { return tws[c < NR ? c : 0]; });
        else
#pragma unroll
        for (int c = 0; c < NR; c++) {
            // (c == 8 only for k0 == 0: Z[512] = Z[0]; bins above kmax land in the row's padding: nobody reads them)
            if (c < nrow) P[psw(k0 + 64 * c)] = pk_split1(v[c & 7], partner_value(c), tws[c]);
        }
        wave_lds_sync();
        // ---- bands (F5-F8)
        if (mel_fast) {
            request_taps();
            float e2[2];
#pragma unroll
            for (int q = 0; q < 2; q++) e2[q] = band_value(q);
#pragma unroll
            for (int q = 0; q < 2; q++) {
                const int m = lane + 64 * q;
                if (all_bands) store_band(f, m, e2[q]); else if (m < p.bands) store_band(f, m, e2[q]);
            }
        } else fe_bands_general(p, T, P, lane, psw, [&](int m, float e) __attribute__((always_inline)) { store_band(f, m, e); });
        wave_lds_sync();
    }
    } else fe_queue_ask(p, nxt);
    if (!p.queue) break;
    chunk = fe_queue_next(s_next, phase, nxt);
    }
}

// The lean instantiations (4 waves per SIMD) serve what they can hold: <= 5 rows of bins, <= 8 taps per band (launch argument mel_max_taps).
// (the general kernel fe_kernel_rx instantiated at R = 8 keeps its invariants in LDS, needs 114 VGPRs = 4 waves per SIMD and
// is slower than this register-resident one: 0.368 vs 0.345 ms — the kernel is VALU + LDS throughput bound)
FeChoice fe_select_r8(const FeParams& p) {
    FeChoice c;
    c.lds = fe_lds_r8(p.mel_total, p.bands).total;
    // co-residency experiments (Tuning::fe_wg_per_cu): dynamic LDS padded so that k workgroups fit a CU's 160 KB and k + 1 do not
    // (negative values: the cap by padding; positive ones cap the persistent launch's grid, which leaves the LDS to the other kernels)
    if (p.wg_per_cu <= -1 && p.wg_per_cu >= -3) c.lds = std::max(c.lds, ((size_t)163840 / (size_t)(-p.wg_per_cu + 1) + 256) & ~(size_t)255);
    // chunks through a queue when the caller provides one (persistent launch), else one per workgroup.  Default TWO workgroups per CU
    // (8 of a CU's 16 wave slots at this kernel's 128 VGPRs, 68 of its 160 KB of LDS): alone the kernel then runs 0.35 instead of 0.27 ms, but a caller that
    // keeps several batches in flight gets the peak scan / gate / tracker of the other batches onto the same CUs beside it — the front end is bound by the
    // LDS pipe, they by instruction issue — and the pipelined step of the 1024-clip batch went from 0.67 to 0.60 ms (profiles/r04_notes.md); 4 restores the old occupancy
    c.queue_wgs = 4;
    const int az = (p.win + 127) / 128;       // non-zero 64-point blocks of packed input
    const bool lean = p.kmax / 64 + 1 <= 5 && p.mel_max_taps <= 8 && p.spec_type == 1 && !p.fat;
    if (az <= 2) { c.kernel = fe_kernel_r8<2, 9, MELW, false>; c.name = "fe_kernel_r8<2,9,12,false>"; }
    else if (az <= 4 && lean && p.mel_max_taps_lo <= 4 && p.win >= 384 && p.bands == 128 && p.kmax / 64 + 1 == 5)
        { c.kernel = fe_kernel_r8<4, 5, 8, true, 4, 3>; c.name = "fe_kernel_r8<4,5,8,true,4,3>"; }      // the baseline geometry (16 kHz: 400-sample window, 128 bands, five rows of bins): BASE
    else if (az <= 4 && lean && p.mel_max_taps_lo <= 4) { c.kernel = fe_kernel_r8<4, 5, 8, true, 4>; c.name = "fe_kernel_r8<4,5,8,true,4>"; }
    else if (az <= 4 && lean) { c.kernel = fe_kernel_r8<4, 5, 8, true>; c.name = "fe_kernel_r8<4,5,8,true>"; }
    else if (az <= 4) { c.kernel = fe_kernel_r8<4, 9, MELW, false>; c.name = "fe_kernel_r8<4,9,12,false>"; }
    else { c.kernel = fe_kernel_r8<8, 9, MELW, false>; c.name = "fe_kernel_r8<8,9,12,false>"; }
    return c;
}

}  // namespace wsa
