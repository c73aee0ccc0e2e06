// fe_r3.hip — K1, the 3 * 2^k family: fe_kernel_r3 and the choice of its instantiation.
//
// NFFT = 3 * 2^k (FE-1 F2: 3072 points at 44.1 / 48 kHz, the rate of the reference's offline path, ref @B18765):
// N2 = 3 M packed complex points, M = 64 RM.  Same mapping as the other families, wave per frame:
//   stage 0  lane m holds z[64 a + m], a < 3 RM (a < AZ non-zero); a = j RM + aM, j = the third of the packed frame.
//            Radix-3 butterfly over j in registers (oracle/frontend.c radix3(): t = x1 + x2, y0 = x0 + t, m = fma(-1/2, t, x0),
//            s = fl32(sqrt(3)/2) (x1 - x2), y1 = m - i s, y2 = m + i s; thirds that are structural zeros are pruned), then the
//            twiddle W_N2^{(64 aM + m) k3} from a per-lane LDS table
//   then     for k3 = 0, 1, 2 the M-point transform exactly as in fe_kernel_rx<RM>: radix-RM pass, twiddle W_M^{m a'}, the RM
//            sub-FFTs of 64 points eight at a time through the [8, 8] tail; lane (al, b') ends up with
//            Z_k3[(8g + al) + RM b' + 8 RM c'] in z[k3][8g + c'], and bin k = 3 k' + k3 of the N2-point transform is Z_k3[k']
//   split    Z[N2 - k]: k3 = 0 pairs with itself (k' <-> M - k': the partner rule of fe_kernel_rx); k3 = 1 pairs with k3 = 2 at
//            k'' = M - 1 - k' = (RM - 1 - a') + RM (7 - b') + 8 RM (7 - c'): group NG - 1 - g, register 7 - c', lane (AL - 1 - al, 7 - b')
#include "fe_stages.hpp"

namespace wsa {

// CR = rows c of the output registers the power spectrum reaches into (3 (8 RM c) <= kmax): the instantiation for the usual band limit
// (f_max well below Nyquist) keeps only those and their split partners 7 - c alive after the last radix-8 stage
// AF > 0 (round 5; the 48 kHz instantiation — a 25 ms window at 44.1 kHz is 1102 samples, under the 9 x 128 this needs, and stays on the AF = 0 kernel): the first AF 64-point blocks of packed input lie inside the window for every lane, so only the blocks
// behind them select samples — branch-free, on lane masks in scalar registers (the bool form compiled to two nested exec-mask branches per block with the masks
// spilled to vector lanes, and to ONE LDS round trip per block for the window: ten serial round trips per frame) —, the window values live in registers, the
// samples and bands travel by buffer addressing (32-bit scalar frame offset + 32-bit lane offset), every output row the template keeps exists (no test
// against kmax per row; fe_select_r3 checks it) and the power rows are padded (no test per lane); with all eight sub-FFTs of a group present (AL == 8)
// the tail's first transpose is the one in registers
template <int RM, int AZ, int MW, int CR = 8, int AF = 0>
__global__ __launch_bounds__(256) void fe_kernel_r3(FeParams p) {
    constexpr bool LN = AF > 0;
    constexpr int NG = (RM + 7) / 8;           // groups of eight 64-point sub-FFTs per M-point transform
    constexpr int AL = RM < 8 ? RM : 8;        // sub-FFTs in a group
    constexpr int M = 64 * RM, N2 = 3 * M;
    constexpr int NZM = AZ < RM ? AZ : RM;     // leading non-zero inputs of every M-point transform
    constexpr int PAD_K = LN ? 3 * 8 * RM * CR + 2 : 0;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: scalar frame counter and addresses)
    __shared__ uint32_t s_next[2];
    const FeLds L = fe_lds(p.mel_total, p.bands, p.kmax, 2 * RM, RM > 1 ? RM - 1 : 1, AZ, MW, PAD_K);
    const FeTables T = fe_tables(smem, p);
    v2f* s_tw3 = reinterpret_cast<v2f*>(smem + L.tw3);
    v2f* s_twl = reinterpret_cast<v2f*>(smem + L.twl);
    v2f* s_tws = reinterpret_cast<v2f*>(smem + L.tws);
    v2f* s_wn = reinterpret_cast<v2f*>(smem + L.wn);
    float* s_mwp = reinterpret_cast<float*>(smem + L.mwp);
    v2f* X = reinterpret_cast<v2f*>(smem + L.wave0 + (size_t)wave * L.xbytes);
    float* P = reinterpret_cast<float*>(smem + L.wave0 + 4 * L.xbytes + (size_t)wave * L.pbytes);

    const int zslot = (int)(reinterpret_cast<float*>(smem + L.zero) - P);      // the zero word a band's padded taps read, as an index into this wave's power rows
    if (threadIdx.x == 0) *reinterpret_cast<float*>(smem + L.zero) = 0.f;
    fe_tables_fill(T, p);
    for (int i = threadIdx.x; i < 2 * RM * 64; i += 256) {
        const int ln = i & 63, aM = (i >> 6) % RM, k3 = (i >> 6) / RM + 1;
        s_tw3[i] = to_v2f(p.tw_n2[(64 * aM + ln) * k3]);
    }
    fe_fill_twiddle_rows(s_twl, p.tw_m, RM - 1);
    for (int i = threadIdx.x; i <= (LN ? PAD_K : p.kmax); i += 256) s_tws[i] = to_v2f(i <= p.kmax ? p.tw_nfft[i] : make_float2(0.f, 0.f));
    fe_fill_window<AZ>(s_wn, p);
    __syncthreads();
    const bool mel_fast = fe_fill_taps<MW>(s_mwp, T, p);

    v2f tw2[8];
    fe_tail_twiddles(tw2, p, lane);
    const v2f ss = fe_both(FE_SQRT_HALF), mhalf = fe_both(-0.5f), c3 = fe_both(0.86602540378443864676f);
    v2f one_mone; one_mone.x = 1.0f; one_mone.y = -1.0f;
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const bool act = hi3 < AL;
    // partner lanes of the real split (see the header): transform 0 as in fe_kernel_rx, transforms 1 <-> 2 mirrored
    const FePartners part = fe_partners(RM, lane);
    const int part_x = ((((AL - 1 - hi3) & 7) << 3) | (7 - lo3)) & 63;
    int mk[2], mn[2];
    fe_mel_first_bin(mk, mn, p, T, lane);

    int ld_idx[AZ]; uint32_t ld_off[AZ]; FeWinPred<LN> ld_w[AZ];          // LN: byte offsets and lane masks
#pragma unroll
    for (int a = 0; a < AZ; a++) {
        const int n = 2 * (64 * a + lane);
        ld_idx[a] = fe_pair_index(n, p.win); ld_off[a] = fe_pair_offset(n, p.win);
        ld_w[a] = fe_win_pred<LN>(n, p.win);
    }
    v2f wn_r[LN ? AZ : 1];
    if (LN) {
#pragma unroll
        for (int a = 0; a < AZ; a++) wn_r[LN ? a : 0] = s_wn[a * 64 + lane];
    }
    // chunk: blockIdx (x = chunk of the clip, y = clip), or — persistent launch — from the queue (the tables above are filled once per workgroup instead of
    // once per 100 frames)
    const uint32_t cpc = p.queue ? (uint32_t)p.chunks_per_clip : gridDim.x;
    uint32_t nxt = 0; int phase = 0;
    fe_queue_ask_first(p, s_next);
    if (p.queue) __syncthreads();
    uint32_t chunk = fe_queue_first(p, s_next, blockIdx.y * gridDim.x + blockIdx.x);
    for (; !p.queue || chunk < p.n_chunks;) {
    const FeChunk ck = fe_chunk(p, chunk, cpc, wave);
    const uint32_t f_begin = ck.f_begin, f_end = ck.f_end;
    if (f_begin < f_end) {
    const __amdgpu_buffer_rsrc_t r_in = fe_buffer(ck.pcm + (uint64_t)f_begin * (uint32_t)p.hop);
    const __amdgpu_buffer_rsrc_t r_out = fe_buffer(ck.out + (uint64_t)f_begin * (uint32_t)p.bands);
    auto load_pcm = [&](uint32_t f, v2f (&x)[AZ]) __attribute__((always_inline)) {
        if constexpr (LN) fe_load_pairs<AZ>(r_in, ld_off, (f - f_begin) * (uint32_t)p.hop * 4u, x);
        else fe_load_pairs<AZ>(ck.pcm + (uint64_t)f * (uint32_t)p.hop, ld_idx, x);
    };
    v2f xin[AZ];
    load_pcm(f_begin, xin);
    fe_queue_ask(p, nxt);

    for (uint32_t f = f_begin; f < f_end; f++) {
        // ---- window: the frame's samples become x·w in place (samples outside the window are zeros of the table)
#pragma unroll
        for (int a = 0; a < AZ; a++) xin[a] = pk_mul(a >= AF ? fe_win_select(xin[a], ld_w[a]) : xin[a], LN ? wn_r[LN ? a : 0] : s_wn[a * 64 + lane]);
        // ---- per output residue k3: the radix-3 stage over the thirds j of the packed frame (a = j RM + aM), recomputed from the windowed
        //      samples for each k3 — the three transforms' inputs are never alive together (48 registers less than holding w[3][RM];
        //      the price is t / d / m / s computed twice) —, then the M-point transform
        v2f z[3][NG * 8];
#pragma unroll
        for (int k3 = 0; k3 < 3; k3++) {
            v2f w[RM];
#pragma unroll
            for (int aM = 0; aM < RM; aM++) {
                v2f zero; zero.x = 0.f; zero.y = 0.f;
                if (aM >= AZ) { w[aM] = zero; continue; }                                       // all three thirds are structural zeros
                const v2f x0 = xin[aM];
                if (RM + aM >= AZ) { w[aM] = k3 == 0 ? x0 : pk_cmul(x0, s_tw3[((k3 - 1) * RM + aM) * 64 + lane]); continue; }      // x1 = x2 = 0: y0 = y1 = y2 = x0
                const v2f x1 = xin[RM + aM];
                v2f t, d;
                if (2 * RM + aM >= AZ) { t = x1; d = x1; }                                        // x2 = 0
                else { const v2f x2 = xin[2 * RM + aM]; t = pk_add(x1, x2); d = pk_sub(x1, x2); }
                if (k3 == 0) { w[aM] = pk_add(x0, t); continue; }
                const v2f m = pk_fma(mhalf, t, x0);
                const v2f sq = pk_mul(c3, d);
                const v2f y = k3 == 1 ? pk_add_mi(m, sq) : pk_sub_mi(m, sq);                      // m - i s, m + i s
                w[aM] = pk_cmul(y, s_tw3[((k3 - 1) * RM + aM) * 64 + lane]);
            }
            if (k3 == 2) { if (LN) load_pcm(min(f + 1, f_end - 1), xin); else if (f + 1 < f_end) load_pcm(f + 1, xin); }          // the windowed samples are dead: the next frame's take their registers
            if constexpr (RM > 1) {
                radix_r<RM, NZM>(w, p.tw_64, ss, one_mone);
#pragma unroll
                for (int k = 1; k < RM; k++) w[k] = pk_cmul(w[k], s_twl[(k - 1) * 64 + lane]);
            }
#pragma unroll
            for (int g = 0; g < NG; g++) {
                v2f u[8];
#pragma unroll
                for (int k = 0; k < AL; k++) u[k] = w[8 * g + k];
                fe_tail64<LN && AL == 8, AL, false>(u, X, tw2, ss, lane);
#pragma unroll
                for (int c = 0; c < 8; c++) z[k3][8 * g + c] = u[c];
            }
        }
        // ---- real-FFT split + 4x power: X[k] from Z[k] and conj(Z[N2 - k]), k = 3 k' + k3
#pragma unroll
        for (int k3 = 0; k3 < 3; k3++) {
#pragma unroll
            for (int g = 0; g < NG; g++) {
#pragma unroll
                for (int c = 0; c < CR; c++) {
                    if (LN || 3 * (8 * g + 8 * RM * c) + k3 <= p.kmax) {        // smallest k of this row (uniform; LN: every kept row exists)
                        const v2f zb = k3 == 0 ? fe_partner_value<NG>(z[0], g, c, lane, part) : fe_shfl(z[3 - k3][8 * (NG - 1 - g) + 7 - c], part_x);
                        const int k = 3 * (8 * g + hi3 + RM * lo3 + 8 * RM * c) + k3;
                        const float pw = pk_split1(z[k3][8 * g + c], zb, s_tws[(LN || k <= p.kmax) ? k : 0]);          // (LN: the table and the power rows are padded to the rows the template keeps)
                        if (act && (LN || k <= p.kmax)) P[k] = pw;
                    }
                }
            }
        }
        if (p.kmax == N2 && lane == 0) P[N2] = pk_split1(z[0][0], z[0][0], s_tws[N2]);      // X[N2] from Z[0] alone
        wave_lds_sync();
        // ---- bands (F5-F8)
        uint32_t* out = ck.out + (uint64_t)f * (uint32_t)p.bands;
        if (mel_fast) fe_bands_two<MW>(p, T, s_mwp, P, mk, mn, zslot, lane, [&](int m, float e) __attribute__((always_inline)) {
            if constexpr (LN) __builtin_amdgcn_raw_buffer_store_b32(to_u32(e), r_out, (uint32_t)m * 4u, (f - f_begin) * (uint32_t)p.bands * 4u, 0);
            else out[m] = to_u32(e);
        });
        else fe_bands_general(p, T, P, lane, FeIdentity(), [&](int m, float e) __attribute__((always_inline)) { out[m] = to_u32(e); });
        wave_lds_sync();
    }
    } else fe_queue_ask(p, nxt);
    if (!p.queue) break;
    chunk = fe_queue_next(s_next, phase, nxt);
    }
}

template <int RM, int AZ, int MW, int CR = 8, int AF = 0>
static FeChoice choice_r3(const FeParams& p, const char* name) {
    FeChoice c;
    c.kernel = fe_kernel_r3<RM, AZ, MW, CR, AF>; c.name = name;
    c.lds = fe_lds(p.mel_total, p.bands, p.kmax, 2 * RM, RM > 1 ? RM - 1 : 1, AZ, MW, AF > 0 ? 3 * 8 * RM * CR + 2 : 0).total;
    c.grid_2d = true;
    // persistent launch (batches) of the AF > 0 instantiation: n_cu x WSA_FE_WGS workgroups (default 2: the kernel's 162 VGPRs admit three) take the chunks
    // from the queue — the ~30 KB of tables are filled once per workgroup, and the other batches' back-end kernels find room beside it
    c.queue_wgs = AF > 0 ? 3 : 0;
    return c;
}

// NFFT = 3 * 64 RM * 2: the smallest instantiation whose non-zero blocks cover the window
FeChoice fe_select_r3(const FeParams& p, int RM) {
    const int az = (p.win + 127) / 128;       // non-zero 64-point blocks of packed input
    if (RM == 1) return az <= 2 ? choice_r3<1, 2, 12>(p, "fe_kernel_r3<1,2,12>") : choice_r3<1, 3, 12>(p, "fe_kernel_r3<1,3,12>");
    if (RM == 2) return az <= 3 ? choice_r3<2, 3, 12>(p, "fe_kernel_r3<2,3,12>") : choice_r3<2, 6, 12>(p, "fe_kernel_r3<2,6,12>");
    if (RM == 4) {
        if (az <= 5 && p.kmax < 3 * 8 * 4 * 3 && !p.fat) return choice_r3<4, 5, 14, 3>(p, "fe_kernel_r3<4,5,14,3>");          // 1536 points = 22.05 kHz: rows c = 0 .. 2
        return az <= 5 ? choice_r3<4, 5, 14>(p, "fe_kernel_r3<4,5,14>") : az <= 8 ? choice_r3<4, 8, 14>(p, "fe_kernel_r3<4,8,14>") : choice_r3<4, 12, 14>(p, "fe_kernel_r3<4,12,14>");
    }
    if (RM == 8) {
        // (3072 points = 44.1 / 48 kHz with the default 4 kHz band limit: bins <= 383 sit in rows c = 0, 1 of the output registers)
        // ... and, at the reference's own geometry (25 ms window at 48 kHz — the offline context's rate; 1102 samples at 44.1 kHz fall short —: at least nine blocks inside the window, both kept rows of every residue
        // exist), the instantiation with the window in registers, mask selects and buffer addressing (AF = 9)
        if (az <= 10 && p.kmax < 3 * 8 * 8 * 2 && p.kmax >= 3 * 8 * 8 + 2 && p.win >= 128 * 9 && !p.fat) return choice_r3<8, 10, 14, 2, 9>(p, "fe_kernel_r3<8,10,14,2,9>");
        if (az <= 10 && p.kmax < 3 * 8 * 8 * 2 && !p.fat) return choice_r3<8, 10, 14, 2>(p, "fe_kernel_r3<8,10,14,2>");
        return az <= 10 ? choice_r3<8, 10, 14>(p, "fe_kernel_r3<8,10,14>") : az <= 16 ? choice_r3<8, 16, 14>(p, "fe_kernel_r3<8,16,14>") : choice_r3<8, 24, 14>(p, "fe_kernel_r3<8,24,14>");
    }
    if (RM == 16) return az <= 20 ? choice_r3<16, 20, 14>(p, "fe_kernel_r3<16,20,14>") : az <= 32 ? choice_r3<16, 32, 14>(p, "fe_kernel_r3<16,32,14>") : choice_r3<16, 48, 14>(p, "fe_kernel_r3<16,48,14>");
    if (RM == 32) return choice_r3<32, 96, 14>(p, "fe_kernel_r3<32,96,14>");
    return FeChoice();
}

}  // namespace wsa
