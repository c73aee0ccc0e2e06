// fe_rx.hip — K1, the general power-of-two family: fe_kernel_rx and the choice of its instantiation.
//
// General FFT length: N2 = 64 R packed complex points, R in {2, 4, 16, 32, 64} (NFFT 256 / 512 / 2048 / 4096 / 8192:
// 4 kHz .. 64 kHz audio at the default band settings).  Same mapping as the 1024-point kernel (fe_r8.hip), wave per frame:
//   pass 1  lane m holds z[64a + m], a < R (a < AZ non-zero); radix-R butterfly in registers (log2 R
//           radix-2 stages, FE-1 twiddle forms, pruned where an input is a structural zero), then the
//           inter-pass twiddle W_N2^{m a'} from a per-lane table in LDS ([a' - 1][lane]: conflict free)
//   then the R sub-FFTs of 64 points, eight at a time (group g = sub-FFTs 8g .. 8g + 7), each group
//   exactly the [8, 8] tail of the 1024-point kernel (X1, pass 2, X2, pass 3):
//           lane (al, b') ends up holding Z[(8g + al) + R b' + 8R c'], c' = 0..7, in z[8g + c'].
//   split   partner values by the rule at fe_partners (fe_stages.hpp).  Split twiddles W_NFFT^k come from LDS.
// For R < 8 only the lanes with al < R carry sub-FFTs.
#include "fe_stages.hpp"

namespace wsa {

template <int R, int AZ, int MW>
__global__ __launch_bounds__(256) void fe_kernel_rx(FeParams p) {
    constexpr int NG = (R + 7) / 8;            // groups of eight 64-point sub-FFTs
    constexpr int AL = R < 8 ? R : 8;          // sub-FFTs in a group
    constexpr int N2 = 64 * R;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));      // (uniform: scalar frame counter and addresses)
    const FeLds L = fe_lds(p.mel_total, p.bands, p.kmax, 0, R - 1, AZ, MW);
    const FeTables T = fe_tables(smem, p);
    v2f* s_twl = reinterpret_cast<v2f*>(smem + L.twl);
    v2f* s_tws = reinterpret_cast<v2f*>(smem + L.tws);
    v2f* s_wn = reinterpret_cast<v2f*>(smem + L.wn);
    float* s_mwp = reinterpret_cast<float*>(smem + L.mwp);
    v2f* X = reinterpret_cast<v2f*>(smem + L.wave0 + (size_t)wave * L.xbytes);
    float* P = reinterpret_cast<float*>(smem + L.wave0 + 4 * L.xbytes + (size_t)wave * L.pbytes);

    const int zslot = (int)(reinterpret_cast<float*>(smem + L.zero) - P);      // the zero word a band's padded taps read, as an index into this wave's power rows
    if (threadIdx.x == 0) *reinterpret_cast<float*>(smem + L.zero) = 0.f;
    fe_tables_fill(T, p);
    fe_fill_twiddle_rows(s_twl, p.tw_n2, R - 1);
    for (int i = threadIdx.x; i <= p.kmax; i += 256) s_tws[i] = to_v2f(p.tw_nfft[i]);
    fe_fill_window<AZ>(s_wn, p);
    __syncthreads();
    const bool mel_fast = fe_fill_taps<MW>(s_mwp, T, p);

    const FeChunk ck = fe_chunk_of(p, blockIdx.y, blockIdx.x, wave);
    const uint32_t f_begin = ck.f_begin, f_end = ck.f_end;
    if (f_begin >= f_end) return;

    v2f tw2[8];
    fe_tail_twiddles(tw2, p, lane);
    const v2f ss = fe_both(FE_SQRT_HALF);
    v2f one_mone; one_mone.x = 1.0f; one_mone.y = -1.0f;
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const bool act = hi3 < AL;                                   // lane carries a sub-FFT (always for R >= 8)
    const FePartners part = fe_partners(R, lane);
    int mk[2], mn[2];
    fe_mel_first_bin(mk, mn, p, T, lane);

    // branch-free prefetch: clamped 8-byte pairs, untouched until the next iteration
    int ld_idx[AZ]; FeWinPred<false> ld_w[AZ];
#pragma unroll
    for (int a = 0; a < AZ; a++) {
        const int n = 2 * (64 * a + lane);
        ld_idx[a] = fe_pair_index(n, p.win);
        ld_w[a] = fe_win_pred<false>(n, p.win);
    }
    v2f xin[AZ];
    fe_load_pairs<AZ>(ck.pcm + (uint64_t)f_begin * (uint32_t)p.hop, ld_idx, xin);

    for (uint32_t f = f_begin; f < f_end; f++) {
        v2f v[R];
#pragma unroll
        for (int a = 0; a < R; a++) { v[a].x = 0.f; v[a].y = 0.f; }
#pragma unroll
        for (int a = 0; a < AZ; a++) v[a] = pk_mul(fe_win_select(xin[a], ld_w[a]), s_wn[a * 64 + lane]);
        if (f + 1 < f_end) fe_load_pairs<AZ>(ck.pcm + (uint64_t)(f + 1) * (uint32_t)p.hop, ld_idx, xin);
        // ---- pass 1: radix R over a, twiddle W_N2^{m a'}
        radix_r<R, AZ>(v, p.tw_64, ss, one_mone);
#pragma unroll
        for (int k = 1; k < R; k++) v[k] = pk_cmul(v[k], s_twl[(k - 1) * 64 + lane]);
        // ---- the R sub-FFTs of 64 points, eight at a time
        v2f z[NG * 8];
#pragma unroll
        for (int g = 0; g < NG; g++) {
            v2f u[8];
#pragma unroll
            for (int k = 0; k < AL; k++) u[k] = v[8 * g + k];
            fe_tail64<false, AL, false>(u, X, tw2, ss, lane);
#pragma unroll
            for (int c = 0; c < 8; c++) z[8 * g + c] = u[c];
        }
        // ---- real-FFT split + 4x power: X[k] from Z[k] and conj(Z[N2 - k])
#pragma unroll
        for (int g = 0; g < NG; g++) {
#pragma unroll
            for (int c = 0; c < 8; c++) {
                if (8 * g + 8 * R * c <= p.kmax) {                       // smallest k of this row (uniform)
                    const v2f zb = fe_partner_value<NG>(z, g, c, lane, part);
                    const int k = 8 * g + hi3 + R * lo3 + 8 * R * c;
                    const float pw = pk_split1(z[8 * g + c], zb, s_tws[k <= p.kmax ? k : 0]);
                    if (act && k <= p.kmax) P[k] = pw;
                }
            }
        }
        if (p.kmax == N2 && lane == 0) P[N2] = pk_split1(z[0], z[0], s_tws[N2]);      // X[N2] from Z[0] alone
        wave_lds_sync();
        // ---- bands (F5-F8)
        uint32_t* out = ck.out + (uint64_t)f * (uint32_t)p.bands;
        auto store_band = [&](int m, float e) __attribute__((always_inline)) { out[m] = to_u32(e); };
        if (mel_fast) fe_bands_two<MW>(p, T, s_mwp, P, mk, mn, zslot, lane, store_band);
        else fe_bands_general(p, T, P, lane, FeIdentity(), store_band);
        wave_lds_sync();
    }
}

template <int R, int AZ, int MW>
static FeChoice choice_rx(const FeParams& p, const char* name) {
    // dynamic LDS up to the device limit (160 KB per workgroup on gfx950) needs no opt-in on ROCm; a configuration
    // that asks for more fails the launch and is reported through hipGetLastError by the caller
    FeChoice c;
    c.kernel = fe_kernel_rx<R, AZ, MW>; c.name = name;
    c.lds = fe_lds(p.mel_total, p.bands, p.kmax, 0, R - 1, AZ, MW).total;
    c.grid_2d = true;
    return c;
}

// the smallest instantiation whose non-zero blocks cover the window
FeChoice fe_select_rx(const FeParams& p, int R) {
    const int az = (p.win + 127) / 128;       // non-zero 64-point blocks of packed input
    if (R == 2) return choice_rx<2, 2, 12>(p, "fe_kernel_rx<2,2,12>");
    if (R == 4) return az <= 2 ? choice_rx<4, 2, 12>(p, "fe_kernel_rx<4,2,12>") : choice_rx<4, 4, 12>(p, "fe_kernel_rx<4,4,12>");
    if (R == 16) return az <= 5 ? choice_rx<16, 5, 14>(p, "fe_kernel_rx<16,5,14>") : az <= 8 ? choice_rx<16, 8, 14>(p, "fe_kernel_rx<16,8,14>") : choice_rx<16, 16, 14>(p, "fe_kernel_rx<16,16,14>");
    if (R == 32) return az <= 10 ? choice_rx<32, 10, 14>(p, "fe_kernel_rx<32,10,14>") : az <= 16 ? choice_rx<32, 16, 14>(p, "fe_kernel_rx<32,16,14>") : choice_rx<32, 32, 14>(p, "fe_kernel_rx<32,32,14>");
    if (R == 64) return choice_rx<64, 64, 14>(p, "fe_kernel_rx<64,64,14>");
    return FeChoice();
}

}  // namespace wsa
