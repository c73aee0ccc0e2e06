// fe_stages.hpp — the stages the three front-end kernel families (fe_r8.hip, fe_rx.hip, fe_r3.hip) have in common, each written once:
// LDS tables and their layout (host and device), window predicates and sample loads, the 64-point [8, 8] tail, the real split's
// partner rules, the band forms, the chunk queue of the persistent launch — and, for frontend.hip, each family's selection function.
// Arithmetic = specification FE-1, bit-exact with oracle/frontend.c: the operations themselves are in fe_common.hpp.
#pragma once
#include "fe_common.hpp"
#include <type_traits>

namespace wsa {

// =====================================================================================================
// LDS layout, one description for the kernels and the host.  Every family's dynamic LDS starts with the shared tables
// [mel_w | mel_k0 | mel_cnt | mel_off | emph].
__host__ __device__ inline size_t fe_tables_bytes(int mel_total, int bands) {
    const size_t shared_words = (size_t)((mel_total + 3) & ~3) + 4 * (size_t)bands;
    return ((shared_words + 3) & ~(size_t)3) * 4;
}
// the 1024-point family: the waves' exchange buffers (the power rows live in them), then the W_512 table of the <.., true> variants [7][64] and the
// split twiddles of the baseline instantiation [5][64], and the word of 0.0f that a band's padded taps read (fe_mel_taps)
struct FeLdsR8 { size_t wave0, tw1, tws, zero, total; };
__host__ __device__ inline FeLdsR8 fe_lds_r8(int mel_total, int bands) {
    FeLdsR8 L;
    L.wave0 = fe_tables_bytes(mel_total, bands);
    L.tw1 = L.wave0 + (size_t)4 * XBUF * 8;
    L.tws = L.tw1 + (size_t)7 * 64 * 8;
    L.zero = L.tws + (size_t)5 * 64 * 8;
    L.total = L.zero + 16;
    return L;
}
// the general families: loop invariants that do not fit the register file next to 2 R data registers live in LDS, one
// conflict-free [..][lane] row per use.  tw3_rows: W_N2^{(64 aM + lane) k3}, [k3 - 1][aM][lane] v2f (NFFT = 3 * 2^k only);
// twl_rows: the inter-pass twiddles W^{lane k}, [k - 1][lane] v2f; pad_k: split twiddles and power rows reach at least this bin
// (the AF > 0 instantiation: up to the last bin of the rows it keeps); zero: the word of 0.0f that a band's padded taps read (fe_mel_taps)
struct FeLds { size_t tw3, twl, tws, wn, mwp, wave0, xbytes, pbytes, zero, total; };
__host__ __device__ inline FeLds fe_lds(int mel_total, int bands, int kmax, int tw3_rows, int twl_rows, int AZ, int MW, int pad_k = 0) {
    if (pad_k > kmax) kmax = pad_k;
    FeLds L;
    L.tw3 = fe_tables_bytes(mel_total, bands);
    L.twl = L.tw3 + (size_t)tw3_rows * 64 * 8;
    L.tws = L.twl + (size_t)twl_rows * 64 * 8;
    L.wn = L.tws + (size_t)((kmax + 2) & ~1) * 8;                 // window pairs [AZ][64] v2f
    L.mwp = L.wn + (size_t)AZ * 64 * 8;                           // mel taps of the lane's two bands, zero padded: [2][MW][64] f32
    L.wave0 = L.mwp + (size_t)2 * MW * 64 * 4;
    L.xbytes = (size_t)XBUF * 8;
    L.pbytes = (size_t)((kmax + 1 + 3) & ~3) * 4;
    L.zero = L.wave0 + 4 * (L.xbytes + L.pbytes);
    L.total = L.zero + 16;
    return L;
}

struct FeTables { float* melw; int* k0; int* cnt; int* off; float* emph; };
__device__ __forceinline__ FeTables fe_tables(char* smem, const FeParams& p) {
    FeTables T;
    T.melw = reinterpret_cast<float*>(smem);
    T.k0 = reinterpret_cast<int*>(T.melw + ((p.mel_total + 3) & ~3));
    T.cnt = T.k0 + p.bands;
    T.off = T.cnt + p.bands;
    T.emph = reinterpret_cast<float*>(T.off + p.bands);
    return T;
}
// (all 256 threads; the caller's barrier stands between this and the first read)
__device__ __forceinline__ void fe_tables_fill(const FeTables& T, const FeParams& p) {
    for (int i = threadIdx.x; i < p.mel_total; i += 256) T.melw[i] = p.mel_w[i];
    for (int i = threadIdx.x; i < p.bands; i += 256) {
        T.emph[i] = p.emph[i];
        if (p.spec_type == 1) { T.k0[i] = p.mel_k0[i]; T.cnt[i] = p.mel_cnt[i]; T.off[i] = p.mel_off[i]; }
    }
}
// inter-pass twiddles W^{lane k}, k = 1 .. rows: [k - 1][lane]
__device__ __forceinline__ void fe_fill_twiddle_rows(v2f* s_tw, const float2* __restrict__ tw, int rows) {
    for (int i = threadIdx.x; i < rows * 64; i += 256) s_tw[i] = to_v2f(tw[(i & 63) * ((i >> 6) + 1)]);
}
// window values of the packed pair n, n + 1 (F1: zero behind the window)
__device__ __forceinline__ v2f fe_window_pair(const FeParams& p, int n) {
    v2f w; w.x = n < p.win ? p.window[n] : 0.0f; w.y = n + 1 < p.win ? p.window[n + 1] : 0.0f;
    return w;
}
template <int AZ>
__device__ __forceinline__ void fe_fill_window(v2f* s_wn, const FeParams& p) {
    for (int i = threadIdx.x; i < AZ * 64; i += 256) s_wn[i] = fe_window_pair(p, 2 * (64 * (i >> 6) + (i & 63)));
}
// [q][j][lane]: tap j of band lane + 64 q, zero padded (a padded tap multiplies the zero word, not a power bin: fe_mel_taps).  Reads the shared
// tables: behind their barrier.  Returns mel_fast: every band's taps fit and each lane has at most two bands.
template <int MW>
__device__ __forceinline__ bool fe_fill_taps(float* s_mwp, const FeTables& T, const FeParams& p) {
    bool taps_fit = true;
    for (int i = threadIdx.x; i < 2 * MW * 64; i += 256) {
        const int ln = i & 63, j = (i >> 6) % MW, q = (i >> 6) / MW, m = ln + 64 * q;
        float w = 0.f;
        if (p.spec_type == 1 && m < p.bands) { if (j < T.cnt[m]) w = T.melw[T.off[m] + j]; if (j == 0 && T.cnt[m] > MW) taps_fit = false; }
        s_mwp[i] = w;
    }
    return p.spec_type == 1 && p.bands <= 128 && __syncthreads_and(taps_fit);
}

// =====================================================================================================
// Window and sample prefetch.  Lane m takes complex points 64 a + m, i.e. samples n = 2 (64 a + m) and n + 1.  Branch-free: every lane reads one 8-byte
// pair inside the window (index clamped to win - 2), the lane that owns the last sample of an odd window takes the pair's second half; samples at
// n >= win are replaced by 0.  MASK: the predicates as lane masks in scalar registers (per-lane loop invariants cost no vector register and no branch
// this way; in the 48 kHz instantiation the bool form compiled to two nested exec-mask branches per block with the masks spilled to vector lanes)
__device__ __forceinline__ int fe_pair_index(int n, int win) { return min(n, win - 2); }
// ... the lane's BYTE offset as an unsigned 32-bit word: uniform base + 32-bit lane offset is one address mode, no 64-bit vector arithmetic per load
__device__ __forceinline__ uint32_t fe_pair_offset(int n, int win) { return (uint32_t)max(fe_pair_index(n, win), 0) * 4u; }
template <bool MASK> struct FeWinPred { typename std::conditional<MASK, uint64_t, bool>::type v0, v1, odd; };
template <bool MASK>
__device__ __forceinline__ FeWinPred<MASK> fe_win_pred(int n, int win) {
    FeWinPred<MASK> w;
    if constexpr (MASK) { w.v0 = __ballot(n < win); w.v1 = __ballot(n + 1 < win); w.odd = __ballot(n == win - 1); }
    else { w.v0 = n < win; w.v1 = n + 1 < win; w.odd = n == win - 1; }
    return w;
}
__device__ __forceinline__ float fe_sel(float f, float t, uint64_t mask) { return sel_mask(f, t, mask); }
__device__ __forceinline__ float fe_sel(float f, float t, bool c) { return c ? t : f; }
template <bool MASK>
__device__ __forceinline__ v2f fe_win_select(v2f x, const FeWinPred<MASK>& w) {
    v2f d;                                                 // samples at n >= win are 0; an odd window's last sample sits in .y
    d.x = fe_sel(0.f, fe_sel(x.x, x.y, w.odd), w.v0);
    d.y = fe_sel(0.f, x.y, w.v1);
    return d;
}
// buffer addressing: the wave's first frame is the base of a raw buffer descriptor (four scalar registers, set up per chunk), a frame is a 32-bit SCALAR byte
// offset from it and a lane a 32-bit vector byte offset — no 64-bit vector address arithmetic per load / store (five v_lshl_add_u64 and eight registers before)
template <class T>
__device__ __forceinline__ __amdgpu_buffer_rsrc_t fe_buffer(const T* base) { return __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, 0x7fffffff, 0x00020000); }
template <int AZ>
__device__ __forceinline__ void fe_load_pairs(__amdgpu_buffer_rsrc_t r_in, const uint32_t (&off)[AZ], uint32_t so, v2f (&x)[AZ]) {
#pragma unroll
    for (int a = 0; a < AZ; a++) {
        const u32x2 q = __builtin_amdgcn_raw_buffer_load_b64(r_in, off[a], so, 0);
        x[a] = __builtin_bit_cast(v2f, q);          // (the whole vector: element-wise bit casts of q.x / q.y compile to ONE dword load copied into both halves on this compiler)
    }
}
template <int AZ>
__device__ __forceinline__ void fe_load_pairs(const float* fr, const int (&idx)[AZ], v2f (&x)[AZ]) {
#pragma unroll
    for (int a = 0; a < AZ; a++) {
        const pcm2 q = *reinterpret_cast<const pcm2*>(fr + idx[a]);
        x[a].x = q.x; x[a].y = q.y;
    }
}

// =====================================================================================================
// Chunk = 4 x frames_per_wave frames of one clip; a wave takes frames_per_wave of them.
struct FeChunk { uint32_t f_begin, f_end; const float* pcm; uint32_t* out; };    // the wave's frames [f_begin, f_end) (empty: f_begin >= f_end), the clip's samples and frames
__device__ __forceinline__ FeChunk fe_chunk_of(const FeParams& p, uint32_t clip, uint32_t cx, int wave) {
    FeChunk c;
    const uint32_t nfr = p.n_frames[clip];
    c.f_begin = (cx * 4u + (uint32_t)wave) * (uint32_t)p.frames_per_wave;
    c.f_end = c.f_begin + (uint32_t)p.frames_per_wave;
    if (c.f_end > nfr) c.f_end = nfr;
    // (both offsets through v_readfirstlane: uniform values the compiler then keeps in scalar registers, so that a frame's addresses are scalar arithmetic and the
    //  loads / stores take the "scalar base + 32-bit lane offset" form; the pointers themselves stay derived from the kernel arguments — global address space)
    c.pcm = p.pcm + uniform_u64((uint64_t)clip * p.clip_stride + (p.pcm_off ? p.pcm_off[clip] : 0u));
    c.out = p.spec + uniform_u64((uint64_t)p.frame_off[clip] * (uint32_t)p.bands);
    return c;
}
__device__ __forceinline__ FeChunk fe_chunk(const FeParams& p, uint32_t chunk, uint32_t chunks_per_clip, int wave) {
    // (the quotient comes out of the vector unit — integer division is a float-reciprocal sequence there — and everything derived from it would stay in vector
    //  registers: the clip's frame count a vector load, the frame's output address a v_readfirstlane pair with its wait states in front of every store)
    const uint32_t clip = __builtin_amdgcn_readfirstlane(chunk / chunks_per_clip);
    return fe_chunk_of(p, clip, chunk - clip * chunks_per_clip, wave);
}
// Persistent launch (p.queue): fewer workgroups than chunks, each takes chunk after chunk from a device counter — the number of the chunk after this one is
// requested before the chunk is worked on (right behind the first frame's samples: the two round trips overlap), so its latency is never waited for — and a
// kernel's per-lane constants and tables are set up once per workgroup instead of once per chunk.  s_next: the hand-off of the next chunk's number (two
// slots: one barrier per chunk), phase: the slot in use, nxt: thread 0's answer.  Order of use: ask_first, the caller's barrier, first; then per chunk ask ... next.
// (phase and nxt are the kernel's own two locals: as members of one struct they came out as vector registers that stay alive across the frame loop, two
//  registers more in every 1024-point instantiation and a spill in the one that sits at its 128)
__device__ __forceinline__ void fe_queue_ask_first(const FeParams& p, uint32_t* s_next) { if (p.queue && threadIdx.x == 0) s_next[0] = atomicAdd(p.queue, 1u); }
__device__ __forceinline__ uint32_t fe_queue_first(const FeParams& p, const uint32_t* s_next, uint32_t chunk) {      // chunk: the workgroup's own when there is no queue
    if (p.queue) chunk = s_next[0];
    return __builtin_amdgcn_readfirstlane(chunk);
}
__device__ __forceinline__ void fe_queue_ask(const FeParams& p, uint32_t& nxt) { if (p.queue && threadIdx.x == 0) nxt = atomicAdd(p.queue, 1u); }
__device__ __forceinline__ uint32_t fe_queue_next(uint32_t* s_next, int& phase, uint32_t nxt) {
    phase ^= 1;
    if (threadIdx.x == 0) s_next[phase] = nxt;
    __syncthreads();
    return __builtin_amdgcn_readfirstlane(s_next[phase]);
}

// =====================================================================================================
// The 64-point [8, 8] tail: X1 transpose, radix 8, twiddle W_64^{c b'}, X2 transpose, radix 8.
// ---- the first transpose without LDS.  v[b] of lane (hi3 = h, lo3) <- v[h] of lane (hi3 = b, lo3): the register index and lane bits
// 3 .. 5 change places, one bit pair per stage.  Lane bit 5 / 4 <-> register bit 2 / 1 are gfx950's v_permlane32_swap / v_permlane16_swap (the upper half of
// one register against the lower half of another; the odd 16-lane rows of one against the even rows of another): one instruction per register pair, no
// selects.  Lane bit 3 <-> register bit 0 has no swap instruction: row_ror:8 (lane ^ 8 inside a row) as the DPP operand of a v_cndmask per register.
__device__ __forceinline__ void fe_swap32(v2f& a, v2f& b) {
    const auto rx = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, (float)a.x), __builtin_bit_cast(unsigned, (float)b.x), false, false);
    const auto ry = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, (float)a.y), __builtin_bit_cast(unsigned, (float)b.y), false, false);
    a.x = __builtin_bit_cast(float, (unsigned)rx[0]); b.x = __builtin_bit_cast(float, (unsigned)rx[1]);
    a.y = __builtin_bit_cast(float, (unsigned)ry[0]); b.y = __builtin_bit_cast(float, (unsigned)ry[1]);
}
__device__ __forceinline__ void fe_swap16(v2f& a, v2f& b) {
    const auto rx = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, (float)a.x), __builtin_bit_cast(unsigned, (float)b.x), false, false);
    const auto ry = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, (float)a.y), __builtin_bit_cast(unsigned, (float)b.y), false, false);
    a.x = __builtin_bit_cast(float, (unsigned)rx[0]); b.x = __builtin_bit_cast(float, (unsigned)rx[1]);
    a.y = __builtin_bit_cast(float, (unsigned)ry[0]); b.y = __builtin_bit_cast(float, (unsigned)ry[1]);
}
// lanes 8 .. 15 of every row (bank mask 0xC) take src from lane ^ 8, the others keep old — and the mirror image (bank mask 0x3): v_mov_b32_dpp row_ror:8, no select
__device__ __forceinline__ float fe_ror8_hi(float old, float src) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x128, 0xf, 0xc, false)); }
__device__ __forceinline__ float fe_ror8_lo(float old, float src) { return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, src), 0x128, 0xf, 0x3, false)); }
__device__ __forceinline__ void fe_transpose_hi3(v2f (&v)[8]) {
#pragma unroll
    for (int k = 0; k < 4; k++) fe_swap32(v[k], v[k + 4]);
#pragma unroll
    for (int k = 0; k < 8; k++) if (!(k & 2)) fe_swap16(v[k], v[k + 2]);
#pragma unroll
    for (int k = 0; k < 8; k += 2) {
        const float ax = v[k].x, ay = v[k].y, bx = v[k + 1].x, by = v[k + 1].y;
        v[k].x = fe_ror8_hi(ax, bx); v[k].y = fe_ror8_hi(ay, by);
        v[k + 1].x = fe_ror8_lo(bx, ax); v[k + 1].y = fe_ror8_lo(by, ay);
    }
}
struct FeNothing { __device__ __forceinline__ void operator()() const {} };
// In: u[k], k < AL, of lane m = value m of sub-FFT k (the lanes with hi3 >= AL carry none: R < 8).  Out: lane (al, b') holds c' = 0 .. 7 of its sub-FFT.
//   X1      lane (a', c) gets b = 0..7 of sub-FFT a' — through LDS (row stride XROW: conflict-free), or X1REG: in registers (AL == 8 only: every lane takes part)
//   pass 2  radix 8 over b, twiddle W_64^{c b'} (CM7: as one asm block, the form of the 1024-point kernel; the general families multiply one by one)
//   X2      LDS transpose inside 8-lane groups: lane (a', b') gets c = 0..7  (row stride 9)
//   pass 3  radix 8 over c
// after_x1 / after_x2: what the caller issues behind a transpose, while it is on its way (the pipelined loop of the baseline geometry)
template <bool X1REG, int AL, bool CM7, class F1 = FeNothing, class F2 = FeNothing>
__device__ __forceinline__ void fe_tail64(v2f (&u)[8], v2f* X, const v2f (&tw2)[8], const v2f ss, int lane, F1 after_x1 = F1(), F2 after_x2 = F2()) {
    static_assert(!X1REG || AL == 8, "the register transpose needs all eight sub-FFTs");
    const int hi3 = lane >> 3, lo3 = lane & 7;
    if constexpr (X1REG) fe_transpose_hi3(u);
    else {
#pragma unroll
        for (int k = 0; k < AL; k++) X[k * XROW + lane] = u[k];
        wave_lds_sync();
#pragma unroll
        for (int b = 0; b < 8; b++) { if (AL == 8 || hi3 < AL) u[b] = X[hi3 * XROW + 8 * b + lo3]; else { u[b].x = 0.f; u[b].y = 0.f; } }
        wave_lds_sync();
    }
    after_x1();
    radix8_pk<8>(u, ss);
    if constexpr (CM7) pk_cmul7(u, tw2);
    else {
#pragma unroll
        for (int k = 1; k < 8; k++) u[k] = pk_cmul(u[k], tw2[k]);
    }
#pragma unroll
    for (int k = 0; k < 8; k++) X[hi3 * XROW + k * 9 + lo3] = u[k];
    wave_lds_sync();
#pragma unroll
    for (int c = 0; c < 8; c++) u[c] = X[hi3 * XROW + lo3 * 9 + c];
    wave_lds_sync();
    after_x2();
    radix8_pk<8>(u, ss);
}
__device__ __forceinline__ void fe_tail_twiddles(v2f (&tw2)[8], const FeParams& p, int lane) {
#pragma unroll
    for (int k = 1; k < 8; k++) tw2[k] = to_v2f(p.tw_64[(lane & 7) * k]);
}
__device__ __forceinline__ v2f fe_both(float s) { v2f d; d.x = s; d.y = s; return d; }
constexpr float FE_SQRT_HALF = 0.70710678118654752440f;

// radix-R butterfly of the general families' first pass (R a power of two)
template <int R, int NZ>
__device__ __forceinline__ void radix_r(v2f (&v)[R], const float2* __restrict__ tw64, const v2f ss, const v2f one_mone) {
    // FE-1 butterfly (oracle/frontend.c butterfly()): in place, bit-reversed result, then reordered.
    // Leading non-zero inputs of a block of size 2h: min(NZ, 2h) (no loop-carried state: the loops must unroll
    // completely or the register arrays turn into indexed moves).
#pragma unroll
    for (int h = R / 2; h >= 1; h >>= 1) {
        const int nz = NZ < 2 * h ? NZ : 2 * h;
#pragma unroll
        for (int blk = 0; blk < R; blk += 2 * h) {
#pragma unroll
            for (int j = 0; j < h; j++) {
                const int a = blk + j, b = a + h;
                v2f t;
                if (j + h < nz) { const v2f u = v[a], w = v[b]; v[a] = pk_add(u, w); t = pk_sub(u, w); }
                else if (j < nz) t = v[a];            // w == 0: u + 0 = u, u - 0 = u
                else continue;                        // both structural zeros
                if (j == 0) v[b] = t;
                else if (2 * j == h) v[b] = pk_mi(t, one_mone);
                else if (4 * j == h) v[b] = pk_mul_w8(t, ss);
                else if (4 * j == 3 * h) v[b] = pk_mul_w83(t, ss);
                else v[b] = pk_cmul(t, to_v2f(tw64[j * 32 / h]));
            }
        }
    }
    constexpr int P = R == 2 ? 1 : R == 4 ? 2 : R == 8 ? 3 : R == 16 ? 4 : R == 32 ? 5 : 6;
    v2f y[R];
#pragma unroll
    for (int k = 0; k < R; k++) {
        int r = 0;
#pragma unroll
        for (int i = 0; i < P; i++) r |= ((k >> i) & 1) << (P - 1 - i);
        y[k] = v[r];
    }
#pragma unroll
    for (int k = 0; k < R; k++) v[k] = y[k];
}

// =====================================================================================================
// Real-FFT split: partner values Z[N2 - k] from the partner lane (ds_bpermute); the bin itself is pk_split1 / pk_split5 (fe_common.hpp).
__device__ __forceinline__ v2f fe_shfl(v2f src, int partner) {
    v2f d;
    d.x = __shfl(src.x, partner, 64);
    d.y = __shfl(src.y, partner, 64);
    return d;
}
// The general families: lane (al, b') holds Z[(8g + al) + R b' + 8R c'] in z[8g + c'].  The partner of (a', b', c') is ((R - a') mod R, 7 - b', 7 - c')
// (a' != 0), i.e. a fixed partner lane whose value sits in group R/8 - g - (al > 0): a select between two registers, then ds_bpermute.
// Partner lanes: al > 0: ((R - al) mod 8, 7 - b'); al == 0: group 0 pairs b' with 8 - b' (lane 0 with itself), later groups with 7 - b'
struct FePartners { int g0, gn; };
__device__ __forceinline__ FePartners fe_partners(int R, int lane) {
    const int hi3 = lane >> 3, lo3 = lane & 7;
    const int part_hi = ((((R - hi3) & 7) << 3) | (7 - lo3)) & 63;
    FePartners pt;
    pt.g0 = hi3 > 0 ? part_hi : ((8 - lo3) & 7);
    pt.gn = hi3 > 0 ? part_hi : (7 - lo3);
    return pt;
}
// Z[N2 - k] for the lane's bin of group g, row c (NG groups in z)
template <int NG>
__device__ __forceinline__ v2f fe_partner_value(const v2f (&z)[NG * 8], int g, int c, int lane, const FePartners& pt) {
    const int hi3 = lane >> 3;
    const v2f s_hi = z[8 * (NG - 1 - g) + 7 - c];        // partner's group when al > 0
    const v2f s_lo = z[8 * ((NG - g) % NG) + 7 - c];     // ... when al == 0
    v2f src; src.x = hi3 > 0 ? s_hi.x : s_lo.x; src.y = hi3 > 0 ? s_hi.y : s_lo.y;
    v2f zb = fe_shfl(src, g == 0 ? pt.g0 : pt.gn);
    if (g == 0 && lane == 0) zb = z[(8 - c) & 7];        // k = 8R c pairs with 8R (8 - c)
    return zb;
}

// =====================================================================================================
// Bands (F5-F8).  pidx: where power bin k sits in the wave's power rows; store(m, e): band m's value, to be converted by to_u32.
struct FeIdentity { __device__ __forceinline__ int operator()(int k) const { return k; } };
// the general loop: any number of bands per lane, mel taps from the shared tables, or linear / square-root bins
template <class PIdx, class Store>
__device__ __forceinline__ void fe_bands_general(const FeParams& p, const FeTables& T, const float* P, int lane, PIdx pidx, Store store) {
    for (int m = lane; m < p.bands; m += 64) {
        float e;
        if (p.spec_type == 1) {
            e = 0.f;
            const int kb = T.k0[m], n = T.cnt[m];
            const float* w = T.melw + T.off[m];
            for (int j = 0; j < n; j++) e = __builtin_fmaf(w[j], P[pidx(kb + j)], e);
        } else {
            e = 0.25f * P[pidx(m)];
            if (p.spec_type == 3) e = __builtin_sqrtf(e)  /* correctly rounded (the __fsqrt_rn intrinsic is the raw 1-ulp v_sqrt_f32) */;
        }
        e = e * T.emph[m];
        e = e * p.gain;
        store(m, e);
    }
}
// the two-band form (mel_fast: at most 128 bands, lane takes m = lane and lane + 64, fixed-length chains whose padded taps multiply the zero word), in two steps so that a
// caller can request the taps of both bands — or put other work — before the first multiply-add: the wave issues nothing while it waits for a read
// first bin and tap count of the lane's two bands
__device__ __forceinline__ void fe_mel_first_bin(int (&mk)[2], int (&mn)[2], const FeParams& p, const FeTables& T, int lane) {
#pragma unroll
    for (int q = 0; q < 2; q++) { const int m = lane + 64 * q; const bool has = p.spec_type == 1 && m < p.bands; mk[q] = has ? T.k0[m] : 0; mn[q] = has ? T.cnt[m] : 0; }
}
// The first n of a band's MW taps, cnt of them its own.  A padded tap (j >= cnt) must leave the chain's e alone WHATEVER the power row holds: its weight is
// 0, but fmaf(0, P, e) is e only while P is finite — one bin can overflow to Inf beside finite neighbours (a loud tone under a small pre_norm_gain), and
// 0 * Inf = NaN would turn a band into 0 that FE-1 gives a value.  So a padded tap reads the word of 0.0f at P[zslot] instead of a bin (0 * 0 + e = e for
// every e the chain can hold: e is never -0).  The tap addresses are loop invariants either way: nothing is added to the frame loop.
template <int MW, class PIdx>
__device__ __forceinline__ void fe_mel_taps(float (&pv)[MW], const float* P, int k0, int cnt, int n, int zslot, PIdx pidx) {
#pragma unroll
    for (int j = 0; j < MW; j++) if (j < n) pv[j] = P[j < cnt ? pidx(k0 + j) : zslot];
}
template <int MW>
__device__ __forceinline__ float fe_mel_chain(const float (&w)[MW], const float (&pv)[MW], int n, float emph, float gain) {
    float e = 0.f;
#pragma unroll
    for (int j = 0; j < MW; j++) if (j < n) e = __builtin_fmaf(w[j], pv[j], e);       // (a padded tap is 0 * 0: fe_mel_taps; a tap dropped by n < MW has a zero weight in every band the caller admits)
    e = e * emph;
    return e * gain;
}
// ... with the weights in the padded LDS table of fe_fill_taps (the general families)
template <int MW, class Store>
__device__ __forceinline__ void fe_bands_two(const FeParams& p, const FeTables& T, const float* s_mwp, const float* P, const int (&mk)[2], const int (&mn)[2], int zslot, int lane, Store store) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const int m = lane + 64 * q;
        // (taps and weights of the band requested before the first multiply-add)
        float pvq[MW], wq[MW];
        fe_mel_taps<MW>(pvq, P, mk[q], mn[q], MW, zslot, FeIdentity());
#pragma unroll
        for (int j = 0; j < MW; j++) wq[j] = s_mwp[(q * MW + j) * 64 + lane];
        const float e = fe_mel_chain<MW>(wq, pvq, MW, T.emph[m < p.bands ? m : 0], p.gain);
        if (m < p.bands) store(m, e);
    }
}

// =====================================================================================================
// Host: which instantiation a geometry runs.  Each family's function looks at the plan-constant fields of FeParams only (win, kmax, bands, spec_type,
// mel_total, mel_max_taps, mel_max_taps_lo, fat, wg_per_cu) and launches nothing.
typedef void (*FeKernel)(FeParams);
struct FeChoice {
    FeKernel kernel = nullptr;
    const char* name = "";      // the instantiation as profiles/frontend_split.md writes it (wsa_debug_fe_choice: the tests assert which one a geometry runs)
    size_t lds = 0;             // dynamic LDS bytes
    int queue_wgs = 0;          // persistent launch: most workgroups per CU Tuning::fe_wg_per_cu may ask for (default 2); 0: the kernel takes no queue
    bool grid_2d = false;       // one chunk per workgroup as grid (chunk of the clip, clip); else as a flat grid of chunks
};
FeChoice fe_select_r8(const FeParams& p);              // 1024 points
FeChoice fe_select_rx(const FeParams& p, int R);       // 128 R points, R in {2, 4, 16, 32, 64}
FeChoice fe_select_r3(const FeParams& p, int RM);      // 3 * 128 RM points, RM in {1, 2, 4, 8, 16, 32}

}  // namespace wsa
