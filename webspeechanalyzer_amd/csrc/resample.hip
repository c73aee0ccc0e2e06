// resample.hip — K0: sample-rate conversion in front of the path (spec RS-1), one LANE per output sample.
//
// Stands in for the conversion to the context rate that the browser's decodeAudioData performs before the reference
// ever sees the samples (its offline path decodes into `new OfflineAudioContext(1, 48e6, 48e3)`, ref dist/main.js:2
// @B18769, i.e. always 48 kHz).  The converter is the browser's, not the reference's: nothing in the tree pins it
// ("parity unpinned").  RS-1 = the published windowed-sinc scheme of the Chromium family: 32 taps, 32 + 1 sub-sample
// offset kernels (Blackman window, cut-off 0.9 x the lower Nyquist), linear interpolation between the two neighbouring
// kernels, 16 zeros of history, one fused multiply-add per tap.  Bit-exact against oracle/resample.c (same table, same operation order).
// Also here: K0s, the same conversion inside a stream step (one workgroup per stream, state carried between steps), and the host's rule for
// which outputs a stream may produce so far (resample_ready).
#include "wsa_internal.hpp"
#include <cmath>

namespace wsa {

void build_resample_table(double fs_in, double fs_out, std::vector<float>& K) {
    const double ratio = fs_in / fs_out;
    const double scale = (ratio > 1.0 ? 1.0 / ratio : 1.0) * 0.9;
    const double pi = 3.14159265358979323846;
    K.resize((size_t)(RS_OFFS + 1) * RS_TAPS);
    for (int o = 0; o <= RS_OFFS; o++) {
        const double s = (double)o / RS_OFFS;
        for (int i = 0; i < RS_TAPS; i++) {
            const double pre = pi * ((double)(i - RS_TAPS / 2) - s);
            const double x = ((double)i - s) / RS_TAPS;
            const double w = 0.42 - 0.5 * std::cos(2.0 * pi * x) + 0.08 * std::cos(4.0 * pi * x);
            K[(size_t)o * RS_TAPS + i] = (float)(w * (pre == 0.0 ? scale : std::sin(scale * pre) / pre));
        }
    }
}

uint64_t resample_length(uint64_t n_in, double fs_in, double fs_out) { return (uint64_t)((double)n_in / (fs_in / fs_out)); }

// The LDS image of the table the kernel stages with straight 16-byte copies: 32 rows of pairs [o][i] = (K[o][i], K[o+1][i]), row stride 33 pairs
void resample_table_image(const std::vector<float>& K, std::vector<float>& img) {
    img.assign((size_t)2 * RS_OFFS * (RS_TAPS + 1), 0.f);
    for (int o = 0; o < RS_OFFS; o++)
        for (int i = 0; i < RS_TAPS; i++) {
            img[2 * ((size_t)o * (RS_TAPS + 1) + i)] = K[(size_t)o * RS_TAPS + i];
            img[2 * ((size_t)o * (RS_TAPS + 1) + i) + 1] = K[(size_t)(o + 1) * RS_TAPS + i];
        }
}

// A block converts S * J consecutive outputs of one clip (J = rs_j(S, ratio)), lane t the outputs n0 + t + j S (j < J).  S is a multiple of
// the period L of the conversion (fs_in / fs_out = M / L reduced) whenever that period is short, so that a lane's outputs
// share their sub-sample offset and with it the two kernel rows: the rows are read from LDS once per lane (64 registers)
// instead of once per output.  (Positions are the fp64 products of the specification; where rounding moves an output to a
// neighbouring row — or the period is long — the rows are re-read.)
// Per output the lane needs 32 consecutive inputs and 64 multiply-adds (both rows on the same inputs): the two rows live interleaved,
// (K[o][i], K[o+1][i]) per register pair, and one v_pk_fma_f32 with the input broadcast to both halves advances both sums: 32 VALU
// instructions per output instead of 64 (each half is the IEEE fma of the specification, ascending i).
// A block is as long as its staging: the 8 KB table image and the block's run of inputs (17 KB at 44.1 -> 48 kHz) come in as batches of
// 16-byte loads that are all in flight before the first LDS store (one load per loop trip, as the first version had it, is a global
// round trip per 768 bytes: 27 trips = the whole 2.2 ms of the kernel; profiles/r04_notes.md).
// inputs a block stages: J = RS_STAGED / (S * ratio) outputs per lane, at most 96 (17 KB of staged input + the 8 KB table: five blocks of three
// waves per CU; 44.1 -> 48 kHz J = 20 / 28 / 36: 1.71 / 1.61 / 1.61 ms, 16 -> 48 kHz J = 24 / 48 / 64 / 96: 1.32 / 1.23 / 1.21 / 1.32 ms)
constexpr int RS_STAGED = 4300;
inline int rs_j(int S, double ratio) { const double j = (double)RS_STAGED / ((double)S * ratio); return j < 1.0 ? 1 : (j > 96.0 ? 96 : (int)j); }     // (a factor-16 reduction: one output per lane, 16 KB staged)
constexpr int RS_KSTRIDE = RS_TAPS + 1;
constexpr int RS_IMG4 = 2 * RS_OFFS * RS_KSTRIDE / 4;      // the table image in 16-byte words
typedef float rs_v2f __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) const float rs_lds_cf;
__host__ __device__ inline int rs_xlen(int span) { return (span + 6) & ~3; }    // staged inputs: the span, up to 3 samples in front of it (the run starts at a multiple of 4), rounded up to whole 16-byte words

// What block `bx` of clip `clip` does; both kernels below are this function (p, clip and bx are the same for the whole block).
__device__ __forceinline__ void rs_block(const RsParams& p, float* const s_mem, const uint32_t clip, const uint32_t bx) {
    rs_v2f* const s_k = reinterpret_cast<rs_v2f*>(s_mem);                               // [32][33] pairs
    float* const s_x0 = s_mem + 2 * RS_OFFS * RS_KSTRIDE;                               // s_x0[q] = x[lo4 + q]
    const uint64_t n_in = p.n_in[clip], n_out = p.n_out[clip];
    const int J = p.J;
    if ((uint64_t)bx * (uint64_t)p.chunks * (uint64_t)(p.S * J) >= n_out) return;
    const float* x = p.in + (uint64_t)clip * p.stride_in;
    const int tid = threadIdx.x, nt = blockDim.x;
    constexpr int U = 6;
    // (loads are unconditional from clamped addresses, so that a batch is straight-line code with every load in flight; what a clamped
    //  load fetched for a place outside the clip is replaced by zeros — or, on the clip's edges, by guarded single loads — before the store)
    {
        const float4* timg = reinterpret_cast<const float4*>(p.table);
        float4* d = reinterpret_cast<float4*>(s_mem);
        for (int q0 = 0; q0 < RS_IMG4; q0 += 3 * nt) {
            float4 v[3];
#pragma unroll
            for (int u = 0; u < 3; u++) v[u] = timg[min(q0 + u * nt + tid, RS_IMG4 - 1)];
            asm volatile("" : "+v"(v[0].x), "+v"(v[1].x), "+v"(v[2].x));       // (keeps the loads from sinking into the guarded stores, one round trip each)
#pragma unroll
            for (int u = 0; u < 3; u++) { const int q = q0 + u * nt + tid; if (q < RS_IMG4) d[q] = v[u]; }
        }
    }
    const uint32_t n_out32 = (uint32_t)n_out;
    float* const out = p.out + (uint64_t)clip * p.stride_out;
    // the block takes p.chunks consecutive runs of S * J outputs: the table is staged once for all of them
    for (int c = 0; c < p.chunks; c++) {
    const uint64_t n0 = ((uint64_t)bx * (uint64_t)p.chunks + (uint64_t)c) * (uint64_t)(p.S * J);
    if (n0 >= n_out) break;
    if (c) __syncthreads();                                                 // the previous run's inputs are not needed any more
    int ts = tid;
    asm volatile("" : "+v"(ts));                                            // (what the staging derives from the lane number stays inside the loop: hoisted, it held 90 registers across the multiply-adds)
    // inputs from the first tap of output n0 (rounded down to a multiple of 4 samples) to the last tap of the run's last output
    const int64_t lo = (int64_t)floor((double)n0 * p.ratio) - RS_TAPS / 2;
    const int64_t lo4 = lo & ~(int64_t)3;
    const int xlen4 = rs_xlen(p.span) / 4;
    // s_x0[q] = x[lo4 + q] where that is inside the clip (q_lo <= q <= q_hi), else 0; indices relative to the run's first staged sample fit 32 bits
    const float* xb = x + lo4;
    const int q_lo = lo4 < 0 ? (int)(-lo4) : 0;
    const int64_t hi64 = (int64_t)n_in - 1 - lo4;
    const int q_hi = hi64 > 0x7fffffff ? 0x7fffffff : (int)hi64;            // (>= q_lo: a run with outputs has inputs)
    const int v_lo = (q_lo + 3) & ~3, v_hi = (q_hi - 3) & ~3;               // first / last whole 16-byte word inside the clip
    if ((reinterpret_cast<uintptr_t>(x) & 15u) == 0 && v_hi >= v_lo && q_hi >= 3) {
        float4* d = reinterpret_cast<float4*>(s_x0);
        for (int q0 = 0; q0 < xlen4; q0 += U * nt) {
            float4 v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = *reinterpret_cast<const float4*>(xb + min(max(4 * (q0 + u * nt + ts), v_lo), v_hi));
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int q4 = q0 + u * nt + ts, q = 4 * q4;
                if (q < v_lo || q > v_hi) {                                 // the clip's edges: sample by sample, zeros outside
                    v[u] = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (q4 < xlen4 && q + 3 >= q_lo && q <= q_hi) {
                        if (q >= q_lo) v[u].x = xb[q];
                        if (q + 1 >= q_lo && q + 1 <= q_hi) v[u].y = xb[q + 1];
                        if (q + 2 >= q_lo && q + 2 <= q_hi) v[u].z = xb[q + 2];
                        if (q + 3 <= q_hi) v[u].w = xb[q + 3];
                    }
                }
                if (q4 < xlen4) d[q4] = v[u];
            }
        }
    } else {                                                                // a clip that does not start on a 16-byte boundary (or a run without a whole word inside the clip): words
        const int xlen = 4 * xlen4;
        for (int q0 = 0; q0 < xlen; q0 += U * nt) {
            float v[U];
#pragma unroll
            for (int u = 0; u < U; u++) v[u] = xb[min(max(q0 + u * nt + ts, q_lo), max(q_hi, q_lo))];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const int q = q0 + u * nt + ts;
                if (q < xlen) s_x0[q] = (q >= q_lo && q <= q_hi) ? v[u] : 0.f;
            }
        }
    }
    __syncthreads();
    if (tid >= p.S) continue;
    rs_v2f k12[RS_TAPS];                                                    // (rows held across the staging would cost its registers: 196 instead of 106)
    int o_have = -1;
    // per output beside the 32 packed multiply-adds and 16 LDS reads: position (7 instructions), window start (3), interpolation and
    // store (9).  Outputs are numbered in 32 bits here (a clip holds fewer than 2^32 samples: n_out is 32 bits wide).
    const uint32_t nb = (uint32_t)n0 + (uint32_t)tid;
    const double lo_taps = (double)(lo4 + RS_TAPS / 2);                      // |lo4| < 2^53: exact
    for (int j = 0; j < J; j++) {
        const uint32_t n = nb + (uint32_t)(j * p.S);
        if (n >= n_out32) break;
        // pos = n * ratio; vo = (pos - floor(pos)) * 32; o = (int)vo; f = vo - o — with v_fract_f64 for the two differences (both exact, as the
        // subtractions are) and the window start straight from pos - (lo4 + 16) (exact: 0 <= difference <= pos; the conversion truncates)
        const double pos = (double)n * p.ratio;
        const double vo = __builtin_amdgcn_fract(pos) * RS_OFFS;
        const int o = (int)vo;
        const double f = __builtin_amdgcn_fract(vo);
        if (o != o_have) {
            const rs_v2f* r1 = s_k + o * RS_KSTRIDE;
#pragma unroll
            for (int i = 0; i < RS_TAPS; i++) k12[i] = r1[i];
            o_have = o;
        }
        const int w = (int)(pos - lo_taps);                                  // first input of the window, relative to lo4 (>= 0)
        // one LDS address, sixteen reads with immediate offsets (left alone the compiler folds the array's base into sixteen separate addresses)
        rs_lds_cf* xw = (rs_lds_cf*)(s_x0 + w);
        asm volatile("" : "+v"(xw));
        // all sixteen reads first (LDS answers in order: the multiply-adds start with the first answer), then the chain of 32
        rs_v2f xv[RS_TAPS / 2];
#pragma unroll
        for (int i = 0; i < RS_TAPS / 2; i++) { xv[i].x = xw[2 * i]; xv[i].y = xw[2 * i + 1]; }
        __builtin_amdgcn_sched_barrier(0);
        rs_v2f acc; acc.x = 0.f; acc.y = 0.f;
#pragma unroll
        for (int i = 0; i < RS_TAPS / 2; i++) {
            // (s1, s2) = fma(x[2i], (k1, k2)[2i], (s1, s2)), then the same with x[2i+1]: v_pk_fma_f32, the input broadcast to both halves by op_sel
            rs_v2f xa, xb; xa.x = xv[i].x; xa.y = xv[i].x; xb.x = xv[i].y; xb.y = xv[i].y;
            acc = __builtin_elementwise_fma(xa, k12[2 * i], acc);
            acc = __builtin_elementwise_fma(xb, k12[2 * i + 1], acc);
        }
        out[n] = (float)((1.0 - f) * (double)acc.x + f * (double)acc.y);
    }
    }
}

// one rate for the whole batch: grid = (the longest clip's blocks) x clips, blocks past their clip's end return at once
__global__ __launch_bounds__(512) void resample_kernel(RsParams p) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    rs_block(p, s_mem, blockIdx.y, blockIdx.x);
}

// Clips of different rates: block b takes entry b of the plan-time work list — (clip, block of that clip) — and its clip's rate class.  The list is
// sorted by class, so neighbouring blocks share table and shape, and it holds no entry for outputs a clip does not have.  Entry, class and clip lengths
// are the same for the whole block (scalar loads).  Launched once per class over the class's slice of the list (block size and LDS as the single-rate
// launch has them), or - WSA_RS_ONE_LAUNCH - once over the whole list with the block as large as the largest class needs: lanes beyond a class's S stage
// and then leave, as the lanes of a block's last wave always did (slower: a 160-output class in 320-lane blocks; profiles/mixed_rate.md).  A copy class (fs_in == fs_out) moves RS_COPY_RUN samples per block as they are.
constexpr uint32_t RS_COPY_RUN = 8192;
__global__ __launch_bounds__(512) void resample_mixed_kernel(RsMixedParams m) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const RsWork w = m.work[blockIdx.x];
    const RsClass c = m.cls[m.clip_class[w.clip]];
    if (c.copy) {
        const uint64_t n_in = m.n_in[w.clip], n_out = m.n_out[w.clip], lim = n_out < n_in ? n_out : n_in;
        const uint64_t n0 = (uint64_t)w.blk * RS_COPY_RUN, end = n0 + RS_COPY_RUN < lim ? n0 + RS_COPY_RUN : lim;
        const float* x = m.in + (uint64_t)w.clip * m.stride_in;
        float* const out = m.out + (uint64_t)w.clip * m.stride_out;
        for (uint64_t n = n0 + threadIdx.x; n < end; n += blockDim.x) out[n] = x[n];
        return;
    }
    RsParams p;
    p.in = m.in; p.stride_in = m.stride_in; p.out = m.out; p.stride_out = m.stride_out; p.n_in = m.n_in; p.n_out = m.n_out;
    p.chunks = 1; p.table = m.tables + c.table_off; p.ratio = c.ratio; p.span = c.span; p.S = c.S; p.J = c.J;
    rs_block(p, s_mem, w.clip, w.blk);
}

// ---- K0s: the conversion inside a stream step (wsa_stream_create_mixed).  One workgroup per stream:
//   1. the carried converted samples (overlap history + what has not filled a frame yet) move to the front of the stream's stage row
//      — what stream_stage_kernel does for a plain set, so a mixed set has this node in its place;
//   2. [input history | this step's samples | zeros] goes to LDS beside the stream's table image, the newest RS_HIST of them back to HBM as the next history;
//   3. outputs [Y, Y + n_out) are formed behind the carried samples, each exactly as rs_block forms it: fp64 position from the ABSOLUTE index, the two
//      offset kernels of the pair image, 32 fmaf per sum in ascending tap order (v_pk_fma_f32 advances both sums, each half the IEEE fma), the fp64 blend.
// A step has about a thousand outputs per stream (four per lane): the kernel is a latency chain — table and inputs staged with all loads in flight, one
// barrier, a few outputs per lane — so rs_block's register-resident kernel rows (worth it at 20 to 96 outputs per lane) are not kept: every output
// reads its 32 pairs from LDS.  Every count comes from the host's control words; the kernel never decides how many outputs exist.
constexpr int RS_STREAM_BLOCK = 256;
__global__ __launch_bounds__(RS_STREAM_BLOCK) void resample_stream_kernel(RsStreamParams p) {
    extern __shared__ __attribute__((aligned(16))) float s_mem[];
    const uint32_t s = blockIdx.x, n = p.n, tid = threadIdx.x;
    const uint32_t* ctl = p.ctl + s;
    if (!(ctl[RS_CTL_BITS * n] & 4u)) return;                              // idle in this step: stage row, history and counts stay
    const bool fresh = (ctl[RS_CTL_BITS * n] & 1u) != 0;                   // START: zeros in front of the first sample (RS-1's history)
    const uint32_t n_in = ctl[RS_CTL_NIN * n], n_out = ctl[RS_CTL_NOUT * n], shift = ctl[RS_CTL_SHIFT * n], carry = ctl[RS_CTL_CARRY * n];
    const int32_t dst0 = (int32_t)ctl[RS_CTL_DST * n];
    float* const st = p.stage + (uint64_t)s * p.stage_stride;
    float* const cv = p.conv + (uint64_t)s * p.conv_stride;
    const float* const x = p.in + (uint64_t)s * p.in_stride;
    // 1. towards the front, in ascending runs through registers: a run's stores land below everything a later run still reads
    if (shift) {
        for (uint32_t c0 = 0; c0 < carry; c0 += RS_STREAM_BLOCK) {
            const uint32_t i = c0 + tid;
            const float v = i < carry ? st[shift + i] : 0.f;
            __syncthreads();
            if (i < carry) st[i] = v;
        }
        __syncthreads();                                                   // the outputs below may land on what was just read
    }
    const RsClass c = p.cls[p.stream_class[s]];
    if (c.copy) {                                                          // a stream at the analysis rate: unfiltered, no look-ahead
        for (uint32_t j = tid; j < n_out; j += RS_STREAM_BLOCK) {
            const float v = x[j];
            if (dst0 + (int32_t)j >= 0) st[dst0 + (int32_t)j] = v;
            cv[j] = v;
        }
        return;
    }
    // 2.
    {
        const float4* timg = reinterpret_cast<const float4*>(p.tables + c.table_off);
        float4* d = reinterpret_cast<float4*>(s_mem);
        for (int q = tid; q < RS_IMG4; q += RS_STREAM_BLOCK) d[q] = timg[q];
    }
    float* const s_x = s_mem + 2 * RS_OFFS * RS_KSTRIDE;                   // s_x[q] = input (N - RS_HIST + q), zeros before the START and beyond the newest sample
    float* const hist = p.hist + (uint64_t)s * RS_HIST;
    const uint32_t xlen = min((uint32_t)RS_HIST + n_in + (uint32_t)RS_TAPS, p.xcap);
    for (uint32_t q = tid; q < xlen; q += RS_STREAM_BLOCK)
        s_x[q] = q < (uint32_t)RS_HIST ? (fresh ? 0.f : hist[q]) : (q - RS_HIST < n_in ? x[q - RS_HIST] : 0.f);
    __syncthreads();
    if (tid < (uint32_t)RS_HIST) hist[tid] = s_x[n_in + tid];
    // 3.
    const uint64_t Y = (uint64_t)ctl[RS_CTL_Y_LO * n] | ((uint64_t)ctl[RS_CTL_Y_HI * n] << 32);
    const int64_t in0 = (int64_t)((uint64_t)ctl[RS_CTL_IN0_LO * n] | ((uint64_t)ctl[RS_CTL_IN0_HI * n] << 32));
    const rs_v2f* const s_k = reinterpret_cast<const rs_v2f*>(s_mem);
    for (uint32_t j = tid; j < n_out; j += RS_STREAM_BLOCK) {
        const double pos = (double)(Y + j) * c.ratio;
        const double fl = floor(pos);
        const double vo = (pos - fl) * RS_OFFS;
        const int o = (int)vo;
        const double f = vo - (double)o;
        const int64_t w = (int64_t)fl - RS_TAPS / 2 - in0;                 // first tap in s_x; the host has checked 0 <= w and w + 32 <= xlen
        float v = 0.f;
        if (w >= 0 && w + RS_TAPS <= (int64_t)xlen) {
            const rs_v2f* k = s_k + o * RS_KSTRIDE;
            const float* xw = s_x + w;
            rs_v2f acc; acc.x = 0.f; acc.y = 0.f;
#pragma unroll
            for (int i = 0; i < RS_TAPS; i++) {
                rs_v2f xa; xa.x = xw[i]; xa.y = xw[i];
                acc = __builtin_elementwise_fma(xa, k[i], acc);
            }
            v = (float)((1.0 - f) * (double)acc.x + f * (double)acc.y);
        }
        if (dst0 + (int32_t)j >= 0) st[dst0 + (int32_t)j] = v;
        cv[j] = v;
    }
}

size_t resample_stream_lds(uint32_t xcap) { return sizeof(float) * ((size_t)2 * RS_OFFS * RS_KSTRIDE + (size_t)xcap); }
void launch_resample_stream(const RsStreamParams& p, hipStream_t s) {
    if (p.n) hipLaunchKernelGGL(resample_stream_kernel, dim3(p.n), dim3(RS_STREAM_BLOCK), resample_stream_lds(p.xcap), s, p);
}

// Output n is ready when its last tap has arrived: floor((double)n * ratio) + 16 <= N, the position formed as K0 and oracle/resample.c form it.
// The predicate is monotone in n; the count of ready outputs is found from an estimate by walking the predicate itself, then clamped to the length.
uint64_t resample_ready(uint64_t n_in, double fs_in, double fs_out) {
    if (fs_in == fs_out) return n_in;
    const double ratio = fs_in / fs_out;
    if (n_in < (uint64_t)(RS_TAPS / 2)) return 0;
    auto ready = [&](uint64_t n) { return (uint64_t)std::floor((double)n * ratio) + (uint64_t)(RS_TAPS / 2) <= n_in; };
    uint64_t g = (uint64_t)((double)(n_in - RS_TAPS / 2) / ratio);
    while (g > 0 && !ready(g - 1)) g--;
    while (ready(g)) g++;
    const uint64_t len = resample_length(n_in, fs_in, fs_out);
    return g < len ? g : len;
}

// What one step can produce, for a stream of ratio r that hands in at most cap = ceil(F hop r) <= F hop r + 1 samples:
//   the tap rule alone counts the n with n r < N - 15, so a step adds at most n_in / r + 1 of them; the length clamp holds at most one back
//   (ceil((N - 15) / r) - floor(N / r) < 2 - 15 / r, r <= 16), which a later step hands on: n_in / r + 2 <= F hop + 1 / r + 2 outputs without STOP;
//   with STOP the step ends at floor(N' / r) from at least (N - 15) / r - 1: (n_in + 15) / r + 1 <= F hop + 16 / r + 1.
// One more for the rounding of the fp64 products: F hop + ceil(16 / r) + 3.  Streams at the analysis rate are copied: at most their F hop inputs.
uint32_t resample_step_outputs_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio) {
    const uint64_t base = (uint64_t)frames_per_step * hop;
    const uint64_t v = min_ratio > 0 ? base + (uint64_t)std::ceil(16.0 / min_ratio) + 3 : base;
    return v > 0xffffffffull ? 0xffffffffu : (uint32_t)v;
}
// Frames: before the step Y < K hop + win (frame K is not complete), after it (K' - 1) hop + win <= Y + outputs, so K' - K < outputs / hop + 1.
uint32_t resample_step_frames_bound(uint32_t frames_per_step, uint32_t hop, double min_ratio) {
    if (!hop) return 0;
    const uint64_t o = resample_step_outputs_bound(frames_per_step, hop, min_ratio);
    return (uint32_t)((o + hop - 1) / hop);
}

// outputs per block row: a multiple of the conversion's period when the rates are integers with a short period
int resample_stride(double fs_in, double fs_out) {
    const double ri = std::floor(fs_in), ro = std::floor(fs_out);
    if (ri == fs_in && ro == fs_out && ri > 0 && ro > 0 && ri < 4e9 && ro < 4e9) {
        uint64_t a = (uint64_t)ri, b = (uint64_t)ro;
        while (b) { const uint64_t t = a % b; a = b; b = t; }
        const uint64_t L = (uint64_t)ro / a;                  // outputs per period
        // the multiple of the period closest to 256 from below if it leaves at most a fifth of its last wave's lanes idle (3 -> 255 of 256, 160 -> 160 of
        // 192: small blocks overlap their staging with the other blocks' arithmetic better than large ones — 44.1 -> 48 kHz: S = 160 1.65 ms, 320 2.2 ms),
        // else the multiple up to 512 that wastes the fewest lanes (147 -> 441 of 448)
        if (L <= 512) {
            const uint64_t S0 = L * (256 / L > 0 ? 256 / L : 1);
            auto waste = [](uint64_t S) { return (double)((S + 63) / 64 * 64 - S) / (double)((S + 63) / 64 * 64); };
            if (waste(S0) <= 0.2) return (int)S0;
            uint64_t best = S0;
            for (uint64_t S = L; S <= 512; S += L) if (S >= 128 && waste(S) < waste(best)) best = S;
            return (int)best;
        }
    }
    return 256;
}

int resample_outputs_per_lane(int S, double ratio) { return rs_j(S, ratio); }
int resample_span(double ratio, int S, int J) { return (int)std::ceil((double)(S * J - 1) * ratio) + RS_TAPS + 2; }

// The single-rate launch's shape: ratio, S, J, span and runs per block — each override where it is positive (WSA_RS_S / WSA_RS_J / WSA_RS_C), else the default
void resample_shape(double fs_in, double fs_out, int S, int J, int chunks, RsParams& p) {
    p.ratio = fs_in / fs_out; p.S = S > 0 ? S : resample_stride(fs_in, fs_out);
    p.J = J > 0 ? J : rs_j(p.S, p.ratio); p.span = resample_span(p.ratio, p.S, p.J); p.chunks = chunks > 0 ? chunks : 1;       // (more runs per block never won: tools/resample_sweep.sh)
}
uint32_t resample_block(const RsParams& p) { return (uint32_t)((p.S + 63) / 64 * 64); }
size_t resample_lds(const RsParams& p) { return sizeof(float) * ((size_t)2 * RS_OFFS * RS_KSTRIDE + (size_t)rs_xlen(p.span)); }

void launch_resample(const RsParams& p, uint32_t n_clips, uint64_t max_out, hipStream_t s) {
    if (n_clips == 0 || max_out == 0) return;
    const uint64_t per_block = (uint64_t)p.S * (uint64_t)p.J * (uint64_t)p.chunks;
    const dim3 grid((unsigned)((max_out + per_block - 1) / per_block), n_clips), block(resample_block(p));
    hipLaunchKernelGGL(resample_kernel, grid, block, resample_lds(p), s, p);
}

// The rate classes of a mixed batch (the distinct fs_in, in order of first appearance) and the work list: per class every clip's blocks, clip by clip.
bool plan_resample_mixed(uint32_t n_clips, const uint32_t* n_out, const double* fs_in, double fs_out, RsMixedPlan& P, std::string& err) {
    P = RsMixedPlan();
    P.clip_class.resize(n_clips);
    std::vector<double> rates;
    for (uint32_t i = 0; i < n_clips; i++) {
        size_t c = 0;
        while (c < rates.size() && rates[c] != fs_in[i]) c++;       // (a map from the rate's bits would do for thousands of distinct rates; a folder has a handful)
        if (c == rates.size()) {
            rates.push_back(fs_in[i]);
            RsClass k = {};
            k.ratio = fs_in[i] / fs_out;
            if (fs_in[i] == fs_out) { k.copy = 1; P.block.push_back(256); P.lds.push_back(0); }
            else {
                std::vector<float> K0, K; build_resample_table(fs_in[i], fs_out, K0); resample_table_image(K0, K);
                k.table_off = (uint32_t)P.tables.size();
                P.tables.insert(P.tables.end(), K.begin(), K.end());
                k.S = resample_stride(fs_in[i], fs_out); k.J = rs_j(k.S, k.ratio); k.span = resample_span(k.ratio, k.S, k.J);
                P.block.push_back((uint32_t)((k.S + 63) / 64 * 64));
                P.lds.push_back((uint32_t)(sizeof(float) * ((size_t)2 * RS_OFFS * RS_KSTRIDE + (size_t)rs_xlen(k.span))));
            }
            P.cls.push_back(k);
            if (P.block.back() > P.max_block) P.max_block = P.block.back();
            if (P.lds.back() > P.max_lds) P.max_lds = P.lds.back();
        }
        P.clip_class[i] = (uint32_t)c;
    }
    P.first.assign(P.cls.size() + 1, 0);
    for (size_t c = 0; c < P.cls.size(); c++) {
        const uint64_t per_block = P.cls[c].copy ? (uint64_t)RS_COPY_RUN : (uint64_t)P.cls[c].S * (uint64_t)P.cls[c].J;
        for (uint32_t i = 0; i < n_clips; i++) {
            if (P.clip_class[i] != c) continue;
            const uint64_t nb = ((uint64_t)n_out[i] + per_block - 1) / per_block;
            if ((uint64_t)P.work.size() + nb > 0x7fffffffull) { err = "the batch needs more rate-converter blocks than one launch holds"; return false; }
            for (uint64_t b = 0; b < nb; b++) P.work.push_back(RsWork{i, (uint32_t)b});
        }
        P.first[c + 1] = (uint32_t)P.work.size();
    }
    P.n_work = (uint32_t)P.work.size();
    return true;
}

void launch_resample_mixed(const RsMixedParams& p, const RsMixedPlan& P, bool per_class, hipStream_t s) {
    if (P.n_work == 0) return;
    if (!per_class) {
        hipLaunchKernelGGL(resample_mixed_kernel, dim3(P.n_work), dim3(P.max_block), P.max_lds, s, p);
        return;
    }
    for (size_t c = 0; c < P.cls.size(); c++) {
        if (P.first[c + 1] == P.first[c]) continue;
        RsMixedParams q = p; q.work = p.work + P.first[c];
        hipLaunchKernelGGL(resample_mixed_kernel, dim3(P.first[c + 1] - P.first[c]), dim3(P.block[c]), P.lds[c], s, q);
    }
}

}  // namespace wsa
