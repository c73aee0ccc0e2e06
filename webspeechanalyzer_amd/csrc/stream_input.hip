// stream_input.hip — how a step's samples reach the front end: the set's input format (PK-1, wsa_stream_set_input_format) or channel selection (PK-3,
// wsa_stream_set_input_channels), the kernels that pull or decode the rows into floats inside the step, and the history shuffle of overlapping windows.
#include <algorithm>
#include "stream_internal.hpp"

using namespace wsa;
using wsa_api::fail;

namespace wsa {
// history shuffle for overlapping windows: stage[s] = [last `hist` samples of the previous stage | new samples]
__global__ __launch_bounds__(256) void stream_stage_kernel(float* stage, uint32_t stage_stride, const float* pcm, uint64_t pcm_stride,
                                                           const uint32_t* ctl_bits, uint32_t hist, uint32_t step_samples) {
    extern __shared__ float s_hist[];
    const uint32_t s = blockIdx.x;
    if (!(ctl_bits[s] & 4u)) return;                       // bit 2 of the device control word: stream active in this step
    float* st = stage + (uint64_t)s * stage_stride;
    for (uint32_t i = threadIdx.x; i < hist; i += 256) s_hist[i] = st[step_samples + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < hist; i += 256) st[i] = s_hist[i];
    const float* src = pcm + (uint64_t)s * pcm_stride;
    for (uint32_t i = threadIdx.x; i < step_samples; i += 256) st[hist + i] = src[i];
}
// host -> device through the mapped pinned buffer (a kernel node: H2D memcpy nodes of more than a few KB from
// pinned memory faulted inside captured graphs on ROCm 7.2 / gfx950, the same copy outside a graph was fine)
__global__ __launch_bounds__(256) void stream_pull_kernel(float* dst, const float* __restrict__ src, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 3 < n) *reinterpret_cast<float4*>(dst + i) = *reinterpret_cast<const float4*>(src + i);
    else for (size_t k = i; k < n; k++) dst[k] = src[k];
}
// packed host or device input -> floats in d_pcm_in (spec PK-1), a kernel node like the float pull.  One block row per stream; a lane takes
// whole 16-byte chunks of the stream's row (8 i16 samples or 16 G.711 codes), decodes channel 0's samples in registers and stores floats.
// Rows of streams that are not active in the step are skipped, and so is everything behind the step's count of a stream.
// ctl: the device control words the step's prologue has just written (word w of stream s at ctl[w * n + s]); count_word = 0: every
// active stream carries fixed_count samples (a plain set), else the word that holds the stream's count (RS_CTL_NIN of a mixed set).
// The caller guarantees count * channels * sample size <= src_stride, src and src_stride multiples of 16, count <= dst_stride.
template <int FORMAT>
__global__ __launch_bounds__(128) void stream_pull_packed_kernel(float* __restrict__ dst, uint32_t dst_stride, const uint8_t* __restrict__ src, uint64_t src_stride,
                                                                 const uint32_t* __restrict__ chan, const uint32_t* __restrict__ ctl, uint32_t n,
                                                                 uint32_t count_word, uint32_t fixed_count) {
    constexpr uint32_t E = FORMAT == WSA_PCM_I16 ? 8u : 16u;      // samples in a 16-byte chunk
    constexpr uint32_t PER = E / 4u;                               // samples per 32-bit word
    constexpr uint32_t BITS = 32u / PER, MASK = BITS == 16u ? 0xFFFFu : 0xFFu;
    const uint32_t s = blockIdx.x;
    if (!(ctl[RS_CTL_BITS * n + s] & 4u)) return;
    const uint32_t cnt = count_word ? ctl[count_word * n + s] : fixed_count;
    if (cnt == 0) return;
    const uint32_t ch = chan[s];
    const uint4* row = reinterpret_cast<const uint4*>(src + (uint64_t)s * src_stride);
    float* out = dst + (uint64_t)s * dst_stride;
    const uint32_t n_el = (cnt - 1u) * ch + 1u;                   // elements of the row up to channel 0 of the last frame (cnt <= 2^24, ch <= 64)
    const uint32_t n_chunks = (n_el + E - 1u) / E;
    const bool vec = (dst_stride & 3u) == 0;                       // rows of d_pcm_in start on 16 bytes
    for (uint32_t c = blockIdx.y * 128u + threadIdx.x; c < n_chunks; c += gridDim.y * 128u) {
        const uint32_t e0 = c * E;
        if (ch == 1u) {
            const uint4 v = row[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
            float f[E];
#pragma unroll
            for (uint32_t k = 0; k < E; k++) f[k] = pcm_decode_one<FORMAT>((w[k / PER] >> (BITS * (k % PER))) & MASK);
            if (vec && e0 + E <= cnt) {
#pragma unroll
                for (uint32_t k = 0; k < E; k += 4) *reinterpret_cast<float4*>(out + e0 + k) = make_float4(f[k], f[k + 1], f[k + 2], f[k + 3]);
            } else {
#pragma unroll
                for (uint32_t k = 0; k < E; k++) if (e0 + k < cnt) out[e0 + k] = f[k];
            }
        } else {
            uint32_t j = (e0 + ch - 1u) / ch;                      // first frame whose channel 0 lies in this chunk or behind it
            uint32_t next = j * ch - e0;
            if (next >= E || j >= cnt) continue;                   // no sample of channel 0 in this chunk: not loaded
            const uint4 v = row[c];
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < E; k++)
                if (k == next && j < cnt) { out[j] = pcm_decode_one<FORMAT>((w[k / PER] >> (BITS * (k % PER))) & MASK); j++; next += ch; }
        }
    }
}
// spec PK-3 for streams: stream s takes channel sel[s], or the mix, of the packed row of stream srcs[s] — one sample per lane from the sample's own
// bytes (a step's few hundred samples per stream; the source's row is read once per stream that takes from it).  Counts and control words are the
// stream's own; the caller guarantees that the source's row holds the stream's count of frames.
template <int FORMAT>
__global__ __launch_bounds__(128) void stream_pull_channels_kernel(float* __restrict__ dst, uint32_t dst_stride, const uint8_t* __restrict__ src, uint64_t src_stride,
                                                                   const uint32_t* __restrict__ chan, const uint32_t* __restrict__ sel, const uint32_t* __restrict__ srcs,
                                                                   const uint32_t* __restrict__ ctl, uint32_t n, uint32_t count_word, uint32_t fixed_count) {
    constexpr uint32_t SB = FORMAT == WSA_PCM_I16 ? 2u : 1u;
    const uint32_t s = blockIdx.x;
    if (!(ctl[RS_CTL_BITS * n + s] & 4u)) return;
    const uint32_t cnt = count_word ? ctl[count_word * n + s] : fixed_count;
    const uint32_t ch = chan[s], pick = sel[s];
    const uint8_t* row = src + (uint64_t)srcs[s] * src_stride;
    float* out = dst + (uint64_t)s * dst_stride;
    for (uint32_t j = blockIdx.y * 128u + threadIdx.x; j < cnt; j += gridDim.y * 128u) {
        const uint8_t* fr = row + (uint64_t)j * ch * SB;
        out[j] = pick == WSA_CHANNEL_MIX ? pcm_mix_frame(ch, [&](uint32_t c) { return pcm_decode_bytes(FORMAT, fr + c * SB); }) : pcm_decode_bytes(FORMAT, fr + pick * SB);
    }
}
}  // namespace wsa

// one packed format's pull: a lane per frame with channel selection (PK-3), else a lane per 16-byte chunk (PK-1)
template <int FORMAT>
static void pull_packed(wsa_stream* b, const uint8_t* src, uint64_t src_stride, hipStream_t s) {
    const uint32_t n = b->n;
    const uint32_t count_word = b->mixed ? (uint32_t)RS_CTL_NIN : 0u;
    if (b->chsel) {
        const dim3 gsel(n, (unsigned)std::min<uint32_t>((b->in_stride + 127u) / 128u, 1024u));
        hipLaunchKernelGGL(stream_pull_channels_kernel<FORMAT>, gsel, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_sel, b->d_sel + n, b->d_ctl, n, count_word, b->step_samples);
        return;
    }
    constexpr uint32_t per_chunk = FORMAT == WSA_PCM_I16 ? 8u : 16u;
    const uint64_t chunks = ((uint64_t)b->in_stride * b->max_ch + per_chunk - 1) / per_chunk;
    const dim3 grid(n, (unsigned)std::min<uint64_t>((chunks + 127) / 128, 1024));
    hipLaunchKernelGGL(stream_pull_packed_kernel<FORMAT>, grid, dim3(128), 0, s, b->d_pcm_in, b->in_stride, src, src_stride, b->d_chan, b->d_ctl, n, count_word, b->step_samples);
}

void wsa_api::launch_stream_pull(wsa_stream* b, const float** d_pcm, uint64_t* stride, bool host_in, hipStream_t s) {
    if (b->fmt != WSA_PCM_F32) {
        const uint8_t* src = host_in ? b->h_pk_dev : reinterpret_cast<const uint8_t*>(*d_pcm);
        const uint64_t src_stride = host_in ? b->pk_stride : *stride;
        if (b->fmt == WSA_PCM_I16) pull_packed<WSA_PCM_I16>(b, src, src_stride, s);
        else if (b->fmt == WSA_PCM_MULAW) pull_packed<WSA_PCM_MULAW>(b, src, src_stride, s);
        else pull_packed<WSA_PCM_ALAW>(b, src, src_stride, s);
    } else if (host_in) {
        const size_t cnt = (size_t)b->n * b->in_stride;
        hipLaunchKernelGGL(stream_pull_kernel, dim3((unsigned)((cnt / 4 + 256) / 256)), dim3(256), 0, s, b->d_pcm_in, b->h_pcm_dev, cnt);
    } else return;
    *d_pcm = b->d_pcm_in; *stride = b->in_stride;
}

void wsa_api::launch_stream_stage(wsa_stream* b, const float* d_pcm, uint64_t stride, hipStream_t s) {
    hipLaunchKernelGGL(stream_stage_kernel, dim3(b->n), dim3(256), (size_t)b->hist * sizeof(float), s,
                       b->d_stage, b->stage_stride, d_pcm, stride, b->d_ctl + 2 * b->n, b->hist, b->step_samples);
}

// wsa_stream_set_input_format (select and source NULL, chsel false: the PK-1 pull kernel) and wsa_stream_set_input_channels (PK-3).
// Everything is validated first; then the last step is awaited, the graph dropped and the old buffers freed; WSA_PCM_F32 allocates nothing
static wsa_status set_input_impl(wsa_stream* b, int32_t format, const uint32_t* channels, const uint32_t* select, const uint32_t* source, bool chsel) {
    wsa_ctx* ctx = b->ctx;
    if (format != WSA_PCM_F32 && format != WSA_PCM_I16 && format != WSA_PCM_MULAW && format != WSA_PCM_ALAW)
        return fail(ctx, WSA_ERR_INVALID, "unknown input format " + std::to_string(format) + " (WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3)");
    uint32_t max_ch = 1;
    for (uint32_t i = 0; channels && i < b->n; i++) {
        if (chsel && source && source[i] != i) continue;          // a consumer takes its source's channel count, its own entry is not read
        if (channels[i] < 1 || channels[i] > 64) return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": channel count " + std::to_string(channels[i]) + " outside 1 .. 64");
        if (format == WSA_PCM_F32 && channels[i] != 1)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": " + std::to_string(channels[i]) + " channels with WSA_PCM_F32: float input is mono, interleaved channels need a packed format");
        if (channels[i] > max_ch) max_ch = channels[i];
    }
    std::vector<uint32_t> ss(chsel ? 2 * (size_t)b->n : 0, 0u);     // [select | source], a consumer's channel count is its source's
    std::vector<uint32_t> ch_of(b->n, 1u);
    for (uint32_t i = 0; chsel && i < b->n; i++) {
        const uint32_t src = source ? source[i] : i;
        if (src >= b->n) return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " outside 0 .. " + std::to_string(b->n - 1));
        if ((source ? source[src] : src) != src)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " is not its own source (it reads stream " + std::to_string(source[src]) + ")");
        ch_of[i] = channels ? channels[src] : 1u;
        ss[i] = select ? select[i] : 0u; ss[b->n + i] = src;
        if (!pcm_select_known(ss[i], ch_of[i]))
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": select " + std::to_string(ss[i]) + " is neither a channel below " + std::to_string(ch_of[i]) + " nor WSA_CHANNEL_MIX");
        if (format == WSA_PCM_F32 && src != i)
            return fail(ctx, WSA_ERR_INVALID, "stream " + std::to_string(i) + ": source " + std::to_string(src) + " with WSA_PCM_F32: float input has one row per stream, shared rows need a packed format");
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (b->stepped) HIP_TRY(ctx, hipStreamSynchronize(b->last_stream ? b->last_stream : b->own));     // the last step may still read the buffer
    b->drop_graph();                                           // the next step recaptures with the format's pull kernel
    if (b->h_pk) { (void)hipHostFree(b->h_pk); b->h_pk = b->h_pk_dev = nullptr; }
    if (b->d_chan) { (void)hipFree(b->d_chan); b->d_chan = nullptr; }
    if (b->d_sel) { (void)hipFree(b->d_sel); b->d_sel = nullptr; }
    b->fmt = WSA_PCM_F32; b->chan.clear(); b->pk_stride = 0; b->max_ch = 1; b->chsel = false;
    if (format == WSA_PCM_F32) return WSA_OK;
    std::vector<uint32_t> ch(b->n, 1u);
    if (chsel) ch = ch_of;
    else if (channels) ch.assign(channels, channels + b->n);
    const uint64_t row = ((uint64_t)b->in_stride * max_ch * pcm_sample_bytes(format) + 15u) & ~(uint64_t)15u;
    if (row > 0xFFFFFFF0ull) return fail(ctx, WSA_ERR_INVALID, "a packed input row of " + std::to_string(row) + " bytes: fewer channels or frames per step");
    void *hp = nullptr, *hd = nullptr, *dc = nullptr, *ds = nullptr;
    bool ok = hipHostMalloc(&hp, (size_t)row * b->n, hipHostMallocMapped) == hipSuccess;
    if (ok && chsel) ok = hipMalloc(&ds, ss.size() * sizeof(uint32_t)) == hipSuccess && hipMemcpy(ds, ss.data(), ss.size() * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (ok) { std::memset(hp, 0, (size_t)row * b->n); ok = hipHostGetDevicePointer(&hd, hp, 0) == hipSuccess; }
    ok = ok && hipMalloc(&dc, (size_t)b->n * sizeof(uint32_t)) == hipSuccess && hipMemcpy(dc, ch.data(), (size_t)b->n * sizeof(uint32_t), hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        const std::string m = std::string("packed input buffer allocation failed: ") + hipGetErrorString(hipGetLastError());
        if (hp) (void)hipHostFree(hp);
        if (dc) (void)hipFree(dc);
        if (ds) (void)hipFree(ds);
        return fail(ctx, WSA_ERR_HIP, m);
    }
    b->h_pk = static_cast<uint8_t*>(hp); b->h_pk_dev = static_cast<uint8_t*>(hd); b->d_chan = static_cast<uint32_t*>(dc); b->d_sel = static_cast<uint32_t*>(ds);
    b->fmt = format; b->chan = ch; b->pk_stride = (uint32_t)row; b->max_ch = max_ch; b->chsel = chsel;
    return WSA_OK;
}

extern "C" {
wsa_status wsa_stream_set_input_format(wsa_stream* b, int32_t format, const uint32_t* channels) {
    return b ? set_input_impl(b, format, channels, nullptr, nullptr, false) : WSA_ERR_INVALID;
}
wsa_status wsa_stream_set_input_channels(wsa_stream* b, int32_t format, const uint32_t* channels, const uint32_t* select, const uint32_t* source) {
    return b ? set_input_impl(b, format, channels, select, source, true) : WSA_ERR_INVALID;
}
}  // extern "C"
