// batch_pcm.hip — spec PK-2: a batch's clips as the bytes a WAV holds -> the float staging rows the front end reads.
// One kernel for every format: blockIdx.y is the clip, its 32-byte descriptor (PcmClipDesc, pcm_formats.hpp) says where the clip's bytes
// start (a multiple of 16 behind the 16-byte aligned base), which format they are in, over how many channels the frames are interleaved and
// how many frames there are.  The format switch is uniform per block.
//   mono: a lane takes whole 16-byte chunks (8 i16, 16 u8 / G.711, 4 i32 / f32; two chunks = 4 f64; three chunks = 16 i24), decodes in
//         registers and stores float4s.  Only chunks that lie entirely inside the clip's frames are loaded; the samples behind the last
//         whole unit (fewer than 16) are written one by one.
//   interleaved channels, or staging rows that do not start on 16 bytes: one sample per lane from the sample's own bytes.
// Nothing behind a clip's last frame is read, nothing behind n_frames floats of a row is written.  No LDS, no scratch.
#include "pcm_formats.hpp"

namespace wsa {
namespace {

// one sample from its own bytes with loads of the sample's size (p is aligned to it: clip offsets are multiples of 16); i24 byte by byte
__device__ inline float unpack_sample(int32_t format, const uint8_t* __restrict__ p) {
    switch (format) {
    case WSA_PCM_I16:   return pcm_decode_one<WSA_PCM_I16>(*reinterpret_cast<const uint16_t*>(p));
    case WSA_PCM_MULAW: return pcm_decode_one<WSA_PCM_MULAW>(p[0]);
    case WSA_PCM_ALAW:  return pcm_decode_one<WSA_PCM_ALAW>(p[0]);
    case WSA_PCM_U8:    return pcm_u8_f32(p[0]);
    case WSA_PCM_I24:   return pcm_i24_f32((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
    case WSA_PCM_I32:   return pcm_i32_f32(*reinterpret_cast<const uint32_t*>(p));
    case WSA_PCM_F64:   { const uint2 v = *reinterpret_cast<const uint2*>(p); return pcm_f64_f32(((uint64_t)v.y << 32) | v.x); }
    default:            return __uint_as_float(*reinterpret_cast<const uint32_t*>(p));
    }
}

template <int FORMAT> struct Unit {                 // what one lane takes per round of the mono path
    static constexpr uint32_t CHUNKS = FORMAT == WSA_PCM_I24 ? 3u : FORMAT == WSA_PCM_F64 ? 2u : 1u;      // 16-byte loads
    static constexpr uint32_t SAMPLES = FORMAT == WSA_PCM_I16 ? 8u : (FORMAT == WSA_PCM_F32 || FORMAT == WSA_PCM_I32 || FORMAT == WSA_PCM_F64) ? 4u : 16u;
};

// sample k of a unit whose words are w[0 .. 4 * CHUNKS)
template <int FORMAT>
__device__ inline float unit_sample(const uint32_t* w, uint32_t k) {
    if (FORMAT == WSA_PCM_I16) return pcm_decode_one<WSA_PCM_I16>((w[k >> 1] >> (16u * (k & 1u))) & 0xFFFFu);
    if (FORMAT == WSA_PCM_MULAW) return pcm_decode_one<WSA_PCM_MULAW>((w[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_ALAW) return pcm_decode_one<WSA_PCM_ALAW>((w[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_U8) return pcm_u8_f32((w[k >> 2] >> (8u * (k & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_I32) return pcm_i32_f32(w[k]);
    if (FORMAT == WSA_PCM_F64) return pcm_f64_f32(((uint64_t)w[2u * k + 1u] << 32) | w[2u * k]);
    if (FORMAT == WSA_PCM_I24) {                                   // bytes 3k .. 3k + 2 of the 48: out of one word, or across two
        const uint32_t i = (3u * k) >> 2, sh = 8u * ((3u * k) & 3u);
        const uint64_t two = ((uint64_t)(i + 1u < 12u ? w[i + 1u] : 0u) << 32) | w[i];
        return pcm_i24_f32((uint32_t)(two >> sh));
    }
    return __uint_as_float(w[k]);
}

// whole units of a mono clip, [0, n_units) spread over the clip's lanes: 16-byte loads, float4 stores
template <int FORMAT>
__device__ inline void unpack_units(const uint4* __restrict__ src, float* __restrict__ dst, uint32_t n_units, uint32_t lane0, uint32_t lanes) {
    constexpr uint32_t C = Unit<FORMAT>::CHUNKS, S = Unit<FORMAT>::SAMPLES;
    for (uint32_t u = lane0; u < n_units; u += lanes) {
        uint32_t w[4 * C];
#pragma unroll
        for (uint32_t c = 0; c < C; c++) { const uint4 v = src[(uint64_t)u * C + c]; w[4 * c] = v.x; w[4 * c + 1] = v.y; w[4 * c + 2] = v.z; w[4 * c + 3] = v.w; }
        float4* o = reinterpret_cast<float4*>(dst + (uint64_t)u * S);
#pragma unroll
        for (uint32_t k = 0; k < S; k += 4) o[k >> 2] = make_float4(unit_sample<FORMAT>(w, k), unit_sample<FORMAT>(w, k + 1), unit_sample<FORMAT>(w, k + 2), unit_sample<FORMAT>(w, k + 3));
    }
}
template <int FORMAT> __device__ inline uint32_t unit_samples() { return Unit<FORMAT>::SAMPLES; }

__global__ __launch_bounds__(256) void batch_unpack_kernel(const uint8_t* __restrict__ packed, const PcmClipDesc* __restrict__ desc, float* __restrict__ out, uint64_t stride) {
    const uint32_t clip = blockIdx.y;
    const PcmClipDesc d = desc[clip];
    const uint32_t n = d.n_frames;
    if (n == 0) return;
    const uint8_t* src = packed + d.offset;
    float* dst = out + (uint64_t)clip * stride;
    const uint32_t lane0 = blockIdx.x * 256u + threadIdx.x, lanes = gridDim.x * 256u;
    uint32_t done = 0;                                             // samples the wide path has written
    if (d.channels == 1u && (stride & 3u) == 0) {                  // rows start on 16 bytes: float4 stores
        const uint4* s4 = reinterpret_cast<const uint4*>(src);
#define WSA_UNPACK_CASE(F) case F: done = n / unit_samples<F>() * unit_samples<F>(); unpack_units<F>(s4, dst, n / unit_samples<F>(), lane0, lanes); break;
        switch (d.format) {
        WSA_UNPACK_CASE(WSA_PCM_F32)
        WSA_UNPACK_CASE(WSA_PCM_I16)
        WSA_UNPACK_CASE(WSA_PCM_MULAW)
        WSA_UNPACK_CASE(WSA_PCM_ALAW)
        WSA_UNPACK_CASE(WSA_PCM_U8)
        WSA_UNPACK_CASE(WSA_PCM_I24)
        WSA_UNPACK_CASE(WSA_PCM_I32)
        WSA_UNPACK_CASE(WSA_PCM_F64)
        default: return;                                           // (the host refuses every other number)
        }
#undef WSA_UNPACK_CASE
    }
    const uint64_t step = (uint64_t)d.channels * pcm_sample_bytes(d.format);
    for (uint32_t j = done + lane0; j < n; j += lanes) dst[j] = unpack_sample(d.format, src + (uint64_t)j * step);
}

}  // namespace

void launch_batch_unpack(const void* packed, const PcmClipDesc* desc, uint32_t n_clips, uint32_t max_frames, float* out, uint64_t stride, hipStream_t s) {
    if (!n_clips) return;
    // a lane's round is 4 .. 16 samples: at 8 per lane the longest clip's row is walked in one or two rounds, capped so that a 1024-clip batch stays a few 10^4 blocks
    uint32_t gx = (max_frames + 256u * 8u - 1u) / (256u * 8u);
    gx = gx < 1u ? 1u : gx > 128u ? 128u : gx;
    hipLaunchKernelGGL(batch_unpack_kernel, dim3(gx, n_clips), dim3(256), 0, s, static_cast<const uint8_t*>(packed), desc, out, stride);
}

}  // namespace wsa
