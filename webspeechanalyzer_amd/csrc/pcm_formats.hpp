// pcm_formats.hpp — specs PK-1, PK-2 and PK-3: a packed sample becomes the float the float path would have been given.  The same
// functions run on the host (wsa_pcm_decode, wsa_pcm_decode_select), in stream_pull_packed_kernel, stream_pull_channels_kernel,
// batch_unpack_kernel and batch_deinterleave_kernel: integer arithmetic first, then one conversion and one exact division.
#pragma once
#include <cstdint>
#include <string>
#include <vector>
#include <hip/hip_runtime.h>
#include "../../include/wsa.h"

namespace wsa {

// ITU-T G.711 mu-law code -> 16-bit linear value (+-32124; codes 0x7F and 0xFF give 0)
__host__ __device__ inline int32_t pcm_mulaw_linear(uint32_t code) {
    const uint32_t u = ~code & 0xFFu, e = (u >> 4) & 7u, m = u & 15u;
    const int32_t mag = (int32_t)((((m << 3) + 0x84u) << e) - 0x84u);
    return (u & 0x80u) ? -mag : mag;
}
// ITU-T G.711 A-law code -> 16-bit linear value (+-32256; 0x55 gives -8, 0xD5 gives +8)
__host__ __device__ inline int32_t pcm_alaw_linear(uint32_t code) {
    const uint32_t a = (code ^ 0x55u) & 0xFFu, e = (a >> 4) & 7u, m = a & 15u;
    const int32_t mag = (int32_t)(e == 0 ? (m << 4) + 8u : ((m << 4) + 0x108u) << (e - 1u));
    return (a & 0x80u) ? mag : -mag;
}
// raw: the sample's bits in the low 16 (i16) or low 8 (G.711) of a word.  Every value is an integer below 2^15 in magnitude (or -2^15): the
// division by 2^15 is exact in fp32.
template <int FORMAT>
__host__ __device__ inline float pcm_decode_one(uint32_t raw) {
    if (FORMAT == WSA_PCM_I16) return (float)(int32_t)(int16_t)(uint16_t)raw / 32768.0f;
    if (FORMAT == WSA_PCM_MULAW) return (float)pcm_mulaw_linear(raw) / 32768.0f;
    return (float)pcm_alaw_linear(raw) / 32768.0f;
}
// ---- PK-2: the linear encodings a WAV holds, little-endian (batches only)
// 8-bit unsigned: (x - 128) / 128, exact
__host__ __device__ inline float pcm_u8_f32(uint32_t x) { return (float)((int32_t)(x & 0xFFu) - 128) / 128.0f; }
// 24-bit signed in the low 24 bits of a word: the sign-extended value / 2^23, exact in fp32
__host__ __device__ inline float pcm_i24_f32(uint32_t x) { return (float)((int32_t)(x << 8) >> 8) / 8388608.0f; }
// 32-bit signed: the conversion rounds to nearest even (2^31 - 1 gives 2^31), the division by 2^31 is exact: fl32(x / 2^31)
__host__ __device__ inline float pcm_i32_f32(uint32_t x) { return (float)(int32_t)x / 2147483648.0f; }
// the bits of a double -> the bits of the nearest float, ties to even, in integer arithmetic: the result does not depend on a denormal mode
// (results below 2^-126 are fp32 denormals and are kept), overflow gives +-Inf, -0 stays -0, a NaN stays a (quiet) NaN
__host__ __device__ inline uint32_t pcm_f64_bits_to_f32_bits(uint64_t b) {
    const uint32_t sign = (uint32_t)(b >> 32) & 0x80000000u, e = (uint32_t)(b >> 52) & 0x7FFu;
    const uint64_t m = b & 0xFFFFFFFFFFFFFull;
    if (e == 0x7FFu) return sign | 0x7F800000u | (m ? 0x400000u | (uint32_t)(m >> 29) : 0u);
    const int32_t E = (int32_t)e - 1023 + 127;                       // the float's biased exponent
    if (E >= 255) return sign | 0x7F800000u;
    if (E >= 1) {                                                    // normal: 23 of the 52 fraction bits, a carry out of them moves the exponent (up to Inf)
        const uint32_t q = ((uint32_t)E << 23) | (uint32_t)(m >> 29), rem = (uint32_t)m & 0x1FFFFFFFu;
        return sign | (q + ((rem > 0x10000000u || (rem == 0x10000000u && (q & 1u))) ? 1u : 0u));
    }
    if (e == 0 || E < -24) return sign;                              // below half of the smallest denormal (2^-150)
    const uint32_t sh = 30u - (uint32_t)E;                           // 30 .. 54: the 53-bit significand in units of 2^-149
    const uint64_t sig = m | (1ull << 52), q = sh >= 64u ? 0ull : sig >> sh, rem = sig & ((1ull << sh) - 1ull), half = 1ull << (sh - 1u);
    return sign | ((uint32_t)q + ((rem > half || (rem == half && (q & 1ull))) ? 1u : 0u));
}
__host__ __device__ inline float pcm_bits_f32(uint32_t u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float f; __builtin_memcpy(&f, &u, 4); return f;
#endif
}
__host__ __device__ inline float pcm_f64_f32(uint64_t bits) { return pcm_bits_f32(pcm_f64_bits_to_f32_bits(bits)); }

// one sample of any format from its own bytes (p: the sample's first byte, any alignment): the host's statement, and the kernel's path for
// interleaved channels and tails
__host__ __device__ inline float pcm_decode_bytes(int32_t format, const uint8_t* p) {
    switch (format) {
    case WSA_PCM_I16:   return pcm_decode_one<WSA_PCM_I16>((uint32_t)p[0] | ((uint32_t)p[1] << 8));
    case WSA_PCM_MULAW: return pcm_decode_one<WSA_PCM_MULAW>(p[0]);
    case WSA_PCM_ALAW:  return pcm_decode_one<WSA_PCM_ALAW>(p[0]);
    case WSA_PCM_U8:    return pcm_u8_f32(p[0]);
    case WSA_PCM_I24:   return pcm_i24_f32((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16));
    case WSA_PCM_I32:   return pcm_i32_f32((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));
    case WSA_PCM_F64: {
        uint64_t b = 0;
        for (int k = 7; k >= 0; k--) b = (b << 8) | p[k];
        return pcm_f64_f32(b);
    }
    default:            return pcm_bits_f32((uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24));      // WSA_PCM_F32: bit for bit
    }
}
__host__ __device__ inline bool pcm_format_known(int32_t format) { return (format >= WSA_PCM_F32 && format <= WSA_PCM_ALAW) || (format >= WSA_PCM_U8 && format <= WSA_PCM_F64); }
// bytes of one sample; 0 for a format nobody knows (4 .. 7 are kept for further 8-bit companded codes)
__host__ __device__ inline uint32_t pcm_sample_bytes(int32_t format) {
    return format == WSA_PCM_F32 || format == WSA_PCM_I32 ? 4u : format == WSA_PCM_I16 ? 2u : format == WSA_PCM_I24 ? 3u : format == WSA_PCM_F64 ? 8u
         : format == WSA_PCM_MULAW || format == WSA_PCM_ALAW || format == WSA_PCM_U8 ? 1u : 0u;
}
inline const char* pcm_format_name(int32_t format) {
    return format == WSA_PCM_F32 ? "f32" : format == WSA_PCM_I16 ? "i16" : format == WSA_PCM_MULAW ? "mulaw" : format == WSA_PCM_ALAW ? "alaw"
         : format == WSA_PCM_U8 ? "u8" : format == WSA_PCM_I24 ? "i24" : format == WSA_PCM_I32 ? "i32" : format == WSA_PCM_F64 ? "f64" : "unknown";
}

// ---- PK-3: what a clip or a stream takes from its interleaved frames.  select: a channel index below `channels`, or WSA_CHANNEL_MIX
__host__ __device__ inline bool pcm_select_known(uint32_t select, uint32_t channels) { return select < channels || select == WSA_CHANNEL_MIX; }
// the mix of one frame: at(c) is channel c's decoded float.  fp32 additions in ascending channel order, then ONE multiply by fl32(1 / channels);
// every decode scale is a power of two, so no product in front of an addition is inexact and a contracted build gives the same bits
template <class At>
__host__ __device__ inline float pcm_mix_frame(uint32_t channels, At at) {
    float acc = at(0u);
    if (channels == 1u) return acc;                                  // the plain decode, bit for bit
    for (uint32_t c = 1; c < channels; c++) acc = acc + at(c);
    return acc * (1.0f / (float)channels);
}

// ---- batch_unpack_kernel (batch_pcm.hip), batch_deinterleave_kernel (pcm_channels.hip): one 32-byte descriptor per clip
struct PcmClipDesc {
    uint64_t offset;       // bytes from the packed base to the clip's first byte, a multiple of 16 (PK-3: the first byte of the clip's source)
    int32_t format;        // WSA_PCM_*
    uint32_t channels;     // 1 .. 64
    uint32_t n_frames;     // floats written to the clip's staging row
    // PK-3 only (batch_unpack_kernel reads none of them)
    uint32_t select;       // channel index, or WSA_CHANNEL_MIX
    uint32_t source;       // the clip whose bytes this one reads; a source names itself
    uint32_t next;         // the next clip that reads the same source, PCM_NO_CLIP behind the last: a source heads the list of its consumers
};
static_assert(sizeof(PcmClipDesc) == 32, "one 32-byte descriptor per clip");
constexpr uint32_t PCM_NO_CLIP = 0xFFFFFFFFu;
// PK-3's tile: frames of one source a workgroup of batch_deinterleave_kernel holds in LDS at a time.  A multiple of 16, so that a tile's bytes
// are whole 16-byte chunks for every format and channel count; at most PCM_TILE_BYTES (64 channels of f64, 512 bytes a frame: 32 frames)
constexpr uint32_t PCM_TILE_BYTES = 16384u, PCM_TILE_MAX_FRAMES = 2048u;
__host__ __device__ inline uint32_t pcm_tile_frames(int32_t format, uint32_t channels) {
    const uint32_t fb = channels * pcm_sample_bytes(format);
    if (fb == 0) return 0;
    const uint32_t t = (PCM_TILE_BYTES / fb) & ~15u;
    return t > PCM_TILE_MAX_FRAMES ? PCM_TILE_MAX_FRAMES : t;
}
// PK-3: every source's tiles once through LDS, one float row per clip that reads it.  desc as plan_channels (batch_input.hip) builds it.
void launch_batch_deinterleave(const void* packed, const PcmClipDesc* desc, uint32_t n_clips, uint32_t max_frames, float* out, uint64_t stride, hipStream_t s);
// PK-3's plan (pcm_channels.hip): desc [n_clips], off [n_clips + 1] (off[i]: where clip i's source starts, off[n_clips]: bytes in all); the refusal's text, or empty
std::string pcm_plan_channels(uint32_t n_clips, const uint32_t* n_frames, const int32_t* formats, const uint32_t* channels, const uint32_t* select,
                              const uint32_t* source, std::vector<PcmClipDesc>& desc, std::vector<uint64_t>& off);
// packed (16-byte aligned) + desc[c].offset -> out + c * stride, channel 0 of desc[c].n_frames frames; max_frames: the longest clip's count (sizes the grid)
void launch_batch_unpack(const void* packed, const PcmClipDesc* desc, uint32_t n_clips, uint32_t max_frames, float* out, uint64_t stride, hipStream_t s);

}  // namespace wsa
