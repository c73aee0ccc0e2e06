// pcm_formats.hpp — spec PK-1: a packed sample becomes the float the float path would have been given.  The same
// functions run on the host (wsa_pcm_decode) and in stream_pull_packed_kernel, integer arithmetic first and one exact division.
#pragma once
#include <cstdint>
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
inline uint32_t pcm_sample_bytes(int32_t format) { return format == WSA_PCM_F32 ? 4u : format == WSA_PCM_I16 ? 2u : 1u; }
inline const char* pcm_format_name(int32_t format) {
    return format == WSA_PCM_F32 ? "f32" : format == WSA_PCM_I16 ? "i16" : format == WSA_PCM_MULAW ? "mulaw" : format == WSA_PCM_ALAW ? "alaw" : "unknown";
}

}  // namespace wsa
