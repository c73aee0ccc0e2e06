// pcm_channels.hip — spec PK-3: interleaved clips -> one float staging row per clip that reads them, any channel or the mono mix.
// batch_deinterleave_kernel: blockIdx.y is a clip; a clip that is not its own source leaves at once.  A source's workgroups walk its tiles of
// T = pcm_tile_frames(format, channels) frames (a multiple of 16: a tile's first byte lies on 16 bytes, its length is whole 16-byte chunks):
//   load    the tile's bytes ONCE, 16-byte loads, lanes side by side — only chunks that lie wholly inside the source's frames; the bytes of the
//           ragged tail (fewer than 16, in the source's last tile alone) one by one.  Nothing behind the source's last frame is read.
//   decode  for every clip on the source's list (the source itself first, then desc.next): lane k takes frames k, k + 256, ... of the tile out of
//           LDS — its selected channel, or all channels in ascending order for the mix — with the decode functions of pcm_formats.hpp, and stores
//           one float; a wave's 64 floats lie side by side in the clip's row.  Nothing behind a clip's own frame count is written.
// LDS layout: word w of the tile lies at w + (w >> 5), one pad word behind every 32.  ds_read_b32 and ds_write_b32 bank by (address / 4) mod 32
// over the two 32-lane halves of a wave.  Lanes read one frame apart, S = channels * sample bytes / 4 words: unpadded, a power of two S >= 2 puts
// a half's 32 lanes on 32 / S banks (64 channels of i32: all on one).  Padded, lane l reads l * S + (l * S >> 5): S = 2 .. 32 is conflict-free,
// S = 64 two-way, S = 128 (64 channels of f64) four-way; odd byte strides (i24, odd channel counts of the 8- and 16-bit formats) spread by
// themselves.  The tile's stores (lane l: words 4l .. 4l + 3, word k of the four at bank 4l + k + (l >> 3) mod 32) are conflict-free.
// No scratch; 16.6 KiB of LDS per workgroup.
#include "pcm_formats.hpp"

namespace wsa {
namespace {

constexpr uint32_t TILE_WORDS = PCM_TILE_BYTES / 4u;
constexpr uint32_t LDS_WORDS = TILE_WORDS + TILE_WORDS / 32u + 2u;     // (+ the word an i24 sample's second read may touch behind the tile)
__device__ inline uint32_t pad_word(uint32_t w) { return w + (w >> 5); }

// element e (sample index inside the tile: frame * channels + channel) out of the padded tile
template <int FORMAT>
__device__ inline float tile_sample(const uint32_t* tile, uint32_t e) {
    if (FORMAT == WSA_PCM_I16) return pcm_decode_one<WSA_PCM_I16>((tile[pad_word(e >> 1)] >> (16u * (e & 1u))) & 0xFFFFu);
    if (FORMAT == WSA_PCM_MULAW) return pcm_decode_one<WSA_PCM_MULAW>((tile[pad_word(e >> 2)] >> (8u * (e & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_ALAW) return pcm_decode_one<WSA_PCM_ALAW>((tile[pad_word(e >> 2)] >> (8u * (e & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_U8) return pcm_u8_f32((tile[pad_word(e >> 2)] >> (8u * (e & 3u))) & 0xFFu);
    if (FORMAT == WSA_PCM_I32) return pcm_i32_f32(tile[pad_word(e)]);
    if (FORMAT == WSA_PCM_F64) return pcm_f64_f32(((uint64_t)tile[pad_word(2u * e + 1u)] << 32) | tile[pad_word(2u * e)]);
    if (FORMAT == WSA_PCM_I24) {                                   // bytes 3e .. 3e + 2: out of one word, or across two (the second word is needed only then)
        const uint32_t w = (3u * e) >> 2, sh = 8u * ((3u * e) & 3u);
        const uint64_t two = ((uint64_t)tile[pad_word(w + 1u)] << 32) | tile[pad_word(w)];
        return pcm_i24_f32((uint32_t)(two >> sh));
    }
    return __uint_as_float(tile[pad_word(e)]);
}

// one clip's part of the tile: frames [f0, f0 + nf) of the source -> dst[f0 ...], nf already cut to the clip's own frame count
template <int FORMAT>
__device__ inline void tile_decode(const uint32_t* tile, float* __restrict__ dst, uint32_t nf, uint32_t channels, uint32_t select) {
    if (select == WSA_CHANNEL_MIX) {
        for (uint32_t k = threadIdx.x; k < nf; k += 256u) {
            const uint32_t e0 = k * channels;
            dst[k] = pcm_mix_frame(channels, [&](uint32_t c) { return tile_sample<FORMAT>(tile, e0 + c); });
        }
    } else {
        for (uint32_t k = threadIdx.x; k < nf; k += 256u) dst[k] = tile_sample<FORMAT>(tile, k * channels + select);
    }
}

template <int FORMAT>
__device__ inline void source_tiles(uint32_t* tile, const uint8_t* __restrict__ src, const PcmClipDesc* __restrict__ desc, uint32_t clip, uint32_t C, uint32_t n,
                                    uint32_t select, uint32_t next, uint32_t n_clips, float* __restrict__ out, uint64_t stride) {
    const uint32_t T = pcm_tile_frames(FORMAT, C);
    const uint32_t frame_bytes = C * pcm_sample_bytes(FORMAT);
    const uint64_t src_bytes = (uint64_t)n * frame_bytes;          // nothing at or behind src + src_bytes is read
    const uint32_t n_tiles = (n + T - 1u) / T;
    for (uint32_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const uint64_t b0 = (uint64_t)t * T * frame_bytes;         // a multiple of 16
        const uint64_t left = src_bytes - b0;
        const uint32_t tb = left < (uint64_t)T * frame_bytes ? (uint32_t)left : T * frame_bytes;       // the tile's bytes, <= PCM_TILE_BYTES
        const uint32_t whole = tb >> 4;
        const uint4* s4 = reinterpret_cast<const uint4*>(src + b0);
        for (uint32_t q = threadIdx.x; q < whole; q += 256u) {
            const uint4 v = s4[q];
            uint32_t* p = tile + pad_word(4u * q);                 // words 4q .. 4q + 3 lie in one group of 32
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        }
        if (threadIdx.x < (tb & 15u))                              // the ragged tail: up to 15 bytes, a lane each (the four words they lie in are one group of 32)
            reinterpret_cast<uint8_t*>(tile + pad_word(4u * whole))[threadIdx.x] = src[b0 + 16u * (uint64_t)whole + threadIdx.x];
        __syncthreads();
        const uint32_t f0 = t * T;
        uint32_t c = clip, c_frames = n, c_select = select, c_next = next;
        for (uint32_t guard = 0; guard < n_clips; guard++) {       // the source, then every clip that reads it (the list ends within n_clips entries)
            if (c_frames > f0) {
                const uint32_t nf = c_frames - f0 < T ? c_frames - f0 : T;
                tile_decode<FORMAT>(tile, out + (uint64_t)c * stride + f0, nf, C, c_select);
            }
            c = c_next;
            if (c >= n_clips) break;
            c_frames = desc[c].n_frames < n ? desc[c].n_frames : n;    // (the host refuses a consumer longer than its source)
            c_select = desc[c].select; c_next = desc[c].next;
        }
        __syncthreads();                                           // the next round's loads overwrite the tile
    }
}

__global__ __launch_bounds__(256) void batch_deinterleave_kernel(const uint8_t* __restrict__ packed, const PcmClipDesc* __restrict__ desc, uint32_t n_clips,
                                                                 float* __restrict__ out, uint64_t stride) {
    __shared__ uint32_t tile[LDS_WORDS];
    const uint32_t clip = blockIdx.y;
    const uint32_t n = desc[clip].n_frames;
    if (desc[clip].source != clip || n == 0) return;               // a consumer's row is written by its source's workgroups; consumers are no longer than their source
    const uint8_t* src = packed + desc[clip].offset;
    const uint32_t C = desc[clip].channels, select = desc[clip].select, next = desc[clip].next;
#define WSA_TILE_CASE(F) case F: source_tiles<F>(tile, src, desc, clip, C, n, select, next, n_clips, out, stride); break;
    switch (desc[clip].format) {                                            // uniform per workgroup
    WSA_TILE_CASE(WSA_PCM_F32)
    WSA_TILE_CASE(WSA_PCM_I16)
    WSA_TILE_CASE(WSA_PCM_MULAW)
    WSA_TILE_CASE(WSA_PCM_ALAW)
    WSA_TILE_CASE(WSA_PCM_U8)
    WSA_TILE_CASE(WSA_PCM_I24)
    WSA_TILE_CASE(WSA_PCM_I32)
    WSA_TILE_CASE(WSA_PCM_F64)
    default: return;                                               // (the host refuses every other number)
    }
#undef WSA_TILE_CASE
}

}  // namespace

// PK-3's plan, shared by the batch entries (batch_input.hip) and wsa_debug_batch_deinterleave: checks select and source, gives a consumer its source's format,
// channel count and offset, lays the sources' bytes out in clip order at multiples of 16 and threads every source's list.  Empty string: fine.
std::string pcm_plan_channels(uint32_t n_clips, const uint32_t* n_frames, const int32_t* formats, const uint32_t* channels, const uint32_t* select,
                              const uint32_t* source, std::vector<PcmClipDesc>& desc, std::vector<uint64_t>& off) {
    desc.assign(n_clips ? n_clips : 1, PcmClipDesc{}); off.assign((size_t)n_clips + 1, 0);
    const auto clip = [](uint32_t i) { return "clip " + std::to_string(i) + ": "; };
    if (!formats && n_clips) return "null formats: one WSA_PCM_* number per clip";
    for (uint32_t i = 0; i < n_clips; i++) {                       // sources first: a consumer may stand in front of its source
        const uint32_t src = source ? source[i] : i;
        if (src >= n_clips) return clip(i) + "source " + std::to_string(src) + " outside 0 .. " + std::to_string(n_clips - 1);
        if ((source ? source[src] : src) != src) return clip(i) + "source " + std::to_string(src) + " is not its own source (it reads clip " + std::to_string(source[src]) + ")";
    }
    uint64_t at = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        if ((source ? source[i] : i) != i) continue;
        const uint32_t ch = channels ? channels[i] : 1u;
        if (!pcm_format_known(formats[i]))
            return clip(i) + "unknown input format " + std::to_string(formats[i])
                   + " (WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3, WSA_PCM_U8 8, WSA_PCM_I24 9, WSA_PCM_I32 10, WSA_PCM_F64 11)";
        if (ch < 1 || ch > 64) return clip(i) + "channel count " + std::to_string(ch) + " outside 1 .. 64";
        desc[i].offset = at; desc[i].format = formats[i]; desc[i].channels = ch;
        at += ((uint64_t)n_frames[i] * ch * pcm_sample_bytes(formats[i]) + 15u) & ~15ull;
    }
    off[n_clips] = at;
    std::vector<uint32_t> last(n_clips ? n_clips : 1);             // the end of every source's list so far
    for (uint32_t i = 0; i < n_clips; i++) { last[i] = i; desc[i].next = PCM_NO_CLIP; }
    for (uint32_t i = 0; i < n_clips; i++) {
        const uint32_t src = source ? source[i] : i, sel = select ? select[i] : 0u;
        PcmClipDesc& d = desc[i];
        d.offset = desc[src].offset; d.format = desc[src].format; d.channels = desc[src].channels; d.n_frames = n_frames[i]; d.select = sel; d.source = src;
        off[i] = d.offset;
        if (!pcm_select_known(sel, d.channels))
            return clip(i) + "select " + std::to_string(sel) + " is neither a channel below " + std::to_string(d.channels) + " nor WSA_CHANNEL_MIX";
        if (n_frames[i] > n_frames[src])
            return clip(i) + std::to_string(n_frames[i]) + " frames, its source clip " + std::to_string(src) + " holds " + std::to_string(n_frames[src]);
        if (src != i) { desc[last[src]].next = i; last[src] = i; }
    }
    return std::string();
}

void launch_batch_deinterleave(const void* packed, const PcmClipDesc* desc, uint32_t n_clips, uint32_t max_frames, float* out, uint64_t stride, hipStream_t s) {
    if (!n_clips) return;
    // a workgroup's round is one tile of 32 .. 2048 frames: one workgroup per 2048 frames of the longest clip walks a stereo 16-bit source in one round and a
    // 64-channel one in up to 128, capped so that a 1024-clip batch stays a few 10^4 workgroups
    uint32_t gx = (max_frames + PCM_TILE_MAX_FRAMES - 1u) / PCM_TILE_MAX_FRAMES;
    gx = gx < 1u ? 1u : gx > 128u ? 128u : gx;
    hipLaunchKernelGGL(batch_deinterleave_kernel, dim3(gx, n_clips), dim3(256), 0, s, static_cast<const uint8_t*>(packed), desc, n_clips, out, stride);
}

}  // namespace wsa
