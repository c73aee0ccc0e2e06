// batch_input.hip — how a batch's PCM reaches the float staging buffer the run reads: clips in host memory (float, int16, any packed format, PK-3
// channel selection) uploaded and unpacked on the device, or one packed device buffer in a layout planned ahead (wsa_batch_set_input_*).
#include <system_error>
#include <thread>
#include "batch_internal.hpp"

using namespace wsa;
using wsa_api::fail;
using wsa_api::run_impl;

namespace wsa {
// int16 PCM as uploaded (clip c at in + off[c] values, interleaved over ch[c] channels) -> float32 channel 0 of every clip, x / 32768 (exact)
__global__ void pcm_i16_to_f32_kernel(const int16_t* in, const uint64_t* off, const uint32_t* ch, const uint32_t* ns, float* out, uint64_t stride) {
    const uint32_t c = blockIdx.y;
    const uint32_t n = ns[c], k = ch[c];
    const int16_t* src = in + off[c];
    float* dst = out + (uint64_t)c * stride;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = (float)src[(uint64_t)i * k] * (1.0f / 32768.0f);
}
}  // namespace wsa

// Host -> device copies of many clips.  A copy out of pageable memory is staged by the runtime on the calling thread (~16 GB/s here),
// so large uploads are spread over a few threads (3: 2 .. 4 measure alike, 6 and 8 lose a quarter; WSA_UPLOAD_THREADS) with a stream each; `s` then waits for all of them.  dst(i) / src(i) / bytes(i) per clip.
template <typename DST, typename SRC, typename LEN>
static wsa_status upload_clips(wsa_batch* b, uint32_t n, DST dst, SRC src, LEN bytes, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; i++) total += bytes(i);
    constexpr int UP_MAX = 8;
    int UP_THREADS = 3;
    if (b->tune.upload_threads >= 1 && b->tune.upload_threads <= UP_MAX) UP_THREADS = b->tune.upload_threads;      // tuning knob; 1 = copies on the calling thread
    // Page-locked sources (wsa_host_alloc, or memory the caller registered): the copy is a DMA out of the caller's buffer, no staging thread is needed, and
    // what costs is the number of copies (~10 us of submission each: 1024 clips = 10 ms) — clips that lie back to back in host AND device memory (views into
    // one pinned slab, lengths that keep the device layout's alignment) travel as ONE copy.
    // Every clip is classified (a slab of wsa_host_alloc: a map lookup; anything else: one attribute query): only when ALL of them are page-locked is this
    // path taken — a batch with pageable clips in the middle keeps the worker threads below, which copy page-locked clips just as well.
    {
        bool pinned = n > 0;
        std::vector<uintptr_t> slab_end(n, 0);          // end of the wsa_host_alloc slab clip i lies in (0: page-locked by other means — never merged)
        for (uint32_t i = 0; i < n && pinned; i++) {
            if (!bytes(i)) continue;
            uintptr_t base = 0; size_t size = 0;
            if (wsa_api::slab_of(src(i), &base, &size)) { slab_end[i] = base + size; continue; }
            hipPointerAttribute_t at;
            if (hipPointerGetAttributes(&at, src(i)) != hipSuccess) { (void)hipGetLastError(); pinned = false; }
            else pinned = at.type == hipMemoryTypeHost;
        }
        if (pinned) {
            uint32_t i = 0;
            while (i < n) {
                const char* s0 = reinterpret_cast<const char*>(src(i)); char* d0 = reinterpret_cast<char*>(dst(i));
                size_t len = bytes(i); uint32_t j = i + 1;
                // a run grows while the next clip follows back to back on both sides AND still ends inside the slab the run started in
                while (slab_end[i] && j < n && reinterpret_cast<const char*>(src(j)) == s0 + len && reinterpret_cast<char*>(dst(j)) == d0 + len
                       && reinterpret_cast<uintptr_t>(s0) + len + bytes(j) <= slab_end[i]) { len += bytes(j); j++; }
                if (len) HIP_TRY(ctx, hipMemcpyAsync(d0, s0, len, hipMemcpyHostToDevice, s));
                i = j;
            }
            return WSA_OK;
        }
    }
    if (n < 16 || total < ((uint64_t)32 << 20) || UP_THREADS == 1) {
        for (uint32_t i = 0; i < n; i++) if (bytes(i)) HIP_TRY(ctx, hipMemcpyAsync(dst(i), src(i), bytes(i), hipMemcpyHostToDevice, s));
        return WSA_OK;
    }
    if (!b->up_ready) {
        for (int t = 0; t < UP_MAX; t++) { HIP_TRY(ctx, hipStreamCreateWithFlags(&b->up_stream[t], hipStreamNonBlocking)); HIP_TRY(ctx, hipEventCreateWithFlags(&b->up_event[t], hipEventDisableTiming)); }
        HIP_TRY(ctx, hipEventCreateWithFlags(&b->up_start, hipEventDisableTiming));
        b->up_ready = true;
    }
    // the upload streams start behind what is already queued on `s` (an earlier run may still read the buffers)
    HIP_TRY(ctx, hipEventRecord(b->up_start, s));
    hipError_t err[UP_MAX];
    std::thread th[UP_MAX];
    // contiguous ranges of equal byte counts
    uint32_t first_[UP_MAX + 1]; first_[0] = 0;
    { uint64_t acc = 0; int t = 1; for (uint32_t i = 0; i < n && t < UP_THREADS; i++) { acc += bytes(i); if (acc >= total * t / UP_THREADS) first_[t++] = i + 1; } while (t <= UP_THREADS) first_[t++] = n; }
    first_[UP_THREADS] = n;
    int started = 0;
    for (int t = 0; t < UP_THREADS; t++) {
        err[t] = hipSuccess;
        try {
        th[t] = std::thread([&, t]() {
            hipError_t e = hipSetDevice(ctx->device);
            if (e == hipSuccess) e = hipStreamWaitEvent(b->up_stream[t], b->up_start, 0);
            for (uint32_t i = first_[t]; i < first_[t + 1] && e == hipSuccess; i++) if (bytes(i)) e = hipMemcpyAsync(dst(i), src(i), bytes(i), hipMemcpyHostToDevice, b->up_stream[t]);
            if (e == hipSuccess) e = hipEventRecord(b->up_event[t], b->up_stream[t]);
            err[t] = e;
        });
        } catch (const std::system_error&) { break; }         // no thread to be had: the calling thread takes what is left below
        started++;
    }
    for (int t = 0; t < started; t++) th[t].join();
    hipError_t first = hipSuccess;
    for (int t = started; t < UP_THREADS && first == hipSuccess; t++)       // (ranges whose thread could not be started)
        for (uint32_t i = first_[t]; i < first_[t + 1] && first == hipSuccess; i++) if (bytes(i)) first = hipMemcpyAsync(dst(i), src(i), bytes(i), hipMemcpyHostToDevice, s);
    // `s` waits for every worker's copies, also when one of them failed: none of them may still be writing the batch's buffers when the caller sees the error
    for (int t = 0; t < started; t++) {
        if (err[t] != hipSuccess) { if (first == hipSuccess) first = err[t]; (void)hipStreamSynchronize(b->up_stream[t]); }
        else { const hipError_t e = hipStreamWaitEvent(s, b->up_event[t], 0); if (e != hipSuccess && first == hipSuccess) first = e; }
    }
    HIP_TRY(ctx, first);
    return WSA_OK;
}

// the float staging buffer every entry below unpacks into: [n_clips][staging_stride()], allocated by the first of them
static wsa_status ensure_staging(wsa_batch* b) {
    if (!b->d_pcm_own && !b->mem.alloc(&b->d_pcm_own, (size_t)b->n_clips * b->staging_stride())) return fail(b->ctx, WSA_ERR_HIP, "PCM staging allocation failed");
    return WSA_OK;
}
// one of the two descriptor tables (d_pk_desc: the host runs', d_pkf_desc: the planned layout's), allocated by its first use
static wsa_status ensure_desc_table(wsa_batch* b, PcmClipDesc** table) {
    if (!*table && !b->mem.alloc(table, (size_t)b->n_clips)) return fail(b->ctx, WSA_ERR_HIP, "packed clip table allocation failed");
    return WSA_OK;
}

// PK-2: the clips' formats and channel counts -> one descriptor per clip, clip i's bytes at a multiple of 16; off [n_clips + 1], off[n_clips] = bytes in all
static wsa_status plan_packed(wsa_batch* b, const int32_t* formats, const uint32_t* channels, std::vector<PcmClipDesc>& desc, std::vector<uint64_t>& off) {
    wsa_ctx* ctx = b->ctx;
    if (!formats && b->n_clips) return fail(ctx, WSA_ERR_INVALID, "null formats: one WSA_PCM_* number per clip");
    const std::vector<uint32_t>& ns_host = b->host_samples();
    desc.assign(b->n_clips ? b->n_clips : 1, PcmClipDesc{}); off.assign((size_t)b->n_clips + 1, 0);
    for (uint32_t i = 0; i < b->n_clips; i++) {
        const uint32_t ch = channels ? channels[i] : 1u;
        if (!pcm_format_known(formats[i]))
            return fail(ctx, WSA_ERR_INVALID, "clip " + std::to_string(i) + ": unknown input format " + std::to_string(formats[i])
                        + " (WSA_PCM_F32 0, WSA_PCM_I16 1, WSA_PCM_MULAW 2, WSA_PCM_ALAW 3, WSA_PCM_U8 8, WSA_PCM_I24 9, WSA_PCM_I32 10, WSA_PCM_F64 11)");
        if (ch < 1 || ch > 64) return fail(ctx, WSA_ERR_INVALID, "clip " + std::to_string(i) + ": channel count " + std::to_string(ch) + " outside 1 .. 64");
        desc[i].offset = off[i]; desc[i].format = formats[i]; desc[i].channels = ch; desc[i].n_frames = ns_host[i];
        off[i + 1] = off[i] + (((uint64_t)ns_host[i] * ch * pcm_sample_bytes(formats[i]) + 15u) & ~15ull);
    }
    return WSA_OK;
}
// PK-3: any channel, every channel or the mix (pcm_channels.hip)
static wsa_status plan_channels(wsa_batch* b, const int32_t* formats, const uint32_t* channels, const uint32_t* select, const uint32_t* source,
                                std::vector<PcmClipDesc>& desc, std::vector<uint64_t>& off) {
    const std::string err = pcm_plan_channels(b->n_clips, b->host_samples().data(), formats, channels, select, source, desc, off);
    return err.empty() ? WSA_OK : fail(b->ctx, WSA_ERR_INVALID, err);
}

// a planned layout's kernel: batch_unpack_kernel (PK-2) or batch_deinterleave_kernel (PK-3), packed clips -> the staging buffer
typedef void (*UnpackLaunch)(const void* packed, const PcmClipDesc* desc, uint32_t n_clips, uint32_t max_frames, float* out, uint64_t stride, hipStream_t s);

// wsa_batch_run_host_packed / _channels behind their planners: the clips go into one upload buffer (own allocation, grown when a run needs more than
// the last one) at the planned offsets, clip i bringing clip_bytes(i) bytes, their table into d_pk_desc; `unpack` and the run follow
template <typename BYTES>
static wsa_status run_host_planned(wsa_batch* b, const void* const* pcm, const std::vector<PcmClipDesc>& desc, const std::vector<uint64_t>& off, BYTES clip_bytes,
                                   UnpackLaunch unpack, hipStream_t s) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const wsa_status st = ensure_staging(b); st != WSA_OK) return st;
    if (!b->d_pk || off[b->n_clips] > b->pk_cap) {
        if (b->d_pk) { (void)hipFree(b->d_pk); b->d_pk = nullptr; b->pk_cap = 0; }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&b->d_pk), (size_t)off[b->n_clips] + 16));
        b->pk_cap = off[b->n_clips];
    }
    if (const wsa_status st = ensure_desc_table(b, &b->d_pk_desc); st != WSA_OK) return st;
    b->h_pk_desc = desc;                                           // (the table travels from a buffer the batch owns: the copy is asynchronous)
    HIP_TRY(ctx, hipMemcpyAsync(b->d_pk_desc, b->h_pk_desc.data(), b->h_pk_desc.size() * sizeof(PcmClipDesc), hipMemcpyHostToDevice, s));
    if (const wsa_status st = upload_clips(b, b->n_clips, [&](uint32_t i) { return b->d_pk + off[i]; }, [&](uint32_t i) { return pcm[i]; }, clip_bytes, s); st != WSA_OK) return st;
    unpack(b->d_pk, b->d_pk_desc, b->n_clips, b->max_host_samples(), b->d_pcm_own, b->staging_stride(), s);
    HIP_TRY(ctx, hipGetLastError());
    return run_impl(b, b->d_pcm_own, b->staging_stride(), nullptr, true, true, s);
}

// wsa_batch_set_input_format / _channels behind their planners: the layout's table goes into d_pkf_desc with a synchronous copy (a captured
// wsa_batch_run_packed reads it at every replay), its offsets stay on the host for wsa_batch_packed_offset
static wsa_status set_planned_layout(wsa_batch* b, const std::vector<PcmClipDesc>& desc, const std::vector<uint64_t>& off, bool channels) {
    wsa_ctx* ctx = b->ctx;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const wsa_status st = ensure_staging(b); st != WSA_OK) return st;
    if (const wsa_status st = ensure_desc_table(b, &b->d_pkf_desc); st != WSA_OK) return st;
    HIP_TRY(ctx, hipMemcpy(b->d_pkf_desc, desc.data(), desc.size() * sizeof(PcmClipDesc), hipMemcpyHostToDevice));
    b->pkf_off = off; b->pkf_set = true; b->pkf_channels = channels;
    return WSA_OK;
}

extern "C" {

wsa_status wsa_batch_run_host(wsa_batch* b, const float* const* pcm, void* stream) {
    if (!b || (!pcm && b->n_clips)) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<uint32_t>& ns_host = b->host_samples();
    const uint64_t stride = b->staging_stride();
    if (const wsa_status st = ensure_staging(b); st != WSA_OK) return st;
    if (const wsa_status st = upload_clips(b, b->n_clips, [&](uint32_t i) { return b->d_pcm_own + (size_t)i * stride; }, [&](uint32_t i) { return pcm[i]; },
                                           [&](uint32_t i) { return (size_t)ns_host[i] * sizeof(float); }, s); st != WSA_OK) return st;
    return run_impl(b, b->d_pcm_own, stride, nullptr, true, true, s);
}

// (its own kernel, 8-byte clip alignment and three tables: folding it into the packed path would change which kernel runs and which clips upload_clips merges)
wsa_status wsa_batch_run_host_i16(wsa_batch* b, const int16_t* const* pcm, const uint32_t* channels, void* stream) {
    if (!b || (!pcm && b->n_clips)) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const std::vector<uint32_t>& ns_host = b->host_samples();
    const uint64_t stride = b->staging_stride();
    if (const wsa_status st = ensure_staging(b); st != WSA_OK) return st;
    // clip offsets inside one int16 upload buffer (8-byte aligned starts), grown when a run needs more than the last one
    std::vector<uint64_t> off(b->n_clips + 1, 0); std::vector<uint32_t> ch(b->n_clips ? b->n_clips : 1, 1u);
    for (uint32_t i = 0; i < b->n_clips; i++) {
        ch[i] = channels ? channels[i] : 1u;
        if (ch[i] < 1 || ch[i] > 64) return fail(ctx, WSA_ERR_INVALID, "channels must be 1 .. 64");
        off[i + 1] = off[i] + (((uint64_t)ns_host[i] * ch[i] + 3u) & ~3ull);
    }
    if (off[b->n_clips] > b->i16_cap) {
        if (b->d_i16) { (void)hipFree(b->d_i16); b->d_i16 = nullptr; b->i16_cap = 0; }
        HIP_TRY(ctx, hipMalloc(reinterpret_cast<void**>(&b->d_i16), (size_t)off[b->n_clips] * sizeof(int16_t) + 16));
        b->i16_cap = off[b->n_clips];
    }
    if (!b->d_i16_off) {
        if (!b->mem.alloc(&b->d_i16_off, (size_t)b->n_clips + 1) || !b->mem.alloc(&b->d_i16_ch, (size_t)b->n_clips + 1) || !b->mem.alloc(&b->d_i16_ns, (size_t)b->n_clips + 1))
            return fail(ctx, WSA_ERR_HIP, "int16 staging allocation failed");
    }
    // (the three small tables travel from buffers the batch owns: the copies are asynchronous)
    b->h_i16_off = off; b->h_i16_ch = ch;
    HIP_TRY(ctx, hipMemcpyAsync(b->d_i16_off, b->h_i16_off.data(), ((size_t)b->n_clips + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(b->d_i16_ch, b->h_i16_ch.data(), (size_t)(b->n_clips ? b->n_clips : 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(b->d_i16_ns, ns_host.data(), (size_t)b->n_clips * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    if (const wsa_status st = upload_clips(b, b->n_clips, [&](uint32_t i) { return b->d_i16 + off[i]; }, [&](uint32_t i) { return pcm[i]; },
                                           [&](uint32_t i) { return (size_t)ns_host[i] * ch[i] * sizeof(int16_t); }, s); st != WSA_OK) return st;
    if (b->n_clips) {
        const uint32_t mx = b->max_host_samples();
        hipLaunchKernelGGL(pcm_i16_to_f32_kernel, dim3((mx + 1023) / 1024 ? (mx + 1023) / 1024 : 1, b->n_clips), dim3(256), 0, s, b->d_i16, b->d_i16_off, b->d_i16_ch, b->d_i16_ns, b->d_pcm_own, stride);
        HIP_TRY(ctx, hipGetLastError());
    }
    return run_impl(b, b->d_pcm_own, stride, nullptr, true, true, s);
}

wsa_status wsa_batch_run_host_packed(wsa_batch* b, const void* const* pcm, const int32_t* formats, const uint32_t* channels, void* stream) {
    if (!b || (!pcm && b->n_clips)) return WSA_ERR_INVALID;
    std::vector<PcmClipDesc> desc; std::vector<uint64_t> off;
    if (const wsa_status st = plan_packed(b, formats, channels, desc, off); st != WSA_OK) return st;
    return run_host_planned(b, pcm, desc, off, [&](uint32_t i) { return (size_t)desc[i].n_frames * desc[i].channels * pcm_sample_bytes(desc[i].format); },
                            launch_batch_unpack, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_run_host_channels(wsa_batch* b, const void* const* pcm, const int32_t* formats, const uint32_t* channels, const uint32_t* select,
                                       const uint32_t* source, void* stream) {
    if (!b || (!pcm && b->n_clips)) return WSA_ERR_INVALID;
    std::vector<PcmClipDesc> desc; std::vector<uint64_t> off;
    if (const wsa_status st = plan_channels(b, formats, channels, select, source, desc, off); st != WSA_OK) return st;
    // a source's bytes travel once; a consumer brings none
    return run_host_planned(b, pcm, desc, off, [&](uint32_t i) { return desc[i].source != i ? (size_t)0 : (size_t)desc[i].n_frames * desc[i].channels * pcm_sample_bytes(desc[i].format); },
                            launch_batch_deinterleave, reinterpret_cast<hipStream_t>(stream));
}

wsa_status wsa_batch_set_input_format(wsa_batch* b, const int32_t* formats, const uint32_t* channels) {
    if (!b) return WSA_ERR_INVALID;
    std::vector<PcmClipDesc> desc; std::vector<uint64_t> off;
    if (const wsa_status st = plan_packed(b, formats, channels, desc, off); st != WSA_OK) return st;
    return set_planned_layout(b, desc, off, false);
}

wsa_status wsa_batch_set_input_channels(wsa_batch* b, const int32_t* formats, const uint32_t* channels, const uint32_t* select, const uint32_t* source) {
    if (!b) return WSA_ERR_INVALID;
    std::vector<PcmClipDesc> desc; std::vector<uint64_t> off;
    if (const wsa_status st = plan_channels(b, formats, channels, select, source, desc, off); st != WSA_OK) return st;
    return set_planned_layout(b, desc, off, true);
}

// (PK-3: pkf_off[i] of a consumer is its source's offset)
uint64_t wsa_batch_packed_offset(const wsa_batch* b, uint32_t clip) { return b && b->pkf_set && clip <= b->n_clips ? b->pkf_off[clip] : 0; }

wsa_status wsa_batch_run_packed(wsa_batch* b, const void* d_packed, void* stream) {
    if (!b) return WSA_ERR_INVALID;
    wsa_ctx* ctx = b->ctx;
    if (!b->pkf_set) return fail(ctx, WSA_ERR_INVALID, "wsa_batch_run_packed before wsa_batch_set_input_format: the clips' formats and offsets are not planned");
    if (!d_packed && b->pkf_off[b->n_clips]) return fail(ctx, WSA_ERR_INVALID, "wsa_batch_run_packed: null packed pointer");
    if (reinterpret_cast<uintptr_t>(d_packed) & 15u) return fail(ctx, WSA_ERR_INVALID, "wsa_batch_run_packed: the packed pointer is not aligned to 16 bytes");
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const uint64_t stride = b->staging_stride();
    const UnpackLaunch unpack = b->pkf_channels ? launch_batch_deinterleave : launch_batch_unpack;
    unpack(d_packed, b->d_pkf_desc, b->n_clips, b->max_host_samples(), b->d_pcm_own, stride, s);
    HIP_TRY(ctx, hipGetLastError());
    return run_impl(b, b->d_pcm_own, stride, nullptr, true, true, s);
}

}  // extern "C"
