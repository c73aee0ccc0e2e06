// debug_input.hip — test entries of libwsa that are NOT part of include/wsa.h, for the kernels in front of the front end: PK-2's batch_unpack_kernel
// (csrc/batch_pcm.hip), PK-3's batch_deinterleave_kernel (csrc/pcm_channels.hip) and K0, the batch rate converter (csrc/resample.hip: resample_kernel,
// resample_mixed_kernel).  Host bytes or clips in, one launch through the product's own launch functions, floats back.
#include <cmath>
#include <cstring>
#include <vector>
#include "api_internal.hpp"
#include "debug_internal.hpp"
#include "pcm_formats.hpp"

using namespace wsa_debug;

// PK-2's kernel (csrc/batch_pcm.hip) on its own: host-given packed bytes through ONE launch of batch_unpack_kernel, floats back.  off [n_clips + 1]:
// clip i's bytes start at packed + off[i] (a multiple of 16) and lie in front of off[i + 1]; off[n_clips] = the bytes of `packed`.  out [n_clips][stride]
// goes to the device as the caller filled it and comes back: what the kernel did not write keeps the caller's value.
// Refused, nothing run: an unknown format, channels outside 1 .. 64, an offset that is no multiple of 16, a clip whose frames do not fit between its
// offset and the next or into a row of `stride` floats.
extern "C" int wsa_debug_batch_unpack(int32_t device, const void* packed, const uint64_t* off, const int32_t* formats, const uint32_t* channels,
                                      const uint32_t* n_frames, uint32_t n_clips, float* out, uint64_t stride) {
    if (!off || !formats || !channels || !n_frames || !out || n_clips < 1 || n_clips > 65535u || stride < 1 || stride > (1u << 26)) return WSA_ERR_INVALID;
    if (off[0] != 0 || off[n_clips] > (1ull << 32) || (off[n_clips] && !packed)) return WSA_ERR_INVALID;
    std::vector<wsa::PcmClipDesc> desc(n_clips);
    uint32_t max_frames = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        if (!wsa::pcm_format_known(formats[i]) || channels[i] < 1 || channels[i] > 64 || (off[i] & 15u) || off[i + 1] < off[i] || n_frames[i] > stride) return WSA_ERR_INVALID;
        const uint64_t need = n_frames[i] ? ((uint64_t)(n_frames[i] - 1u) * channels[i] + 1u) * wsa::pcm_sample_bytes(formats[i]) : 0;   // up to channel 0 of the last frame
        if (need > off[i + 1] - off[i]) return WSA_ERR_INVALID;
        desc[i] = wsa::PcmClipDesc{off[i], formats[i], channels[i], n_frames[i], 0, 0, 0};
        if (n_frames[i] > max_frames) max_frames = n_frames[i];
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; uint4* dp = nullptr; wsa::PcmClipDesc* dd = nullptr; float* dout = nullptr;
    const size_t nout = (size_t)n_clips * stride;
    bool ok = A.alloc(&dp, (size_t)(off[n_clips] + 15u) / 16u) && put(reinterpret_cast<char*>(dp), static_cast<const char*>(packed), (size_t)off[n_clips])
           && A.upload(&dd, desc) && up(A, &dout, out, nout);
    if (ok) {
        wsa::launch_batch_unpack(dp, dd, n_clips, max_frames, dout, stride, nullptr);
        ok = ran() && down(out, dout, nout);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// PK-3's kernel (csrc/pcm_channels.hip) on its own: host-given packed bytes through ONE launch of batch_deinterleave_kernel, floats back.  The plan is
// pcm_plan_channels', as the batch entries use it: off_out [n_clips + 1] comes back as planned (off_out[i]: where clip i's source starts), `packed` holds
// packed_bytes bytes laid out by it — call with out == NULL first to get the offsets alone.  out [n_clips][stride] (any stride >= the longest clip, multiples
// of four or not) goes to the device as the caller filled it and comes back: what the kernel did not write keeps the caller's value.  The device buffer is
// exactly packed_bytes long.  Refused, nothing run: what the plan refuses (its message goes to err [err_cap], the planning call needs no device), a clip
// longer than `stride`, fewer bytes than the plan needs.
extern "C" int wsa_debug_batch_deinterleave(int32_t device, const void* packed, uint64_t packed_bytes, const int32_t* formats, const uint32_t* channels,
                                            const uint32_t* select, const uint32_t* source, const uint32_t* n_frames, uint32_t n_clips, uint64_t* off_out,
                                            float* out, uint64_t stride, char* err, uint32_t err_cap) {
    if (err && err_cap) err[0] = 0;
    if (!formats || !n_frames || !off_out || n_clips < 1 || n_clips > 65535u) return WSA_ERR_INVALID;
    std::vector<wsa::PcmClipDesc> desc; std::vector<uint64_t> off;
    const std::string why = wsa::pcm_plan_channels(n_clips, n_frames, formats, channels, select, source, desc, off);
    if (!why.empty()) {
        if (err && err_cap) { const size_t k = std::min<size_t>(why.size(), err_cap - 1u); std::memcpy(err, why.data(), k); err[k] = 0; }
        return WSA_ERR_INVALID;
    }
    for (uint32_t i = 0; i <= n_clips; i++) off_out[i] = off[i];
    if (!out) return WSA_OK;
    if (stride < 1 || stride > (1u << 26) || off[n_clips] > (1ull << 32)) return WSA_ERR_INVALID;
    uint32_t max_frames = 0;
    uint64_t need = 0;                                             // the last byte any source's frames reach
    for (uint32_t i = 0; i < n_clips; i++) {
        if (n_frames[i] > stride) return WSA_ERR_INVALID;
        if (n_frames[i] > max_frames) max_frames = n_frames[i];
        if (desc[i].source == i) need = std::max<uint64_t>(need, desc[i].offset + (uint64_t)n_frames[i] * desc[i].channels * wsa::pcm_sample_bytes(desc[i].format));
    }
    if (need > packed_bytes || (packed_bytes && !packed)) return WSA_ERR_INVALID;
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    wsa::DevArena A; uint8_t* dp = nullptr; wsa::PcmClipDesc* dd = nullptr; float* dout = nullptr;
    const size_t nout = (size_t)n_clips * stride;
    bool ok = A.alloc(&dp, (size_t)packed_bytes + 1) && put(dp, static_cast<const uint8_t*>(packed), (size_t)packed_bytes) && A.upload(&dd, desc) && up(A, &dout, out, nout);
    if (ok) {
        wsa::launch_batch_deinterleave(dp, dd, n_clips, max_frames, dout, stride, nullptr);
        ok = ran() && down(out, dout, nout);
    }
    return ok ? WSA_OK : WSA_ERR_HIP;
}

// K0 (csrc/resample.hip) on its own, no front end behind it: host clips in [n_clips][stride_in] through ONE form of the batch rate converter.
//   form 0: resample_kernel, every clip at fs_in[0] (all rates equal); S, J, chunks > 0 override the launch shape as WSA_RS_S / WSA_RS_J / WSA_RS_C do (0: default)
//        1: resample_mixed_kernel, one launch per rate class         2: the mixed kernel as one launch over the whole work list          (1, 2: no overrides)
// The device copy of `in` starts offset_bytes (0, 4, 8 or 12) behind a 16-byte boundary; every byte of that buffer outside the copy holds `fill`.
// out [n_clips][stride_out] goes to the device as the caller filled it and comes back as the kernel left it; n_out [n_clips] = resample_length per clip;
// plan [plan_cap][6] = per rate class {S, J, span, block, lds bytes, copy} in the classes' order (form 0: one class), shape3 = {classes, the block and the
// LDS bytes of form 2's launch (forms 0, 1: of the largest class)}.  The shape comes from resample_shape / plan_resample_mixed, the launches are
// launch_resample / launch_resample_mixed: the product's own.  Refused, nothing launched: an S outside 1 .. 512, a negative J or chunks, a launch whose
// LDS exceeds the device's limit per block, rates that are not positive and finite, a clip or its conversion longer than its row, too few plan rows.
extern "C" int wsa_debug_resample(int32_t device, const float* in, uint32_t n_clips, uint64_t stride_in, uint32_t offset_bytes, uint32_t fill, const uint32_t* n_in,
                                  const double* fs_in, double fs_out, int32_t form, int32_t S, int32_t J, int32_t chunks, float* out, uint64_t stride_out,
                                  uint32_t* n_out, int32_t* plan, uint32_t plan_cap, uint32_t* shape3) {
    using namespace wsa;
    if (!in || !n_in || !fs_in || !out || !n_out || !plan || !shape3 || n_clips < 1 || n_clips > (1u << 16) || form < 0 || form > 2) return WSA_ERR_INVALID;
    if ((offset_bytes & 3u) || offset_bytes > 12 || stride_in < 1 || stride_out < 1 || stride_in > (1ull << 28) || stride_out > (1ull << 28)) return WSA_ERR_INVALID;
    if (S < 0 || S > 512 || J < 0 || J > (1 << 16) || chunks < 0 || chunks > (1 << 16) || (form != 0 && (S || J || chunks))) return WSA_ERR_INVALID;
    if (!(fs_out > 0) || !std::isfinite(fs_out)) return WSA_ERR_INVALID;
    std::vector<uint32_t> len_in(n_in, n_in + n_clips), len_out(n_clips);
    uint64_t max_out = 0;
    for (uint32_t i = 0; i < n_clips; i++) {
        if (!(fs_in[i] > 0) || !std::isfinite(fs_in[i]) || (form == 0 && fs_in[i] != fs_in[0]) || n_in[i] > stride_in) return WSA_ERR_INVALID;
        const uint64_t n = resample_length(n_in[i], fs_in[i], fs_out);
        if (n > stride_out) return WSA_ERR_INVALID;
        len_out[i] = (uint32_t)n;
        if (n > max_out) max_out = n;
    }
    if (hipSetDevice(device) != hipSuccess) return WSA_ERR_NO_DEVICE;
    int lds_limit = 0;
    if (hipDeviceGetAttribute(&lds_limit, hipDeviceAttributeMaxSharedMemoryPerBlock, device) != hipSuccess) return WSA_ERR_HIP;
    RsParams r{}; RsMixedPlan P; std::string err;
    uint32_t n_cls = 1;
    if (form == 0) {
        resample_shape(fs_in[0], fs_out, S, J, chunks, r);
        if (resample_lds(r) > (size_t)lds_limit || (uint64_t)r.S * (uint64_t)r.J * (uint64_t)r.chunks > 0x7fffffffull) return WSA_ERR_INVALID;
        if (plan_cap < 1) return WSA_ERR_INVALID;
        const int32_t row[6] = {r.S, r.J, r.span, (int32_t)resample_block(r), (int32_t)resample_lds(r), 0};
        memcpy(plan, row, sizeof(row));
        shape3[0] = 1; shape3[1] = resample_block(r); shape3[2] = (uint32_t)resample_lds(r);
    } else {
        if (!plan_resample_mixed(n_clips, len_out.data(), fs_in, fs_out, P, err)) return WSA_ERR_INVALID;
        n_cls = (uint32_t)P.cls.size();
        if (P.max_lds > (uint32_t)lds_limit || P.max_block > 512 || plan_cap < n_cls) return WSA_ERR_INVALID;
        for (uint32_t c = 0; c < n_cls; c++) {
            const int32_t row[6] = {P.cls[c].S, P.cls[c].J, P.cls[c].span, (int32_t)P.block[c], (int32_t)P.lds[c], P.cls[c].copy};
            memcpy(plan + (size_t)c * 6, row, sizeof(row));
        }
        shape3[0] = n_cls; shape3[1] = P.max_block; shape3[2] = P.max_lds;
    }
    memcpy(n_out, len_out.data(), (size_t)n_clips * sizeof(uint32_t));
    const size_t words_in = (size_t)n_clips * stride_in, words_out = (size_t)n_clips * stride_out;
    std::vector<uint32_t> padded(words_in + 8, fill);                       // 4 words in front of the clips (the offset) and 4 behind
    const size_t first = offset_bytes / 4;
    memcpy(padded.data() + first, in, words_in * sizeof(float));
    DevArena A; uint32_t *d_in = nullptr, *d_nin = nullptr, *d_nout = nullptr, *d_clip_class = nullptr; float *d_out = nullptr, *d_table = nullptr;
    RsClass* d_cls = nullptr; RsWork* d_work = nullptr;
    bool ok = A.upload(&d_in, padded) && A.upload(&d_nin, len_in) && A.upload(&d_nout, len_out) && A.alloc(&d_out, words_out + 4) && put(d_out, out, words_out);
    if (ok && form == 0) {
        std::vector<float> K0, K; build_resample_table(fs_in[0], fs_out, K0); resample_table_image(K0, K);
        ok = A.upload(&d_table, K);
    } else if (ok) {
        ok = A.upload(&d_table, P.tables) && A.upload(&d_cls, P.cls) && A.upload(&d_clip_class, P.clip_class) && A.upload(&d_work, P.work);
    }
    if (!ok) return WSA_ERR_HIP;
    const float* base = reinterpret_cast<const float*>(d_in) + first;
    if (form == 0) {
        r.in = base; r.stride_in = stride_in; r.out = d_out; r.stride_out = stride_out; r.n_in = d_nin; r.n_out = d_nout; r.table = d_table;
        launch_resample(r, n_clips, max_out, nullptr);
    } else {
        RsMixedParams m; m.in = base; m.stride_in = stride_in; m.out = d_out; m.stride_out = stride_out; m.n_in = d_nin; m.n_out = d_nout;
        m.tables = d_table; m.cls = d_cls; m.clip_class = d_clip_class; m.work = d_work;
        launch_resample_mixed(m, P, form == 1, nullptr);
    }
    ok = ran() && down(out, d_out, words_out);
    return ok ? WSA_OK : WSA_ERR_HIP;
}
