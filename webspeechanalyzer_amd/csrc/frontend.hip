// frontend.hip — K1: batched PCM -> Hann window -> real FFT -> power -> mel bands -> emphasis / gain -> Uint32 frame, for gfx950 (MI355X):
// what the rest of the library calls.  The kernels are one file per FFT family — fe_r8.hip (1024 points), fe_rx.hip (other powers of two),
// fe_r3.hip (3 * 2^k) — over the stages they share (fe_stages.hpp) and the FE-1 arithmetic (fe_common.hpp).
//
// Stands in for the reference's "spectrum-processor" AudioWorklet (source not in the reference
// tree: fetched from unpkg at run time, ref dist/main.js:2 @B6480; configured @B6726; its output,
// one Uint32Array(spec_bands) per frame, is consumed @B8568).  Arithmetic = specification FE-1
// (DESIGN.md): bit-exact with oracle/frontend.c.  Compiled with -ffp-contract=off: only the
// explicit __builtin_fmaf calls fuse.
#include "fe_stages.hpp"

namespace wsa {

bool fe_supported_R(int R, int three) { return three ? (R == 1 || R == 2 || R == 4 || R == 8 || R == 16 || R == 32) : (R == 2 || R == 4 || R == 8 || R == 16 || R == 32 || R == 64); }

static FeChoice fe_select(const FeParams& p, int R, int three) { return three ? fe_select_r3(p, R) : R == 8 ? fe_select_r8(p) : fe_select_rx(p, R); }

void launch_frontend(const FeParams& p, int n_clips, int max_frames, int R, int three, hipStream_t s) {
    if (n_clips <= 0 || max_frames <= 0) return;
    const FeChoice c = fe_select(p, R, three);
    if (!c.kernel) return;
    const int frames_per_block = 4 * p.frames_per_wave;
    FeParams q = p;
    q.chunks_per_clip = (uint32_t)((max_frames + frames_per_block - 1) / frames_per_block); q.n_chunks = q.chunks_per_clip * (uint32_t)n_clips;
    dim3 grid = c.grid_2d ? dim3(q.chunks_per_clip, n_clips, 1) : dim3(q.n_chunks, 1, 1);
    // persistent launch: n_cu x WSA_FE_WGS workgroups take the chunks from the queue, where that is fewer than one workgroup per chunk
    // (p.queue is null under WSA_FE_NO_QUEUE: Tuning::fe_no_queue, read when the batch was planned)
    if (c.queue_wgs && q.queue) {
        const uint32_t want = (uint32_t)(p.n_cu > 0 ? p.n_cu : 256) * (uint32_t)(p.wg_per_cu >= 1 && p.wg_per_cu <= c.queue_wgs ? p.wg_per_cu : 2);
        if (want < q.n_chunks) grid = dim3(want, 1, 1); else q.queue = nullptr;
    } else q.queue = nullptr;
    hipLaunchKernelGGL(c.kernel, grid, dim3(256), c.lds, s, q);
}

// dynamic LDS the front-end kernel of this geometry asks for (a workgroup may have 160 KB on gfx950; wsa_batch_create / wsa_stream_create refuse settings beyond that)
static FeChoice fe_choice_of_plan(const FePlanHost& P, bool fat) {
    FeParams p{};
    p.win = P.win; p.hop = P.hop; p.kmax = P.kmax; p.bands = P.bands; p.spec_type = P.spec_type; p.mel_total = (int)P.mel_w.size();
    for (int32_t c_ : P.mel_cnt) if (c_ > p.mel_max_taps) p.mel_max_taps = c_;
    for (size_t i_ = 0; i_ < P.mel_cnt.size() && i_ < 64; i_++) if (P.mel_cnt[i_] > p.mel_max_taps_lo) p.mel_max_taps_lo = P.mel_cnt[i_];
    p.fat = fat ? 1 : 0;
    return fe_select(p, P.R, P.three);
}
size_t fe_lds_required(const FePlanHost& P, bool fat) { return fe_choice_of_plan(P, fat).lds; }
// the instantiation this geometry runs, as profiles/frontend_split.md names it ("" for an FFT length no family serves); launches nothing
const char* fe_choice_name(const FePlanHost& P, bool fat) { return fe_supported_R(P.R, P.three) ? fe_choice_of_plan(P, fat).name : ""; }

}  // namespace wsa
