// tracker_finalize.hpp — the end of a span: the result part of finalize O(e) (ref @B27190-28506) — get_ranked_formants, straighten, sep_syllables, the
// feature rows — or the level-3 export of the raw tracks.  Included by tracker.hip behind its constants, Ws, SpanState and OneLds.
// Used by: every tracker kernel but tracker_kernel_pair_acc / tracker_kernel_quad_acc (which leave a header per span for tracker_kernel_finalize); every
// piece takes (p, sp, L, lane) — the kernel's parameters, the span's state, the LDS block and the lane — and none knows which kernel it runs in.
#pragma once

namespace wsa {

// rows go to a pool in completion order; K3 (compaction) restores (clip, segment, syllable) order
__device__ __forceinline__ long long take_rows(const TrParams& p, SpanState& sp, int lane, int n) {
    uint32_t r0 = 0;
    if (lane == 0) r0 = atomicAdd(&p.clip_rows[sp.clip], (uint32_t)n);      // one counter per clip: no two waves queue up on it
    r0 = (uint32_t)read_lane_i32((int)r0, 0);
    if ((uint64_t)r0 + (uint32_t)n > p.row_cap) { sp.overflow = true; return -1; }
    return (long long)sp.clip * p.row_cap + r0;
}
// ---- get_ranked_formants (ref @B35670) and the slot assignment of straighten_formants (ref @B35074), once for the LDS finalize, the generic finalize
//      and the level-3 export: the three differ in where the scratch lives (the pointers) and in what they keep per track (the callbacks).
// qualify: count >= 2 and mean bin >= 7, in track order; clear(t) runs for every track; returns the number of qualified tracks
template <typename Clear>
__device__ __forceinline__ int qualify_tracks(const Ws& W, int n_tr, int lane, double* qmb, int32_t* qt, Clear&& clear) {
    int nq = 0;
    for (int base = 0; base < n_tr; base += 64) {
        const int t = base + lane;
        bool q = false; double mb = 0;
        if (t < n_tr) {
            clear(t);
            const int tl = W.tr_len[t]; const double sb = W.tr_sumEbin[t], se = W.tr_sumE[t];      // one round trip, not two
            if (tl >= 2) { mb = sb / se; q = mb >= 7; }
        }
        const uint64_t mask = __ballot(q);
        if (q) { const int pos = nq + __popcll(mask & lanemask_lt(lane)); qmb[pos] = mb; qt[pos] = t; }
        nq += __popcll(mask);
    }
    return nq;
}
// rank: stable ascending by mean bin; put(rank, qi) for every qualified track qi
template <typename Put>
__device__ __forceinline__ void rank_tracks(int nq, const double* qmb, int lane, Put&& put) {
    for (int base = 0; base < nq; base += 64) {
        const int qi = base + lane;
        if (qi < nq) {
            const double mb = qmb[qi];
            int rank = 0;
            for (int u = 0; u < nq; u++) { const double o = qmb[u]; rank += (o < mb || (o == mb && u < qi)) ? 1 : 0; }
            put(rank, qi);
        }
    }
}
// slot assignment (ref @B35074, first loop header): walking the ranked tracks, `if |mb - last| > 20: last = mb, slot++, stop at slot 3`.  Lane = rank,
// each jump found by a ballot: one lane walking the ranks was a chain of three dependent global loads per rank wherever the ranking scratch does not
// fit LDS (a 266-frame segment has ~180 qualified tracks: 0.4 ms of its finalize).  key(t, rank << 2 | slot) for every track that takes part — ONE
// word, so that a point needs one gather, not two; returns how many take part (= ranks 0 .. n - 1)
template <typename Key>
__device__ __forceinline__ int assign_slots(int nq, const double* qmb, const int32_t* qt, const int32_t* srt, int lane, Key&& key) {
    int n_part = 0;
    double last = 0; int slot = 0; bool stopped = false;
    for (int base = 0; base < nq && !stopped; base += 64) {
        const int r = base + lane;
        double mb = 0; int t = 0;
        if (r < nq) { const int qi = srt[r]; mb = qmb[qi]; t = qt[qi]; }
        uint64_t todo = __ballot(r < nq);
        int myslot = -1;
        while (todo) {
            const uint64_t jm = __ballot(((todo >> lane) & 1ull) && fabs(mb - last) > 20);
            if (jm == 0ull) { if ((todo >> lane) & 1ull) myslot = slot; break; }
            const int j = __ffsll((long long)jm) - 1;
            if (((todo >> lane) & 1ull) && lane < j) myslot = slot;
            last = read_lane_f64(mb, j);
            slot++;
            if (slot >= 3) { stopped = true; break; }
            todo &= ~lanemask_lt(j);
        }
        if (myslot >= 0) key(t, (r << 2) | myslot);
        n_part += __popcll(__ballot(myslot >= 0));
    }
    return n_part;
}
// ---- a point of a processed track filed at an index >= len makes the reference throw (r[d] undefined, ref @B35484): segments_ci keeps the entry,
//      nothing else is stored.  Looks at the points filed under len .. c_ci + 1 (by_index) and at the first frame's where its stale index is that late
template <typename Part>
__device__ __forceinline__ bool files_past_the_end(const SpanState& sp, int lane, bool by_index, Part&& takes_part) {
    bool bad = false;
    for (int base = sp.len; base <= (by_index ? sp.c_ci + 1 : -1); base += 64) {
        const int d = base + lane;
        if (d <= sp.c_ci + 1 && sp.W.d_gen[d] == sp.gen)
            for (int q = sp.W.d_p0[d]; q < sp.W.d_p1[d]; q++) if (takes_part(q)) bad = true;
    }
    if (sp.stale_d >= sp.len && lane == 0)
        for (int q = 0; q < sp.stale_p1; q++) if (takes_part(q)) bad = true;
    return bad;
}
// ---- straighten body as a selection loop, lane = frame index d: the frame's points — those filed under d and, where d is the stale index, the first
//      frame's — are applied in (track rank, arrival) order by taking the smallest key above the last one over and over.  key_of(q): the point's
//      place in that order (Key: int or long long), negative when its track takes no part; point(q, l, f, wd, E): its slot, bin, width and band energy
template <typename Key, typename KeyOf, typename Point>
__device__ __forceinline__ void straighten_select(const TrParams& p, const SpanState& sp, int lane, float* fr, float* smv, KeyOf&& key_of, Point&& point) {
    for (int base = 0; base < ((WSA_TUNE(DBG_NO_STRAIGHTEN)) ? 0 : sp.len); base += 64) {
        const int d = base + lane;
        if (d < sp.len) {
            float f9[9];
#pragma unroll
            for (int q = 0; q < 9; q++) f9[q] = 0.f;
            float sm = 0.f;
            const int a1 = (sp.stale_d == d) ? sp.stale_p1 : 0;
            const int dg = sp.W.d_gen[d], dp0 = sp.W.d_p0[d], dp1 = sp.W.d_p1[d];                         // one round trip, not two
            const bool has_main = dg == sp.gen;
            const int b0 = has_main ? dp0 : 0, b1 = has_main ? dp1 : 0;
            Key last_key = -1;
            for (;;) {
                Key best_key = sizeof(Key) == 4 ? (Key)0x7fffffff : (Key)0x7fffffffffffffffLL; int best_q = -1;
                for (int part = 0; part < 2; part++) {
                    const int q0 = part ? b0 : 0, q1 = part ? b1 : a1;
                    for (int q = q0; q < q1; q++) {
                        const Key key = key_of(q);
                        if (key > last_key && key < best_key) { best_key = key; best_q = q; }
                    }
                }
                if (best_q < 0) break;
                last_key = best_key;
                int l; double f, wd, E;
                point(best_q, l, f, wd, E);
                const float cur = l == 0 ? f9[0] : (l == 1 ? f9[3] : f9[6]);
                if ((double)cur > sp.floor_ && (double)cur < f && l < 2) l++;
                const float ff = (float)f, Ef = (float)E, wf = (float)wd;
                if (l == 0) { f9[0] = ff; f9[1] = Ef; f9[2] = wf; }
                else if (l == 1) { f9[3] = ff; f9[4] = Ef; f9[5] = wf; }
                else { f9[6] = ff; f9[7] = Ef; f9[8] = wf; }
                sm = (float)((double)sm + E);
            }
#pragma unroll
            for (int q = 0; q < 9; q++) fr[9 * d + q] = f9[q];
            smv[d] = sm;
        }
    }
}
// ---- the row and segment write-out behind straighten: levels 4 / 10 hand out the straightened frames themselves (ref @B28124, @B27713): the segment's
//      [len][9] fp32 frames go to formants[frame_off[clip] + start + d] (segments never overlap); levels 4 / 5 one row per segment; levels 10 / 13
//      sep_syllables (ref @B34757), then one feature row per syllable.  features(frames, n, x) fills a row's 53 numbers.
//      LANES: lane k keeps syllable k (the 65th and later ones of a very long segment go through the global scratch); else all go through it.
template <bool LANES, typename Feat>
__device__ __forceinline__ void write_rows(const TrParams& p, SpanState& sp, int lane, const float* fr, const float* smv, Feat&& features) {
    if (p.formants && (p.level == 4 || p.level == 10)) {
        // (frame index & ring_mask: a batch's mask is all ones, a stream keeps the frames in its ring like the frame records)
        for (int q = lane; q < 9 * sp.len; q += 64) { const int d = q / 9; p.formants[((uint64_t)sp.foff + (((uint32_t)sp.start + (uint32_t)d) & p.ring_mask)) * 9 + (uint32_t)(q - 9 * d)] = fr[q]; }
        if (p.sums) { for (int q = lane; q < sp.len; q += 64) p.sums[(uint64_t)sp.foff + (((uint32_t)sp.start + (uint32_t)q) & p.ring_mask)] = smv[q]; }
    }
    double accS, accC; sp.totals(accS, accC);
    const double cs = accC / accS;
    const double lg_ctx = jsm::log10(sp.ctx_max);
    if (p.level == 4 || p.level == 5) {
        const long long r0 = take_rows(p, sp, lane, 1);
        if (r0 < 0) return;
        double* x = p.row_feat + (uint64_t)r0 * WSA_NFEAT;
        if (WSA_TUNE(DBG_CYCLES)) sp.ph[2] = __builtin_readcyclecounter();
        if (p.level == 5) {
            if (!(WSA_TUNE(DBG_NO_FEATURES))) features(fr, sp.len, x);
            if (WSA_TUNE(DBG_CYCLES)) sp.ph[3] = __builtin_readcyclecounter();
            if (lane == 0) { x[0] = sp.len; x[1] = sqrt((double)sp.len); x[2] = cs; x[3] = lg_ctx; x[4] = sp.floor_; }
        } else if (lane < WSA_NFEAT) x[lane] = 0;
        if (lane == 0) {
            int32_t* m = p.row_meta + (uint64_t)r0 * 8;
            m[0] = (int32_t)sp.clip; m[1] = 0; m[2] = 0; m[3] = 0; m[4] = sp.my_seg; m[5] = 0; m[6] = sp.start; m[7] = sp.len;
            sp.sg[SEG_FLAG] = 1; sp.sg[SEG_NROWS] = 1; sp.sg[SEG_ROW0] = (int32_t)r0;
        }
        return;
    }
    // ---- levels 10 / 13: pass 1 finds the syllables (sequential scan over the frame sums), pass 2 fills the rows
    int nsyl = 0, my_si = 0, my_sl = 0;
    {
        int si = -1, cc = 0, uu = 0;
        for (int base = 0; base < sp.len; base += 64) {
            const int dd = base + lane;
            const float smq = dd < sp.len ? smv[dd] : 0.f;
            const int lim = min(64, sp.len - base);
            for (int j = 0; j < lim; j++) {
                const int e2 = base + j;
                const double v = __builtin_bit_cast(float, read_lane_i32(__builtin_bit_cast(int, smq), j));
                if (v > sp.floor_) { cc = 0; uu++; if (si < 0) si = e2; } else cc++;
                if ((uu > 20 && cc > 0) || (uu > 10 && cc > 1) || (uu > 0 && cc > 4) || (e2 >= sp.len - 1 && uu > 4)) {
                    const int t = e2 - cc;
                    if (t - si > 1) {
                        if (LANES && nsyl < 64) { if (lane == nsyl) { my_si = si; my_sl = t - si; } }
                        else if (lane == 0) { sp.W.q_idx[2 * nsyl] = si; sp.W.q_idx[2 * nsyl + 1] = t - si; }
                        nsyl++;
                        si = -1; uu = 0;
                    }
                }
            }
        }
    }
    wsync();
    long long r0 = 0;
    if (nsyl > 0) { r0 = take_rows(p, sp, lane, nsyl); if (r0 < 0) return; }
    for (int k = 0; k < nsyl; k++) {
        const int si = LANES && k < 64 ? read_lane_i32(my_si, k) : sp.W.q_idx[2 * k], sl = LANES && k < 64 ? read_lane_i32(my_sl, k) : sp.W.q_idx[2 * k + 1];
        double* x = p.row_feat + (uint64_t)(r0 + k) * WSA_NFEAT;
        if (p.level == 13) {
            if (!(WSA_TUNE(DBG_NO_FEATURES))) features(fr + 9 * si, sl, x);
            if (lane == 0) { x[0] = sl; x[1] = sqrt((double)sl); x[2] = cs; x[3] = lg_ctx; x[4] = sp.floor_; }
        } else if (lane < WSA_NFEAT) x[lane] = 0;
        if (lane == 0) {
            int32_t* m = p.row_meta + (uint64_t)(r0 + k) * 8;
            m[0] = (int32_t)sp.clip; m[1] = 0; m[2] = si; m[3] = sl; m[4] = sp.my_seg; m[5] = k; m[6] = sp.start + si; m[7] = sl;
        }
    }
    if (lane == 0) { sp.sg[SEG_FLAG] = nsyl > 0 ? 1 : 0; sp.sg[SEG_NROWS] = nsyl; sp.sg[SEG_ROW0] = (int32_t)r0; }
}
// ---- the same finalize out of LDS (the usual case): track keys, the ranking scratch, the points of the span (key | bin | width, energy) and the straightened
//      frames all fit the block the dead active table leaves behind, every pointer below is a plain LDS pointer (ds_ instructions, no flat accesses), and the two
//      inherently sequential steps of the slow version — slot assignment and the energy-event scan — run on ballots / v_readlane.  Returns false (nothing touched)
//      when the span does not fit; finalize_generic then runs. G (third form, the batch finalize kernel only): the straightened frames do not fit the block and live
//      in the span's region of the pool (W.fr, W.sm1) — keys, ranking scratch and 4-byte points stay in LDS, straighten takes the selection loop (its slots are
//      registers, stored once per frame), the feature sums read the frames through flat loads.  Holds spans of up to ~330 frames (4.8 points per frame); what the
//      generic path cost such a span: profiles/r06_notes.md section 4.
template <int AC, bool G>
__device__ __forceinline__ bool finalize_lds(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane) {
    constexpr int BIG = OneLds<AC>::BYTES;
    const int off_u = (int)align16((size_t)2 * sp.n_tr);                           // union starts behind the track keys
    const int rank_bytes = 16 * sp.n_tr, fr_bytes = G ? 0 : (int)align16((size_t)40 * sp.len);
    const int off_pt = off_u + fr_bytes;
    // (behind the straightened frames the block also has to hold the scratch of the feature reductions: a span of more than ~130 frames takes the generic path)
    // A point costs the block 12 bytes (band energy f64 + packed bin / width / key) — or 4 where that does not fit: the energies then stay in the span's
    // region of the pool and straighten reads them from there (an 8-byte load per applied point out of lines the copy loop below has just touched).
    // At the library's 25 ms step every span of the bench batch fits the 12-byte form; at the application's 15 ms step (segments 1.67 x as long in frames)
    // 29 % of the spans did not and took the generic path in HBM, which made the finalize kernel 3.5 x as long (profiles/r06_notes.md section 4).
    const bool pe_lds = !G && off_pt + 12 * sp.n_pt <= BIG;
    const int ppb = pe_lds ? 12 : 4;
    if (sp.n_tr > 8000 || sp.n_pt > 60000 || off_u + rank_bytes > BIG || off_pt + ppb * sp.n_pt > BIG || off_pt + FEAT_SCRATCH * 8 > BIG) return false;
    int16_t* const trk_key = reinterpret_cast<int16_t*>(L.big);               // per track id: rank << 2 | slot, or -1
    double* const qmb = reinterpret_cast<double*>(L.big + off_u);              // ranking scratch (dies before fr / points are written)
    int32_t* const qt = reinterpret_cast<int32_t*>(L.big + off_u + 8 * sp.n_tr);
    int32_t* const srt = qt + sp.n_tr;
    float* const fr = G ? sp.W.fr : reinterpret_cast<float*>(L.big + off_u);      // [len][9]
    float* const smv = G ? sp.W.sm1 : fr + 9 * sp.len;                               // [len]
    double* const pE = reinterpret_cast<double*>(L.big + off_pt);              // [n_pt] band energy (pe_lds)
    uint32_t* const pkb = reinterpret_cast<uint32_t*>(L.big + off_pt + (pe_lds ? 8 * sp.n_pt : 0));      // [n_pt] bin | width << 8 | key15 << 17 (0x7fff: no part)
    auto energy_of = [&](int q) __attribute__((always_inline)) -> double { return pe_lds ? pE[q] : reinterpret_cast<const double*>(sp.W.pt + q)[1]; };      // (a point record's .z / .w are the f64's words)
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[0] = sp.ph[1] = sp.ph[2] = sp.ph[3] = __builtin_readcyclecounter();
    const int nq = qualify_tracks(sp.W, sp.n_tr, lane, qmb, qt, [&](int t) __attribute__((always_inline)) { trk_key[t] = -1; });
    wsync();
    rank_tracks(nq, qmb, lane, [&](int rank, int qi) __attribute__((always_inline)) { srt[rank] = qi; });
    wsync();
    const int n_part = assign_slots(nq, qmb, qt, srt, lane, [&](int t, int key) __attribute__((always_inline)) { trk_key[t] = (int16_t)key; });      // ranked tracks that got a slot = ranks 0 .. n_part - 1
    wsync();
    // ---- straighten applies a frame's points in (track rank, arrival) order.  The tracks that take part are the first n_part of the ranking (the slot walk above
    //      stops at the fourth jump), and a track files at most one point per index — except that the span's first frame is usually filed under a stale index (quirk
    //      1), which a later frame may carry as well: its points get a row of their own.  So the points go into a table [filing index][rank] (the filing index
    //      travels in the point record) next to a 64-bit map of the ranks present per index, and a frame's lane walks the set bits of its map instead of searching
    //      its points for the next key over and over (the selection loop below).  More than 64 ranks or no room in the block: the selection loop.
    const int off_tbl = (int)align16((size_t)off_pt + (size_t)ppb * (size_t)sp.n_pt);
    const int tbl_bytes = 4 * (sp.len + 1) + 2 * (sp.len + 1) * n_part;
    const bool use_tbl = !G && n_part <= 32 && sp.c_ci + 1 < 0x7fff && sp.stale_d < 0x7fff && off_tbl + tbl_bytes <= BIG && !(p.dbg & DBG_SELECT_LOOP);
    uint32_t* const tblm = reinterpret_cast<uint32_t*>(L.big + off_tbl);                         // [len + 1]: ranks present at index d (32 of them: more take the selection loop); [len]: in the stale row
    uint16_t* const tbl = reinterpret_cast<uint16_t*>(tblm + sp.len + 1);                           // [len + 1][n_part]: point index + 1; row len = the stale row
    if (use_tbl) for (int q = lane; q <= sp.len; q += 64) tblm[q] = 0u;
    wsync();
    // ---- the points of the span move into LDS with their application key: (rank of the track) << 2 | slot
    bool bad = false;
    {
        int4 nxt4 = lane < sp.n_pt ? sp.W.pt[lane] : make_int4(0, 0, 0, 0);
        for (int q = lane; q < sp.n_pt; q += 64) {
            const int4 rec4 = nxt4;
            if (q + 64 < sp.n_pt) nxt4 = sp.W.pt[q + 64];
            const int key = trk_key[rec4.x];
            if (pe_lds) pE[q] = __hiloint2double(rec4.w, rec4.z);
            pkb[q] = ((uint32_t)rec4.y & 0x1ffffu) | ((key < 0 ? 0x7fffu : (uint32_t)key) << 17);
            if (use_tbl && key >= 0) {
                const int d = (int)((uint32_t)rec4.y >> 17);
                // a point of a processed track filed at an index >= len makes the reference throw (below)
                if (d >= sp.len) bad = true;
                else {
                    const int row = (q < sp.stale_p1 && sp.stale_d >= 0) ? sp.len : d;        // the first frame's points when it was filed under a stale index
                    tbl[row * n_part + (key >> 2)] = (uint16_t)(q + 1);
                    atomicOr(&tblm[row], 1u << (key >> 2));
                }
            }
        }
    }
    wsync();
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[0] = __builtin_readcyclecounter();
    if (files_past_the_end(sp, lane, !use_tbl, [&](int q) __attribute__((always_inline)) { return (pkb[q] >> 17) != 0x7fffu; })) bad = true;      // (with the table, the copy loop above has looked at the filing indices)
    if (__ballot(bad) != 0ull) { if (lane == 0) { sp.sg[SEG_FLAG] = -1; sp.sg[SEG_NROWS] = 0; } return true; }
    // ---- straighten body, lane = frame index d: apply this frame's points in (track rank, arrival) order
    if (use_tbl) {
        const uint32_t stale_m = tblm[sp.len];
        // The slots live in the frame's row of `fr` (LDS) while the points are applied: a point reads the one float it compares with and writes its
        // three — the nine selects of a register copy cost more than the round trip.  The slots hold bins (small integers, or 0) as floats, so the
        // reference's `cur > floor && cur < f` (f64) is decided in fp32: cur > floor <=> cur >= floor(floor) + 1 (clamped to 256: no bin reaches it;
        // a negative floor admits every bin, -0 admits cur > 0; a NaN floor admits none, as there), cur < f exactly.
        float thr_f;
        { const double t0 = sp.floor_ < 0 ? 0.0 : floor(sp.floor_) + 1.0; thr_f = (float)(t0 > 256.0 ? 256.0 : t0); }
        for (int base = 0; base < ((WSA_TUNE(DBG_NO_STRAIGHTEN)) ? 0 : sp.len); base += 64) {
            const int d = base + lane;
            float* const row = fr + 9 * (d < sp.len ? d : 0);
            if (d < sp.len) {
#pragma unroll
                for (int q = 0; q < 9; q++) row[q] = 0.f;
            }
            float sm = 0.f;
            auto apply = [&](int q) __attribute__((always_inline)) {
                const uint32_t w = pkb[q];
                int l = (int)((w >> 17) & 3u);
                const double E = energy_of(q);
                const float ff = (float)(w & 0xffu), cur = row[3 * l];
                if (cur >= thr_f && cur < ff && l < 2) l++;
                row[3 * l] = ff; row[3 * l + 1] = (float)E; row[3 * l + 2] = (float)((w >> 8) & 0x1ffu);
                sm = (float)((double)sm + E);
            };
            const uint32_t m_main = d < sp.len ? tblm[d] : 0u, m_st = (d < sp.len && d == sp.stale_d) ? stale_m : 0u;
            uint32_t mm = m_main | m_st;
            while (mm) {                                   // ranks in ascending order; of one rank the stale frame's point first (it arrived first)
                const int r = __ffs((int)mm) - 1; mm &= mm - 1u;
                if ((m_st >> r) & 1u) apply((int)tbl[sp.len * n_part + r] - 1);
                if ((m_main >> r) & 1u) apply((int)tbl[d * n_part + r] - 1);
            }
            if (d < sp.len) smv[d] = sm;
        }
    } else
    straighten_select<int>(p, sp, lane, fr, smv,      // key: rank << 16 | arrival
        [&](int q) __attribute__((always_inline)) -> int { const uint32_t w = pkb[q]; return (w >> 17) == 0x7fffu ? -1 : (int)(((w >> 19) << 16) | (uint32_t)q); },
        [&](int q, int& l, double& f, double& wd, double& E) __attribute__((always_inline)) {
            const uint32_t w = pkb[q];
            l = (int)((w >> 17) & 3u); f = w & 0xffu; wd = (w >> 8) & 0x1ffu; E = energy_of(q);
        });
    wsync();
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[1] = __builtin_readcyclecounter();
    // scratch of the feature reductions: what the points and the straighten table occupied (dead by now), when it is large enough
    double* const red = reinterpret_cast<double*>(L.big + off_pt);
    write_rows<true>(p, sp, lane, fr, smv, [&](const float* f, int n, double* x) __attribute__((always_inline)) {
        formant_features_lds(f, n, sp.ctx_max, x, lane, red, !G && n <= 15 && !(p.dbg & DBG_NO_PACKED_COLUMNS), G || (p.dbg & DBG_EVENTS_BLOCK) != 0);
    });
    return true;
}
// ---- the generic finalize through the span's work space in HBM: any span, however many tracks, points and frames
template <int AC>
__device__ __forceinline__ void finalize_generic(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane) {
    constexpr int FRCAP = OneLds<AC>::FRCAP;
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[0] = sp.ph[1] = sp.ph[2] = sp.ph[3] = __builtin_readcyclecounter();
    const int nq = qualify_tracks(sp.W, sp.n_tr, lane, sp.W.q_mb, sp.W.q_idx, [&](int t) __attribute__((always_inline)) { sp.W.tr_slot[t] = -1; });
    wsync();
    // ranking scratch: LDS when the qualified tracks fit (they almost always do), else the
    // global arrays; generic pointers serve both
    const bool q_lds = nq <= AC;
    double* qmb = sp.W.q_mb; int32_t* qidx = sp.W.q_idx; int32_t* sorted = sp.W.sorted;
    if (q_lds) {
        for (int qi = lane; qi < nq; qi += 64) { L.f_qmb[qi] = sp.W.q_mb[qi]; L.f_qidx[qi] = sp.W.q_idx[qi]; }
        qmb = L.f_qmb; qidx = L.f_qidx; sorted = L.f_sorted;
        wsync();
    }
    rank_tracks(nq, qmb, lane, [&](int rank, int qi) __attribute__((always_inline)) { sorted[rank] = qi; });
    wsync();
    assign_slots(nq, qmb, qidx, sorted, lane, [&](int t, int key) __attribute__((always_inline)) { sp.W.tr_slot[t] = key; });
    wsync();
    // every point gets its application key once: (rank of its track) << 2 | slot, or -1 when the
    // track takes no part (lane = point; the frame lanes below then read keys, not track tables); the next round's track ids are on their way
    // while this round's keys are gathered
    {
        int t_nxt = lane < sp.n_pt ? sp.W.pt[lane].x : 0;
        for (int q = lane; q < sp.n_pt; q += 64) {
            const int t = t_nxt;
            if (q + 64 < sp.n_pt) t_nxt = sp.W.pt[q + 64].x;
            sp.W.pt_key[q] = sp.W.tr_slot[t];
        }
    }
    wsync();
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[0] = __builtin_readcyclecounter();
    if (__ballot(files_past_the_end(sp, lane, true, [&](int q) __attribute__((always_inline)) { return sp.W.pt_key[q] >= 0; })) != 0ull) { if (lane == 0) { sp.sg[SEG_FLAG] = -1; sp.sg[SEG_NROWS] = 0; } return; }
    // ---- straighten body, lane = frame index d: apply this frame's points in
    //      (track rank, arrival) order
    // the q_* scratch is dead from here on; fr / sm of the segment go to LDS when they fit
    float* const fr = sp.len <= FRCAP ? L.f_fr : sp.W.fr;
    float* const smv_ = sp.len <= FRCAP ? L.f_sm : sp.W.sm1;
    // the features of a span whose frames live in HBM (more frames than the block holds): the block is free then, and the wave-parallel reductions of the
    // LDS path run on it with the frames read through flat loads — formant_features_wave walks the energy events frame by frame on ONE lane, a dependent
    // global round trip per frame, which made a 266-frame segment's finalize 600 us and with it the whole kernel (the application's settings at 48 kHz)
    // (formant_features_lds takes at most FEAT_LDS_MAX frames: longer spans and syllables keep the frame-by-frame walk, which has no limit)
    auto features = [&](const float* f, int a, double* x) __attribute__((always_inline)) {
        if (sp.len > FRCAP && a <= FEAT_LDS_MAX) formant_features_lds(f, a, sp.ctx_max, x, lane, reinterpret_cast<double*>(L.big), false, true);
        else formant_features_wave(f, a, sp.ctx_max, x, sp.W.Aev, sp.aev_stride, lane);
    };
    straighten_select<long long>(p, sp, lane, fr, smv_,
        [&](int q) __attribute__((always_inline)) -> long long { const int pk = sp.W.pt_key[q]; return pk < 0 ? -1LL : (long long)(pk >> 2) * (long long)(p.pcap + 1) + q; },
        [&](int q, int& l, double& f, double& wd, double& E) __attribute__((always_inline)) {
            l = sp.W.pt_key[q] & 3;
            const int4 rec4 = sp.W.pt[q];
            f = rec4.y & 0xff; wd = (rec4.y >> 8) & 0x1ff; E = __hiloint2double(rec4.w, rec4.z);
        });
    wsync();
    if (WSA_TUNE(DBG_CYCLES)) sp.ph[1] = __builtin_readcyclecounter();
    write_rows<false>(p, sp, lane, fr, smv_, features);
}
// ---- level 3 hands out the ranked raw tracks themselves (ref @B28273 `s.push(i)`, i = get_ranked_formants() @B35670):
//      the span's points (arrival order) and the ranked track ids go to a pool behind the span's first frame
//      (a frame brings at most MAXC points / tracks); the host rebuilds the 18-field records from them.
//      ring: the pool's slots are a stream's ring (tracker_kernel_stream_raw), not a batch's frames (tracker_kernel_raw)
__device__ __forceinline__ void export_raw_tracks(const TrParams& p, SpanState& sp, int lane, bool ring) {
    const int nq = qualify_tracks(sp.W, sp.n_tr, lane, sp.W.q_mb, sp.W.q_idx, [](int) __attribute__((always_inline)) {});
    wsync();
    // batch: the pool entries of a span start behind its first frame's slot.  Streams: the slots are the stream's ring, so the
    // entries run modulo the ring (the host unwraps them, wsa_stream_collect); the span's first frame is what the gate noted
    const uint64_t pbase = (uint64_t)sp.foff * MAXC;
    const uint64_t pmask = ring ? (uint64_t)(p.ring_mask + 1u) * MAXC - 1ull : ~0ull;
    const uint64_t poff = (ring ? (uint64_t)((uint32_t)sp.sg[SEG_FBEGIN] & p.ring_mask) : (uint64_t)sp.f_begin) * MAXC;
    const uint64_t pool0 = pbase + poff;
    auto slot = [&](uint64_t q) __attribute__((always_inline)) -> uint64_t { return pbase + ((poff + q) & pmask); };
    rank_tracks(nq, sp.W.q_mb, lane, [&](int rank, int qi) __attribute__((always_inline)) { p.trk_rank[slot((uint64_t)rank)] = sp.W.q_idx[qi]; });
    for (int q = lane; q < sp.n_pt; q += 64) { int4 v = sp.W.pt[q]; v.y &= 0x1ffff; p.trk_pts[2 * slot((uint64_t)q)] = v; p.trk_pts[2 * slot((uint64_t)q) + 1] = sp.W.ptx[q]; }   // (the filing index also sits in ptx.z)
    if (lane == 0) {
        int32_t* ts = p.trk_seg + ((uint64_t)sp.clip * p.seg_cap + sp.my_seg) * 4;
        ts[0] = (int32_t)(pool0 & 0xffffffffu); ts[1] = sp.n_pt; ts[2] = nq; ts[3] = (int32_t)(pool0 >> 32);
    }
}
// ---- end of a span: the live tracks hand their summaries over, then the result part of finalize (or the level-3 export).
//      THIRD: the finalize kernel's third LDS form exists (its spans' regions of the pool hold their straightened frames)
template <int AC, bool RAW, bool THIRD>
__device__ __forceinline__ void finish_span(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane, bool ring = false) {
    // tracks still in the table hand their summaries over as well (the group kernels and the finalize kernel come with an empty table: n_act = 0)
    for (int j = lane; j < sp.n_act; j += 64) { const int gi = L.a_gid[j]; sp.W.tr_len[gi] = L.a_len[j]; sp.W.tr_sumE[gi] = L.a_sumE[j]; sp.W.tr_sumEbin[gi] = L.a_sumEbin[j]; }
    wsync();
    if constexpr (RAW) export_raw_tracks(p, sp, lane, ring);
    else if (!(WSA_TUNE(DBG_NO_FINALIZE))) {
        if (!(p.dbg & DBG_GENERIC_FINALIZE)) {
            if (finalize_lds<AC, false>(p, sp, L, lane)) return;
            if constexpr (THIRD) { if (!(p.dbg & DBG_NO_THIRD_FORM) && finalize_lds<AC, true>(p, sp, L, lane)) return; }
        }
        finalize_generic<AC>(p, sp, L, lane);
    }
}
// ---- tracker_kernel_finalize: the span's state comes from the header tracker_kernel_pair_acc / quad_acc left (write_span_headers, tracker_group.hpp),
//      its tracks and points from its region of the pool
template <int AC>
__device__ __forceinline__ void finalize_from_header(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane) {
    const double* hd = p.span_hdr + ((uint64_t)sp.clip * p.seg_cap + (uint32_t)sp.my_seg) * 8;
    const double h0 = hd[0], h1 = hd[1], h2 = hd[2], h3 = hd[3], h4 = hd[4], h5 = hd[5], h6 = hd[6];
    const int flag = (int)h6;
    if (flag == 0) return;                                              // on the redo list: the one-span kernel does the whole span
    if (flag & 2) { if (lane == 0) atomicOr(&p.shared[1], 1u); return; }
    const int F = (int)(sp.f_end - sp.f_begin);
    sp.W = carve_ws(p.pool + (uint64_t)(sp.foff + sp.f_begin) * p.pool_bpf, MAXC * F, MAXC * F, F, 0, nullptr);
    sp.aev_stride = F + 2;
    sp.n_tr = (int)h0; sp.n_pt = (int)h1; sp.n_act = 0; sp.stale_d = (int)h2; sp.stale_p1 = (int)h3;
    sp.accG = h4; sp.accL = lane == 0 ? h5 : 0.0;
    sp.gen = 1;
    const unsigned long long tf0 = WSA_TUNE(DBG_CYCLES) ? __builtin_readcyclecounter() : 0ull;
    finish_span<AC, false, true>(p, sp, L, lane);
    if (WSA_TUNE(DBG_CYCLES) && lane == 0 && p.trace) {      // tuning: per-span finalize cycles and phases into the trace buffer (tools/fin_probe.py)
        double* tr = p.trace + (uint64_t)atomicAdd(&p.shared[0], 1u) * 12;
        tr[0] = 0; tr[1] = (double)(__builtin_readcyclecounter() - tf0); tr[2] = sp.len; tr[3] = F; tr[4] = sp.n_tr; tr[5] = sp.n_pt; tr[6] = blockIdx.x;
        tr[7] = (double)(sp.ph[0] - tf0); tr[8] = (double)(sp.ph[1] - sp.ph[0]); tr[9] = (double)(sp.ph[2] - sp.ph[1]); tr[10] = (double)(sp.ph[3] - sp.ph[2]);
    }
    if (sp.overflow && lane == 0) atomicOr(&p.shared[1], 1u);
    wsync();
}

}  // namespace wsa
