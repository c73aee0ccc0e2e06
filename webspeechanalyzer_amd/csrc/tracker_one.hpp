// tracker_one.hpp — accumulate_fm (ref @B35952) for one span per wave, and its two drivers: a batch's span (64-frame blocks, entries prefetched) and a
// stream's step (state carried in HBM).  Included by tracker.hip behind tracker_finalize.hpp.
// Used by: tracker_kernel_fast / _full / _raw (track_span) and tracker_kernel_stream / _stream_raw (track_stream).
#pragma once

namespace wsa {
// ---- frames of the span.  Per frame gate.hip left: info (filing index | stale << 30, or -1 when accumulate_fm is not called), v (acceptance floor), fl (floor
// handed to accumulate_fm). Everything of frame f+1 is requested before frame f is processed. The header words are the same for all lanes, but they are loaded
// through a lane-dependent zero offset
// (vz) so that the compiler treats them as ordinary vector data: knowing them uniform it wants them in
// SGPRs the moment they are loaded (v_readfirstlane behind an s_waitcnt), which turned every header load
// into an exposed memory round trip.  They become scalars (read_first_lane_*) only where they are consumed.
struct Hdr { int info; double v, fl; uint4 h; };                 // h = the frame's record header, as loaded (decoded where it is consumed)
struct Pre { int info; double v, fl, g; int n; uint32_t pk, amp, plo, phi, hi; };
__device__ __forceinline__ void load_hdr(const TrParams& p, const SpanState& sp, int vz, uint32_t f, Hdr& q) {      // branch-free: frames past the span read its last frame
    const uint32_t fi = (min(f, sp.f_end - 1) & p.ring_mask) + (uint32_t)vz;
    q.info = p.fr_info[sp.foff + fi]; q.v = p.fr_v[sp.foff + fi]; q.fl = p.fr_fl[sp.foff + fi];
    q.h = p.rec.hdr[sp.foff + fi];
}
__device__ __forceinline__ void load_ent(const TrParams& p, const SpanState& sp, int lane, uint32_t f, const Hdr& h, Pre& q) {
    const int hy = read_first_lane_i32((int)h.h.y);
    q.info = f < sp.f_end ? read_first_lane_i32(h.info) : -1; q.v = read_first_lane_f64(h.v); q.fl = read_first_lane_f64(h.fl);
    q.g = (double)(hy & 0xff) * 4294967296.0 + (double)(uint32_t)read_first_lane_i32((int)h.h.x);      // exact: g < 2^40
    q.n = (hy >> 8) & 0xff; q.pk = q.amp = q.plo = q.phi = q.hi = 0;
    if (q.info >= 0 && lane < q.n && !(WSA_TUNE(DBG_NO_ENTRIES))) {           // only frames accumulate_fm sees, only the entries they hold
        const uint32_t c = (uint32_t)read_first_lane_i32((int)h.h.w) + (uint32_t)lane;
        const uint4 e4 = p.rec.ent[c];
        q.amp = p.rec.amp[c]; q.pk = e4.x; q.plo = e4.y; q.phi = e4.z; q.hi = e4.w;
    }
}
// ---- accumulate_fm for one frame (ref @B35952); `cur` = the frame's header words and this lane's candidate entry
// `refill` runs exactly once, as soon as this lane's candidate entry of `cur` is no longer needed (behind the compaction
// of the accepted peaks): the batch path requests a later frame's entry into the same registers there
template <int AC, bool RAW, typename Refill>
__device__ __forceinline__ void accumulate(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane, const Pre& cur, Refill&& refill) {
    const int info = cur.info;
    if (!(info >= 0 && !(WSA_TUNE(DBG_NO_ACCUMULATE)))) { refill(); return; }
    const int ncand = cur.n;
    const double g = cur.g, v = cur.v;
    const uint32_t pkw = cur.pk, amp = cur.amp;
    // exact prefix sums P[i-1], P[s] (< 2^40) from their low words and high bytes
    const double plo = (double)(cur.hi & 0xffu) * 4294967296.0 + (double)cur.plo, phi = (double)((cur.hi >> 8) & 0xffu) * 4294967296.0 + (double)cur.phi;
    const bool reset_this_frame = (info >> 30) & 1;
    const int t_idx = info & 0x3fffffff;
    // accepted peaks (ref @B25827: `e[l] > v`), lane = candidate
    const bool acc = lane < ncand && (double)amp > v;
    const uint64_t amask = __ballot(acc);
    const int n = __popcll(amask);
    if (n < 1) { refill(); return; }
    // ---- accumulate_fm(e, peaks, t_idx, g, floor_) (ref @B35952)
    sp.acp.start(WSA_TUNE(DBG_PHASES));
    const int nfile = t_idx;
    const double fl = cur.fl;
    sp.accG += g;
    // compact the accepted peaks: lane o < n owns peak o
    const int my_o = __popcll(amask & lanemask_lt(lane));
    if (acc) { L.s_pk[my_o] = pkw; L.s_amp[my_o] = amp; L.s_plo[my_o] = plo; L.s_phi[my_o] = phi; }
    refill();
    wsync();
    int pk_i = 0, pk_s = 0, pk_l = -1000; uint32_t pk_amp = 0; double pk_plo = 0, pk_phi = 0;
    if (lane < n) {
        const uint32_t w = L.s_pk[lane];
        pk_i = w & 0xff; pk_s = (w >> 8) & 0xff; pk_l = (w >> 16) & 0xff;
        pk_amp = L.s_amp[lane]; pk_plo = L.s_plo[lane]; pk_phi = L.s_phi[lane];
    }
    sp.acp.lap(WSA_TUNE(DBG_PHASES), 0);
    // 1. retire tracks whose last filing index is 4 or more behind (gap only grows); most frames retire
    //    nothing from a block of 64, which then stays as it is
    {
        int kept = 0;
        for (int base = 0; base < sp.n_act; base += 64) {
            const int j = base + lane;
            const bool valid = j < sp.n_act;
            const int lf = valid ? L.a_last_frame[j] : 0;
            const bool keep = valid && (nfile - lf) < 4;
            const uint64_t km = __ballot(keep);
            if (kept == base && km == __ballot(valid)) { kept += __popcll(km); continue; }
            int ln = 0, gi = 0; uint32_t bn = 0, am = 0; double ve = 0, se = 0, sb = 0;
            if (valid) { ln = L.a_len[j]; gi = L.a_gid[j]; bn = L.a_bins[j]; am = L.a_amp[j]; ve = L.a_vel[j]; se = L.a_sumE[j]; sb = L.a_sumEbin[j]; }
            if (valid && !keep) { sp.W.tr_len[gi] = ln; sp.W.tr_sumE[gi] = se; sp.W.tr_sumEbin[gi] = sb; }   // the summary finalize ranks by
            wsync();
            if (keep) {
                const int q = kept + __popcll(km & lanemask_lt(lane));
                L.a_last_frame[q] = lf; L.a_len[q] = ln; L.a_gid[q] = gi; L.a_bins[q] = bn; L.a_amp[q] = am; L.a_vel[q] = ve; L.a_sumE[q] = se; L.a_sumEbin[q] = sb;
            }
            kept += __popcll(km);
            wsync();
        }
        sp.n_act = kept;
    }
    sp.acp.lap(WSA_TUNE(DBG_PHASES), 1);
    // 2. score every (track, peak) pair inside the track's search window; per peak keep
    //    the best score > 1, the EARLIER track on ties (ref: `i>1&&i>d[o]` in track order)
    int asg = -1; double best = 0;
    for (int tbase = 0; tbase < sp.n_act; tbase += 64) {
        const int j = tbase + lane;
        const bool valid = j < sp.n_act;
        int gap = -1, bin = 0;
        if (valid) { gap = nfile - L.a_last_frame[j]; bin = (int)(L.a_bins[j] & 0xff); L.a_mmask[j] = 0ull; }
        const bool live = valid && gap >= 0 && gap < 4;
        const int win = gap == 0 ? 3 : (gap == 1 ? 4 : (gap == 2 ? 6 : 9));      // ref @B32325
        int o_lo = 0, o_hi = 0;
        for (int o = 0; o < n; o++) {
            const int lo = __builtin_amdgcn_readlane(pk_l, o);
            o_lo += (lo <= bin - win) ? 1 : 0;
            o_hi += (lo < bin + win) ? 1 : 0;
        }
        const int cnt = live ? o_hi - o_lo : 0;
        const int incl = (int)wave_incl_scan_u32((uint32_t)cnt);
        const int off = incl - cnt;
        const int M = __builtin_amdgcn_readlane(incl, 63);
        const int maxc = (int)wave_max_u32((uint32_t)cnt);
        for (int base = 0; base < M; base += 64) {
            if (lane < MAXC) { L.s_best[lane] = 0ull; L.s_asg[lane] = 0x7fffffff; }
            for (int c = 0; c < maxc; c++) {
                const int slot = off + c - base;
                if (c < cnt && slot >= 0 && slot < 64) { L.s_pr_j[slot] = j; L.s_pr_o[slot] = o_lo + c; }
            }
            wsync();
            const bool pv = base + lane < M;
            int jj = 0, oo = 0; double sc = 0;
            if (pv) {
                jj = L.s_pr_j[lane]; oo = L.s_pr_o[lane];
                const int tb = (int)(L.a_bins[jj] & 0xff), tg = nfile - L.a_last_frame[jj];
                const int pl = (int)((L.s_pk[oo] >> 16) & 0xff);
                sc = match_score(tg, (double)abs(tb - pl), (double)L.a_len[jj], (double)tb, (double)pl,
                                 (double)L.a_amp[jj], (double)L.s_amp[oo], L.a_vel[jj]);
                if (sc > 1) atomicMax(&L.s_best[oo], (unsigned long long)__double_as_longlong(sc));
            }
            wsync();
            if (pv && sc > 1 && (unsigned long long)__double_as_longlong(sc) == L.s_best[oo]) atomicMin(&L.s_asg[oo], jj);
            wsync();
            if (lane < n) {
                const int cj = L.s_asg[lane];
                if (cj != 0x7fffffff) {
                    const double cs = __longlong_as_double((long long)L.s_best[lane]);
                    if (cs > best) { best = cs; asg = cj; }
                }
            }
            wsync();
        }
    }
    sp.acp.lap(WSA_TUNE(DBG_PHASES), 2);
    // 3. hand each matched track the set of its peaks
    if (lane < n && asg >= 0) atomicOr(&L.a_mmask[asg], 1ull << lane);
    wsync();
    const int p_begin = sp.n_pt;
    // 4. matched tracks update themselves (lane = track), points in track order
    for (int tbase = 0; tbase < sp.n_act; tbase += 64) {
        const int j = tbase + lane;
        const unsigned long long mm = j < sp.n_act ? L.a_mmask[j] : 0ull;
        bool upd = false; int pb = 0, st = 0, en = 0; uint32_t a0 = 0; double be = 0;
        if (mm) {
            const int first = __ffsll((long long)mm) - 1;
            const uint32_t w0 = L.s_pk[first];
            pb = (w0 >> 16) & 0xff;
            a0 = L.s_amp[first];                       // amplitude of the FIRST assigned peak (quirk 3)
            if ((double)a0 > fl) {
                upd = true;
                st = w0 & 0xff; en = (w0 >> 8) & 0xff;
                double lo_sum = L.s_plo[first], hi_sum = L.s_phi[first];
                uint32_t pb_amp = a0;
                unsigned long long rest = mm & (mm - 1ull);       // (the first assigned peak is where st / en / pb start from)
                while (rest) {
                    const int o = __ffsll((long long)rest) - 1; rest &= rest - 1;
                    const uint32_t w = L.s_pk[o];
                    const int oi = w & 0xff, os = (w >> 8) & 0xff, ol = (w >> 16) & 0xff;
                    if (os > en) { en = os; hi_sum = L.s_phi[o]; }
                    if (oi < st) { st = oi; lo_sum = L.s_plo[o]; }
                    if (L.s_amp[o] > pb_amp) { pb = ol; pb_amp = L.s_amp[o]; }
                }
                be = hi_sum - lo_sum;                // sum e[st..en], exact
            }
        }
        const uint64_t um = __ballot(upd);
        const int nu = __popcll(um);
        if (sp.n_pt + nu > p.pcap) { sp.overflow = true; }
        else if (upd) {
            const int q = sp.n_pt + __popcll(um & lanemask_lt(lane));
            const int hlen = L.a_len[j];
            const uint32_t bn = L.a_bins[j];
            const int P1 = bn & 0xff, P2 = (bn >> 8) & 0xff, P3 = (bn >> 16) & 0xff;
            double vel = L.a_vel[j];
            if (hlen >= 3) {      // x / 3, correctly rounded: q = x * (1/3), r = x - 3q (exact), q + r * (1/3)
                const double xv = (double)((pb - P1) + (P2 - P1) + (P3 - P2)), third = 1.0 / 3.0;
                const double q0 = xv * third;
                vel = __builtin_fma(__builtin_fma(-3.0, q0, xv), third, q0);
            }
            else if (hlen == 2) vel = (double)((pb - P1) + (P2 - P1)) / 2;
            else if (hlen == 1) vel = (double)(pb - P1);
            const double se = L.a_sumE[j] + be, sb = L.a_sumEbin[j] + be * pb;
            L.a_vel[j] = vel; L.a_bins[j] = (uint32_t)pb | ((uint32_t)P1 << 8) | ((uint32_t)P2 << 16);
            L.a_amp[j] = a0; L.a_last_frame[j] = nfile; L.a_len[j] = hlen + 1; L.a_sumE[j] = se; L.a_sumEbin[j] = sb;
            const int t = L.a_gid[j];
            sp.W.pt[q] = make_int4(t, pb | ((en - st + 1) << 8) | (min(nfile, 0x7fff) << 17), __double2loint(be), __double2hiint(be));
            if (RAW) sp.W.ptx[q] = make_int4(st, (int)a0, nfile, en);
        }
        if (upd) sp.accL += be;                     // integer-valued: exact in any order
        if (!sp.overflow) sp.n_pt += nu;
    }
    sp.acp.lap(WSA_TUNE(DBG_PHASES), 3);
    // 5. unassigned peaks above the floor open new tracks, in peak order (lane = peak)
    const bool mk = lane < n && asg == -1 && (double)pk_amp > fl;
    const uint64_t nm = __ballot(mk);
    const int nnew = __popcll(nm);
    // (WSA_DBG bit 10, tests: the LDS table of the default variant pretends to hold 12 tracks, so that the rerun path runs on ordinary input)
    if (sp.n_act + nnew > ((p.dbg & DBG_SMALL_TABLE) && AC < AC_MAX ? 12 : AC)) { sp.act_overflow = true; sp.overflow = true; }
    if (sp.n_tr + nnew > p.tcap || sp.n_pt + nnew > p.pcap) sp.overflow = true;
    if (sp.overflow) {}
    else if (mk) {
        const int r = __popcll(nm & lanemask_lt(lane));
        const int t = sp.n_tr + r, q = sp.n_pt + r, j = sp.n_act + r;
        const double be = pk_phi - pk_plo;
        L.a_last_frame[j] = nfile; L.a_len[j] = 1; L.a_gid[j] = t; L.a_bins[j] = (uint32_t)pk_l; L.a_amp[j] = pk_amp;
        L.a_vel[j] = 0; L.a_sumE[j] = be; L.a_sumEbin[j] = be * pk_l;
        sp.W.pt[q] = make_int4(t, pk_l | ((pk_s - pk_i + 1) << 8) | (min(nfile, 0x7fff) << 17), __double2loint(be), __double2hiint(be));
        if (RAW) sp.W.ptx[q] = make_int4(pk_i, (int)pk_amp, nfile, pk_s);
    }
    if (!sp.overflow) { sp.n_tr += nnew; sp.n_pt += nnew; sp.n_act += nnew; }
    sp.acp.lap(WSA_TUNE(DBG_PHASES), 4);
    // file this frame's point range under its (possibly stale) index
    if (reset_this_frame) { sp.stale_d = nfile; sp.stale_p1 = sp.n_pt; }
    else if (lane == 0 && nfile < p.fcap + 2) { sp.W.d_p0[nfile] = p_begin; sp.W.d_p1[nfile] = sp.n_pt; sp.W.d_gen[nfile] = sp.gen; }
    wsync();
}
// tuning (WSA_DBG bit 16): per-span cycle counts into the trace buffer (tools/span_probe.py); tk0 .. tk1 = the accumulate part
__device__ __forceinline__ void trace_span_cycles(const TrParams& p, const SpanState& sp, int lane, unsigned long long tk0, unsigned long long tk1) {
    if ((WSA_TUNE(DBG_CYCLES)) && lane == 0 && p.trace) {      // tuning: per-span cycle counts into the trace buffer
        double* tr = p.trace + (uint64_t)atomicAdd(&p.shared[0], 1u) * 12;      // shared[0] is otherwise unused
        tr[0] = (double)(tk1 - tk0); tr[1] = (double)(__builtin_readcyclecounter() - tk1); tr[2] = sp.len; tr[3] = (double)(sp.f_end - sp.f_begin); tr[4] = sp.n_tr; tr[5] = sp.n_pt; tr[6] = blockIdx.x;
        if (WSA_TUNE(DBG_PHASES)) { tr[7] = (double)sp.acp.cy[0]; tr[8] = (double)sp.acp.cy[1]; tr[9] = (double)sp.acp.cy[2]; tr[10] = (double)sp.acp.cy[3]; tr[11] = (double)sp.acp.cy[4]; }
        else { tr[7] = (double)(sp.ph[0] - tk1); tr[8] = (double)(sp.ph[1] - sp.ph[0]); tr[9] = (double)(sp.ph[2] - sp.ph[1]); tr[10] = (double)(sp.ph[3] - sp.ph[2]); }
    }
}
// ---- a batch's span, frame by frame
// What gate.hip left per frame (info, v, fl) and the record header are fetched for 64 frames at a time, lane j = frame blk + j, one block ahead; a frame gets its
// values by v_readlane.  The candidate entries (lane = candidate) of frame f + PFD are requested while frame f is processed — as soon as f's own entry has been
// copied out of its registers — so that neither fetch is waited for (before: groups of 4 frames paid one memory round trip each, ~900 cycles a frame).
template <int AC, bool RAW>
__device__ __forceinline__ void track_span(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane) {
    constexpr int PFD = 4;
    struct Ent { uint32_t pk, amp, plo, phi, hi; };
    auto load_blk = [&](uint32_t fb, Hdr& q) __attribute__((always_inline)) {
        const uint32_t f = fb + (uint32_t)lane, fi = sp.foff + min(f, sp.f_end - 1);
        q.info = p.fr_info[fi]; q.v = p.fr_v[fi]; q.fl = p.fr_fl[fi]; q.h = p.rec.hdr[fi];
        if (f >= sp.f_end) q.info = -1;
    };
    Hdr bc, bn;
    // entry of the frame at position j of the current block (j >= 64: of the next block)
    auto request = [&](int j, Ent& e) __attribute__((always_inline)) {
        const int info_ = j < 64 ? read_lane_i32(bc.info, j & 63) : read_lane_i32(bn.info, j & 63);
        const int hy = j < 64 ? read_lane_i32((int)bc.h.y, j & 63) : read_lane_i32((int)bn.h.y, j & 63);
        const uint32_t cb = (uint32_t)(j < 64 ? read_lane_i32((int)bc.h.w, j & 63) : read_lane_i32((int)bn.h.w, j & 63));
        e.pk = e.amp = e.plo = e.phi = e.hi = 0u;
        if (info_ >= 0 && lane < ((hy >> 8) & 0xff) && !(WSA_TUNE(DBG_NO_ENTRIES))) {           // only frames accumulate_fm sees, only the entries they hold
            const uint32_t c = cb + (uint32_t)lane;
            const uint4 e4 = p.rec.ent[c];
            e.amp = p.rec.amp[c]; e.pk = e4.x; e.plo = e4.y; e.phi = e4.z; e.hi = e4.w;
        }
    };
    load_blk(sp.f_begin, bc);
    bn = bc;
    if (sp.f_begin + 64 < sp.f_end) load_blk(sp.f_begin + 64, bn);
    Ent ring[PFD];
    #pragma unroll
    for (int k = 0; k < PFD; k++) request(k, ring[k]);
    for (uint32_t blk = sp.f_begin; blk < sp.f_end; blk += 64) {
      const int nb = (int)min(64u, sp.f_end - blk);
      for (int j0 = 0; j0 < nb; j0 += PFD) {
    #pragma unroll
        for (int k = 0; k < PFD; k++) {
          const int j = j0 + k;
          if (j >= nb) break;
          Pre cur;
          const int hy = read_lane_i32((int)bc.h.y, j);
          cur.info = read_lane_i32(bc.info, j); cur.v = read_lane_f64(bc.v, j); cur.fl = read_lane_f64(bc.fl, j);
          cur.g = (double)(hy & 0xff) * 4294967296.0 + (double)(uint32_t)read_lane_i32((int)bc.h.x, j);      // exact: g < 2^40
          cur.n = (hy >> 8) & 0xff;
          cur.pk = ring[k].pk; cur.amp = ring[k].amp; cur.plo = ring[k].plo; cur.phi = ring[k].phi; cur.hi = ring[k].hi;
          accumulate<AC, RAW>(p, sp, L, lane, cur, [&]() __attribute__((always_inline)) { request(j + PFD, ring[k]); });
          if (p.trace && !(WSA_TUNE(DBG_CYCLES))) { double accS, accC; sp.totals(accS, accC); if (lane == 0) { double* tr = p.trace + ((uint64_t)sp.foff + blk + (uint32_t)j) * 12; tr[10] = accS; tr[11] = accC; } }
        }
      }
      bc = bn;
      if (blk + 128 < sp.f_end && !(WSA_TUNE(DBG_NO_PREFETCH))) load_blk(blk + 128, bn);
    }
}
// ---- incremental streaming: this wave owns stream `sp.clip`.  Its tracker state (counters, accumulators, the active table; the track / point arrays live in the
//      stream's work space anyway) comes from HBM, the frames of this step are accumulated one by one, a segment the gate closed in this step is finalized right
//      behind its last frame, and the state goes back.  Every reset_segment of the reference clears the tracker: gate.hip notes for each accumulate call the span it
//      belongs to (fr_span) and a change of span clears the state here.
template <int AC, bool RAW>
__device__ __forceinline__ void track_stream(const TrParams& p, SpanState& sp, const OneLds<AC>& L, int lane) {
    int vz; asm volatile("v_mov_b32 %0, 0" : "=v"(vz));          // a zero the compiler cannot see through (see load_hdr)
    int32_t* stt = p.st_state + (uint64_t)sp.clip * TR_STATE_WORDS;
    double* std_ = reinterpret_cast<double*>(stt + 8);
    sp.n_tr = stt[0]; sp.n_pt = stt[1]; sp.n_act = stt[2]; sp.stale_d = stt[3]; sp.stale_p1 = stt[4]; int my_span = stt[5]; sp.gen = stt[6];
    sp.accG = std_[0] + std_[1]; sp.accL = lane == 0 ? std_[1] : 0.0;
    char* ab = p.st_act + (uint64_t)sp.clip * TR_ACT_BYTES;
    double* const g_vel = reinterpret_cast<double*>(ab); double* const g_sumE = g_vel + AC; double* const g_sumEbin = g_sumE + AC;
    int32_t* const g_lf = reinterpret_cast<int32_t*>(g_sumEbin + AC); int32_t* const g_len = g_lf + AC; int32_t* const g_gid = g_len + AC;
    uint32_t* const g_bins = reinterpret_cast<uint32_t*>(g_gid + AC); uint32_t* const g_amp = g_bins + AC;
    for (int j = lane; j < sp.n_act; j += 64) {
        L.a_vel[j] = g_vel[j]; L.a_sumE[j] = g_sumE[j]; L.a_sumEbin[j] = g_sumEbin[j];
        L.a_last_frame[j] = g_lf[j]; L.a_len[j] = g_len[j]; L.a_gid[j] = g_gid[j]; L.a_bins[j] = g_bins[j]; L.a_amp[j] = g_amp[j];
    }
    wsync();
    auto clear_state = [&](int span) __attribute__((always_inline)) { sp.clear_tracks(); sp.gen++; my_span = span; };
    const uint32_t nfr = p.n_frames_step[sp.clip];
    const uint32_t fbase = (uint32_t)p.gate_state[(uint64_t)sp.clip * GATE_STATE] - nfr;       // the gate has counted this step's frames already
    const int nseg = (int)p.seg_count[sp.clip];
    sp.f_begin = fbase; sp.f_end = fbase + nfr;                 // the record fetchers clamp to [f_begin, f_end)
    int ks = 0;
    auto close_segments = [&](uint32_t f_next, bool all) __attribute__((always_inline)) {
        while (ks < nseg) {
            int32_t* sgk = p.seg_i + ((uint64_t)sp.clip * p.seg_cap + ks) * 8;
            if (!all && (uint32_t)sgk[SEG_FEND] != f_next) break;
            if (sgk[SEG_FBEGIN] != my_span) clear_state(sgk[SEG_FBEGIN]);      // no frame of the span reached accumulate_fm
            sp.my_seg = ks; sp.load_segment(p, false);                         // (f_begin / f_end stay the step's frames)
            finish_span<AC, RAW, false>(p, sp, L, lane, true);
            clear_state(-2);                                                    // every finalize is followed by a reset_segment
            ks++;
        }
    };
    for (uint32_t f = fbase; f < fbase + nfr; f++) {
        Hdr h; load_hdr(p, sp, vz, f, h);
        Pre cur; load_ent(p, sp, lane, f, h, cur);
        if (cur.info >= 0) {
            const int span = p.fr_span[sp.foff + (f & p.ring_mask)];
            if (span != my_span) clear_state(span);
            accumulate<AC, RAW>(p, sp, L, lane, cur, [] {});
        }
        close_segments(f + 1, false);
    }
    close_segments(0, true);
    double accS, accC; sp.totals(accS, accC);
    if (lane == 0) { stt[0] = sp.n_tr; stt[1] = sp.n_pt; stt[2] = sp.n_act; stt[3] = sp.stale_d; stt[4] = sp.stale_p1; stt[5] = my_span; stt[6] = sp.gen; std_[0] = accS; std_[1] = accC; }
    for (int j = lane; j < sp.n_act; j += 64) {
        g_vel[j] = L.a_vel[j]; g_sumE[j] = L.a_sumE[j]; g_sumEbin[j] = L.a_sumEbin[j];
        g_lf[j] = L.a_last_frame[j]; g_len[j] = L.a_len[j]; g_gid[j] = L.a_gid[j]; g_bins[j] = L.a_bins[j]; g_amp[j] = L.a_amp[j];
    }
}

}  // namespace wsa
