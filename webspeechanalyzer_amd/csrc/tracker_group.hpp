// tracker_group.hpp — accumulate_fm for two or four spans per wave, in lock step.  Included by tracker.hip behind tracker_finalize.hpp.
// Used by: tracker_kernel_pair (GW = 32, then finalize_pair), tracker_kernel_pair_acc (GW = 32) and tracker_kernel_quad_acc (GW = 16), which end in write_span_headers.
// Two spans per wave: accumulate_fm keeps ~10 of a wave's 64 lanes busy (ten peaks, ten-odd live tracks), and the kernel is bound by instruction issue, so the
// halves of the wave track two spans in lock step: every instruction below serves both. Each half has its own active-track table (PAIR_AC entries), peak scratch and
// work space; quantities that are scalars in the one-span code are vector registers that hold one value per half.  A frame brings at most 32 accepted peaks here and
// a span at most PAIR_AC live tracks; a span that needs more is put on the redo list and tracked by the one-span kernel afterwards. Retired tracks only leave the
// table every fourth frame (a dead track never matches: its gap only grows), the window counts come from a bit map of the accepted peaks' bins instead of a loop
// over the peaks.  Finalize then runs for one span after the other with the whole wave, out of the same LDS block (both tables are dead by then).
#pragma once

namespace wsa {

// a group's part of the LDS block: its active-track table (t_*), then the per-frame scratch (q_*)
template <int GW>
struct GroupLds {
    static constexpr int ACG = GW == 32 ? PAIR_AC : QUAD_AC, NGR = 64 / GW, GSZ = GW == 32 ? PAIR_GSZ : QUAD_GSZ;
    static_assert(GSZ % 16 == 0 && GSZ >= ACG * 48 + GW * 40 + 24 && (ACG * 24) % 8 == 0 && (ACG * 48 + GW * 20) % 8 == 0, "group layout fits its share of the block");
    double *t_vel, *t_sumE, *t_sumEbin; uint32_t* t_mmask; int32_t *t_lf, *t_len, *t_gid; uint32_t *t_bins, *t_amp;
    uint32_t *q_pk, *q_amp, *q_plo, *q_phi, *q_hi;      // accepted peaks of the group's frame, compacted: entry word, amplitude, low words of P[i-1] / P[s], their high bytes
    unsigned long long* q_best; int32_t *q_asg, *q_prj, *q_pro;
    uint32_t* q_map;                                    // {0, bins 0..31, 32..63, 64..95, 96..127, 0}: which bins hold an accepted peak
    __device__ __forceinline__ GroupLds(unsigned char* big, int g) {
        unsigned char* const gb = big + g * GSZ;
        t_vel = reinterpret_cast<double*>(gb); t_sumE = t_vel + ACG; t_sumEbin = t_sumE + ACG;
        t_mmask = reinterpret_cast<uint32_t*>(t_sumEbin + ACG);
        t_lf = reinterpret_cast<int32_t*>(t_mmask + ACG); t_len = t_lf + ACG; t_gid = t_len + ACG;
        t_bins = reinterpret_cast<uint32_t*>(t_gid + ACG); t_amp = t_bins + ACG;
        q_pk = t_amp + ACG; q_amp = q_pk + GW; q_plo = q_amp + GW; q_phi = q_plo + GW; q_hi = q_phi + GW;
        q_best = reinterpret_cast<unsigned long long*>(q_hi + GW);
        q_asg = reinterpret_cast<int32_t*>(q_best + GW); q_prj = q_asg + GW; q_pro = q_prj + GW;
        q_map = reinterpret_cast<uint32_t*>(q_pro + GW);
    }
};
// what a group of lanes knows about its span (one value per group: vector registers where the one-span code has scalars)
struct GroupState {
    bool has, redo, ovf;                                // a span was dealt to the group; it goes on the redo list; its work space overflowed
    uint32_t clip, seg, fb, fe, foff; int F, tcap, fcap; Ws W;
    int ntr, npt, nact, stale_d, stale_p1; double accG, accL;
    PhaseClock clk; int pn_chunk2, pn_pass, pn_on;      // tuning (WSA_DBG bit 16): cycles per phase, steps with two track chunks, pair passes, frames with peaks
};
// ---- the group's span (entry NGR * t.group + g of the length-sorted list), its work space — SPLIT: the span's own region of the pool, 64 tracks /
//      points per frame — and an empty table
template <int GW, int SPLIT>
__device__ __forceinline__ void group_begin(const TrParams& p, GroupState& gs, const GroupLds<GW>& G, int lane, const SpanTurn& t) {
    constexpr int NGR = 64 / GW;
    const int g = lane / GW, gl = lane % GW;
    const uint32_t e_idx = (uint32_t)(NGR * t.group) + (uint32_t)g;
    gs.has = e_idx < t.total;
    const uint2 oe = gs.has ? p.order[e_idx] : make_uint2(0u, 0u);
    gs.clip = oe.x; gs.seg = oe.y;
    const int32_t* gsg = p.seg_i + ((uint64_t)gs.clip * p.seg_cap + gs.seg) * 8;
    gs.fb = gs.has ? (uint32_t)gsg[SEG_FBEGIN] : 0u; gs.fe = gs.has ? (uint32_t)gsg[SEG_FEND] : 0u;
    gs.foff = p.frame_off[gs.clip];
    gs.F = (int)(gs.fe - gs.fb);
    gs.tcap = SPLIT ? MAXC * gs.F : p.tcap; gs.fcap = SPLIT ? gs.F : p.fcap;            // split finalize: the span's own region, 64 tracks / points per frame
    gs.W = SPLIT ? carve_ws(p.pool + (uint64_t)(gs.foff + gs.fb) * p.pool_bpf, gs.tcap, gs.tcap, gs.fcap, 0, nullptr)
                        : carve_ws(p.ws + ((uint64_t)blockIdx.x * 2 + (uint32_t)g) * p.ws_stride, p.tcap, p.pcap, p.fcap, 0, nullptr);
    if (SPLIT) { if (gs.has) for (int d = gl; d < gs.F + 2; d += GW) gs.W.d_gen[d] = 0; }
    gs.ntr = 0; gs.npt = 0; gs.nact = 0; gs.stale_d = -1; gs.stale_p1 = 0;
    gs.accG = 0; gs.accL = 0;
    gs.ovf = false; gs.redo = SPLIT && gs.has && gs.F < 1;
    if (gl == 0) { G.q_map[0] = 0u; G.q_map[5] = 0u; }
    gs.pn_chunk2 = gs.pn_pass = gs.pn_on = 0;
}
// ---- the frames of the group's spans in lock step; `gen` marks the d_* entries of this turn (unsplit pair).  Returns the number of steps
template <int GW, int SPLIT>
__device__ __forceinline__ int group_accumulate(const TrParams& p, GroupState& gs, const GroupLds<GW>& G, int lane, int gen) {
    constexpr int ACG = GroupLds<GW>::ACG;
    const int gl = lane % GW;
    const uint32_t below = (1u << gl) - 1u;
    auto dbl40 = [](uint32_t lo, uint32_t hi8) __attribute__((always_inline)) { return (double)(hi8 & 0xffu) * 4294967296.0 + (double)lo; };
    // per frame: what gate.hip left (info, v, fl), the record header, the first 32 candidate entries; two / one frame(s) ahead
    struct FH { int info; double v, fl; uint4 h; };
    struct FC { uint4 e; uint32_t amp; };
    auto load_fh = [&](uint32_t k, FH& q) __attribute__((always_inline)) {
        const uint32_t f = gs.fb + k, fi = gs.foff + (gs.fe > gs.fb ? min(f, gs.fe - 1u) : 0u);
        // 32-bit byte offsets off the (uniform) table bases: `global_load v, v_off, s[base]` instead of a 64-bit address per table (a batch holds fewer
        // than 2^28 frames: wsa_batch_create)
        auto at = [](const auto* base, uint32_t byte_off) __attribute__((always_inline)) { return *reinterpret_cast<decltype(base)>(reinterpret_cast<const char*>(base) + byte_off); };
        q.info = at(p.fr_info, fi << 2); q.v = at(p.fr_v, fi << 3); q.fl = at(p.fr_fl, fi << 3); q.h = at(p.rec.hdr, fi << 4);
        if (f >= gs.fe) q.info = -1;
    };
    auto load_fc = [&](const FH& h, FC& q) __attribute__((always_inline)) {
        q.e = make_uint4(0u, 0u, 0u, 0u); q.amp = 0u;
        if (h.info >= 0 && gl < (int)((h.h.y >> 8) & 0xffu)) { const uint32_t c = h.h.w + (uint32_t)gl; q.e = p.rec.ent[c]; q.amp = p.rec.amp[c]; }
    };
    const int nsteps = groups_max_i32<GW>((int)(gs.fe - gs.fb));
    FH h0, h1, h2; FC c0, c1;
    load_fh(0u, h0); load_fh(1u, h1); load_fc(h0, c0);
    for (int step = 0; step < nsteps; step++) {
        load_fh((uint32_t)step + 2u, h2);
        load_fc(h1, c1);
        const bool act = h0.info >= 0 && !gs.redo && !WSA_TUNE(DBG_NO_ACCUMULATE);      // (WSA_DBG bit 2, TUNING builds: the what-if "no accumulate" — the spans are walked, nothing is tracked)
        if (__ballot(act) != 0ull) {
            const int info = h0.info, nfile = info & 0x3fffffff;
            const bool rst = ((info >> 30) & 1) != 0;
            const int ncand = (int)((h0.h.y >> 8) & 0xffu);
            const double v = h0.v, fl = h0.fl;
            gs.clk.start(WSA_TUNE(DBG_CYCLES));
            if (gl < 4) G.q_map[1 + gl] = 0u;
            wsync();
            // ---- accepted peaks (ref @B25827: `e[l] > v`), compacted per half; their bins into the bit map
            int n = 0;
            const int ncmax = groups_max_i32<GW>(act ? ncand : 0);
            for (int cb = 0; cb < ncmax; cb += GW) {
                uint4 e4 = c0.e; uint32_t am = c0.amp;
                const bool hasc = act && cb + gl < ncand;
                if (cb > 0) { e4 = make_uint4(0u, 0u, 0u, 0u); am = 0u; if (hasc) { const uint32_t c = h0.h.w + (uint32_t)(cb + gl); e4 = p.rec.ent[c]; am = p.rec.amp[c]; } }
                const bool acc = hasc && (double)am > v;
                const uint32_t m = group_ballot<GW>(acc, lane);
                const int pos = n + __popc(m & below);
                if (acc && pos < GW) {
                    G.q_pk[pos] = e4.x; G.q_amp[pos] = am; G.q_plo[pos] = e4.y; G.q_phi[pos] = e4.z; G.q_hi[pos] = e4.w;
                    const uint32_t lb = (e4.x >> 16) & 0x7fu;
                    atomicOr(&G.q_map[1 + (lb >> 5)], 1u << (lb & 31u));
                }
                n += __popc(m);
            }
            if (WSA_TUNE(DBG_CYCLES) && act && n > GW && !gs.redo && gl == 0) atomicAdd(&p.shared[10], 1u);      // tuning: spans declined for their peaks ...
            if (act && n > GW) gs.redo = true;                       // more peaks than the group of lanes holds: the one-span kernel takes the span
            const bool on = act && n >= 1 && n <= GW;
            if (on) gs.accG += (double)(h0.h.y & 0xffu) * 4294967296.0 + (double)h0.h.x;          // g < 2^40, exact
            wsync();
            if (__ballot(on) != 0ull) {
                const bool ispk = on && gl < n;
                // (reads without a lane test where the index stays inside the group's arrays: what a lane without a peak / a track reads is never used —
                //  every conditional block costs the wave an exec save, a branch and a restore, and this kernel is bound by its instruction count)
                const uint32_t pkw = G.q_pk[gl], pamp = G.q_amp[gl];
                const int pk_i = pkw & 0xff, pk_s = (pkw >> 8) & 0xff, pk_l = (pkw >> 16) & 0xff;
                const uint32_t m0 = G.q_map[1], m1 = G.q_map[2], m2 = G.q_map[3], m3 = G.q_map[4];
                const int pc1 = __popc(m0), pc2 = pc1 + __popc(m1), pc3 = pc2 + __popc(m2);
                gs.clk.lap(WSA_TUNE(DBG_CYCLES), 0); gs.pn_on++;
                // ---- 1. retired tracks leave the table (stable compaction): every fourth frame, or when the frame's new tracks might not fit
                const bool compact = on && ((step & 3) == 0 || gs.nact + n > ACG);
                if (__ballot(compact) != 0ull) {
                    int kept = 0;
                    const int na_max = groups_max_i32<GW>(compact ? gs.nact : 0);
                    for (int tb = 0; tb < na_max; tb += GW) {
                        const int j = tb + gl;
                        const bool valid = compact && j < gs.nact;
                        const int jr = GW == 32 ? j : min(j, ACG - 1);      // (two chunks of 32 are the 64 entries; a third chunk of 16 would reach past 38)
                        const int lf = G.t_lf[jr], ln = G.t_len[jr], gi = G.t_gid[jr]; const uint32_t bn = G.t_bins[jr], am = G.t_amp[jr]; const double ve = G.t_vel[jr], se = G.t_sumE[jr], sb = G.t_sumEbin[jr];
                        const bool keep = valid && (nfile - lf) < 4;
                        const uint32_t km = group_ballot<GW>(keep, lane);
                        if (valid && !keep) { gs.W.tr_len[gi] = ln; gs.W.tr_sumE[gi] = se; gs.W.tr_sumEbin[gi] = sb; }   // the summary finalize ranks by
                        wsync();
                        if (keep) {
                            const int q = kept + __popc(km & below);
                            G.t_lf[q] = lf; G.t_len[q] = ln; G.t_gid[q] = gi; G.t_bins[q] = bn; G.t_amp[q] = am; G.t_vel[q] = ve; G.t_sumE[q] = se; G.t_sumEbin[q] = sb;
                        }
                        kept += __popc(km);
                        wsync();
                    }
                    if (compact) gs.nact = kept;
                }
                // ---- 2. score every (track, peak) pair inside the track's search window; per peak the best score > 1, the EARLIER
                //         track on ties (ref: `i>1&&i>d[o]` in track order)
                gs.clk.lap(WSA_TUNE(DBG_CYCLES), 1);
                int asg = -1; double best = 0;
                const int na_max = groups_max_i32<GW>(on ? gs.nact : 0);
                if (na_max > GW) gs.pn_chunk2++;
                for (int tb = 0; tb < na_max; tb += GW) {
                    const int j = tb + gl;
                    const bool valid = on && j < gs.nact;
                    const int jr = GW == 32 ? j : min(j, ACG - 1);
                    const int gap = nfile - G.t_lf[jr], bin = (int)(G.t_bins[jr] & 0xffu);
                    if (valid) G.t_mmask[j] = 0u;
                    const bool live = valid && gap >= 0 && gap < 4;
                    const int win = (int)((0x9643u >> (4 * (gap & 3))) & 0xfu);               // [3, 4, 6, 9][gap], ref @B32325 (gap in 0 .. 3 wherever the value is used)
                    // peaks with bin - win < l < bin + win: the map's bits [lo, bin + win); o_lo = peaks below lo (the peaks are in bin order)
                    const int lo = max(bin - win + 1, 0), width = bin + win - lo;              // width in 3 .. 17
                    const int w0 = lo >> 5, sh = lo & 31;
                    const uint32_t wa = w0 == 0 ? m0 : (w0 == 1 ? m1 : (w0 == 2 ? m2 : m3));
                    const uint32_t wb = w0 == 0 ? m1 : (w0 == 1 ? m2 : (w0 == 2 ? m3 : 0u));
                    const uint32_t wnd = (uint32_t)(((((unsigned long long)wb) << 32) | wa) >> sh) & ((1u << width) - 1u);
                    const int o_lo = (w0 == 0 ? 0 : (w0 == 1 ? pc1 : (w0 == 2 ? pc2 : pc3))) + __popc(wa & ((1u << sh) - 1u));
                    const int cnt = live ? __popc(wnd) : 0;
                    const int incl = (int)group_incl_scan_u32<GW>((uint32_t)cnt);
                    const int off = incl - cnt;
                    const int M = (int)group_last_u32<GW>((uint32_t)incl, lane);
                    const int M_max = groups_max_i32<GW>(M);
                    for (int base = 0; base < M_max; base += GW) {
                        gs.pn_pass++;
                        G.q_best[gl] = 0ull; G.q_asg[gl] = 0x7fffffff;
                        for (int c = 0; __ballot(c < cnt) != 0ull; c++) {
                            const int slot = off + c - base;
                            if (c < cnt && slot >= 0 && slot < GW) { G.q_prj[slot] = j; G.q_pro[slot] = o_lo + c; }
                        }
                        wsync();
                        const bool pv = base + gl < M;
                        // (a lane without a pair scores whatever its list slot holds, clamped into the tables, and keeps the result to itself)
                        const int jj = (int)min((uint32_t)G.q_prj[gl], (uint32_t)(ACG - 1)), oo = (int)min((uint32_t)G.q_pro[gl], (uint32_t)(GW - 1));
                        const int tbn = (int)(G.t_bins[jj] & 0xffu), tg = nfile - G.t_lf[jj];
                        const int pl = (int)((G.q_pk[oo] >> 16) & 0xffu);
                        const double sc = match_score(tg, (double)abs(tbn - pl), (double)G.t_len[jj], (double)tbn, (double)pl,
                                                      (double)G.t_amp[jj], (double)G.q_amp[oo], G.t_vel[jj]);
                        const bool cand = pv && sc > 1;
                        if (cand) atomicMax(&G.q_best[oo], (unsigned long long)__double_as_longlong(sc));
                        wsync();
                        if (cand && (unsigned long long)__double_as_longlong(sc) == G.q_best[oo]) atomicMin(&G.q_asg[oo], jj);
                        wsync();
                        {
                            const int cj = G.q_asg[gl];
                            const double cs = __longlong_as_double((long long)G.q_best[gl]);
                            if (ispk && cj != 0x7fffffff && cs > best) { best = cs; asg = cj; }
                        }
                        wsync();
                    }
                }
                gs.clk.lap(WSA_TUNE(DBG_CYCLES), 2);
                // ---- 3. hand each matched track the set of its peaks
                if (ispk && asg >= 0) atomicOr(&G.t_mmask[asg], 1u << gl);
                wsync();
                const int p_begin = gs.npt;
                // ---- 4. matched tracks update themselves (lane = track)
                for (int tb = 0; tb < na_max; tb += GW) {
                    const int j = tb + gl;
                    const uint32_t mm = (on && j < gs.nact) ? G.t_mmask[j] : 0u;
                    // the first assigned peak is where st / en / pb start from (a track without one reads peak 0: not used)
                    const int first = mm ? __ffs((int)mm) - 1 : 0;
                    const uint32_t w0_ = G.q_pk[first], a0 = G.q_amp[first], hb = G.q_hi[first];      // a0: amplitude of the FIRST assigned peak (quirk 3)
                    const uint32_t plo0 = G.q_plo[first], phi0 = G.q_phi[first];
                    const bool upd = mm != 0u && (double)a0 > fl;
                    int pb = (w0_ >> 16) & 0xff, st = w0_ & 0xff, en = (w0_ >> 8) & 0xff;
                    // P[i-1] and P[s] as 40-bit integers {low word, high byte}: the band sum is one 64-bit subtraction, converted once
                    uint32_t lo_l = plo0, lo_h = hb & 0xffu, hi_l = phi0, hi_h = (hb >> 8) & 0xffu;
                    {
                        uint32_t pb_amp = a0;
                        uint32_t rest = upd ? mm & (mm - 1u) : 0u;
                        while (rest) {
                            const int o = __ffs((int)rest) - 1; rest &= rest - 1u;
                            const uint32_t w = G.q_pk[o];
                            const int oi = w & 0xff, os = (w >> 8) & 0xff, ol = (w >> 16) & 0xff;
                            const uint32_t hbo = G.q_hi[o], ao = G.q_amp[o], plo_o = G.q_plo[o], phi_o = G.q_phi[o];
                            if (os > en) { en = os; hi_l = phi_o; hi_h = (hbo >> 8) & 0xffu; }
                            if (oi < st) { st = oi; lo_l = plo_o; lo_h = hbo & 0xffu; }
                            if (ao > pb_amp) { pb = ol; pb_amp = ao; }
                        }
                    }
                    // sum e[st..en] = P[en] - P[st-1], exact (below 2^40)
                    const unsigned long long be_i = (((unsigned long long)hi_h << 32) | hi_l) - (((unsigned long long)lo_h << 32) | lo_l);
                    const double be = upd ? (double)(uint32_t)(be_i >> 32) * 4294967296.0 + (double)(uint32_t)be_i : 0.0;
                    const uint32_t um = group_ballot<GW>(upd, lane);
                    const int nu = __popc(um);
                    // (the split tracker's span regions hold 64 points and tracks per frame of the span and a frame adds at most GW <= 32 of either: they cannot overflow)
                    if (!SPLIT && gs.npt + nu > gs.tcap) gs.ovf = true;
                    else if (upd) {
                        const int q = gs.npt + __popc(um & below);
                        const int hlen = G.t_len[j];
                        const uint32_t bn = G.t_bins[j];
                        const int P1 = bn & 0xff, P2 = (bn >> 8) & 0xff, P3 = (bn >> 16) & 0xff;
                        // velocity (ref @B36624): all three forms evaluated, one selected (three nested branches cost more than the two extra conversions)
                        // x / 3, correctly rounded: q = x * (1/3), r = x - 3q (exact), q + r * (1/3); x / 2 = x * 0.5 exactly
                        const double xv = (double)((pb - P1) + (P2 - P1) + (P3 - P2)), third = 1.0 / 3.0;
                        const double q0 = xv * third;
                        const double v3 = __builtin_fma(__builtin_fma(-3.0, q0, xv), third, q0);
                        const double v2 = (double)((pb - P1) + (P2 - P1)) * 0.5, v1 = (double)(pb - P1);
                        const double vel = hlen >= 3 ? v3 : (hlen == 2 ? v2 : (hlen == 1 ? v1 : G.t_vel[j]));
                        const double se = G.t_sumE[j] + be, sb = G.t_sumEbin[j] + be * pb;
                        G.t_vel[j] = vel; G.t_bins[j] = (uint32_t)pb | ((uint32_t)P1 << 8) | ((uint32_t)P2 << 16);
                        G.t_amp[j] = a0; G.t_lf[j] = nfile; G.t_len[j] = hlen + 1; G.t_sumE[j] = se; G.t_sumEbin[j] = sb;
                        gs.W.pt[q] = make_int4(G.t_gid[j], pb | ((en - st + 1) << 8) | (min(nfile, 0x7fff) << 17), __double2loint(be), __double2hiint(be));
                    }
                    if (upd) gs.accL += be;                   // integer-valued: exact in any order
                    if (!gs.ovf) gs.npt += nu;
                }
                gs.clk.lap(WSA_TUNE(DBG_CYCLES), 3);
                // ---- 5. unassigned peaks above the floor open new tracks, in peak order (lane = peak)
                const bool mk = ispk && asg == -1 && (double)pamp > fl;
                const uint32_t nm = group_ballot<GW>(mk, lane);
                const int nnew = __popc(nm);
                // (WSA_DBG bits 1024 / 16384, tests: the table pretends to hold 12 tracks, so that the redo list is used on ordinary input)
                if (WSA_TUNE(DBG_CYCLES) && on && gs.nact + nnew > ACG && !gs.redo && gl == 0) atomicAdd(&p.shared[11], 1u);      // ... and for their live tracks
                if (on && gs.nact + nnew > ((p.dbg & (DBG_SMALL_TABLE | DBG_SMALL_GROUP_TABLE)) ? 12 : ACG)) gs.redo = true;           // more live tracks than the half's table holds
                if (!SPLIT && on && (gs.ntr + nnew > gs.tcap || gs.npt + nnew > gs.tcap)) gs.ovf = true;
                const bool grow = on && !gs.ovf && !gs.redo;
                if (grow && mk) {
                    const int r = __popc(nm & below);
                    const int t = gs.ntr + r, q = gs.npt + r, j = gs.nact + r;
                    const uint32_t hb = G.q_hi[gl];
                    const double be = dbl40(G.q_phi[gl], hb >> 8) - dbl40(G.q_plo[gl], hb);
                    G.t_lf[j] = nfile; G.t_len[j] = 1; G.t_gid[j] = t; G.t_bins[j] = (uint32_t)pk_l; G.t_amp[j] = pamp;
                    G.t_vel[j] = 0; G.t_sumE[j] = be; G.t_sumEbin[j] = be * pk_l;
                    gs.W.pt[q] = make_int4(t, pk_l | ((pk_s - pk_i + 1) << 8) | (min(nfile, 0x7fff) << 17), __double2loint(be), __double2hiint(be));
                }
                if (grow) { gs.ntr += nnew; gs.npt += nnew; gs.nact += nnew; }
                // file this frame's point range under its (possibly stale) index
                if (on) {
                    if (rst) { gs.stale_d = nfile; gs.stale_p1 = gs.npt; }
                    else if (gl == 0 && nfile < gs.fcap + 2) { gs.W.d_p0[nfile] = p_begin; gs.W.d_p1[nfile] = gs.npt; gs.W.d_gen[nfile] = SPLIT ? 1 : gen; }
                }
                wsync();
                gs.clk.lap(WSA_TUNE(DBG_CYCLES), 4);
            }
        }
        h0 = h1; h1 = h2; c0 = c1;
    }
    return nsteps;
}
// ---- split tracker: a header per span for the finalize kernel (sum E of the group: integer-valued terms, exact in any order)
template <int GW>
__device__ __forceinline__ void write_span_headers(const TrParams& p, const GroupState& gs, int lane) {
    constexpr int NGR = 64 / GW;
    const int g = lane / GW, gl = lane % GW;
    double cg[NGR];
#pragma unroll
    for (int q = 0; q < NGR; q++) cg[q] = g == q ? gs.accL : 0.0;
    wave_sums_f64(cg);
    double c_mine = cg[0];
#pragma unroll
    for (int q = 1; q < NGR; q++) c_mine = g == q ? cg[q] : c_mine;
    if (gs.has && gl == 0) {
        if (gs.redo) { const uint32_t k = atomicAdd(p.redo_count, 1u); p.redo[k] = make_uint2(gs.clip, gs.seg); }
        double* hd = p.span_hdr + ((uint64_t)gs.clip * p.seg_cap + gs.seg) * 8;
        hd[0] = gs.ntr; hd[1] = gs.npt; hd[2] = gs.stale_d; hd[3] = gs.stale_p1; hd[4] = gs.accG; hd[5] = c_mine;
        hd[6] = gs.redo ? 0.0 : (gs.ovf ? 2.0 : 1.0);
    }
}
// ---- unsplit pair: one finalize after the other with the whole wave, out of the same LDS block (both tables are dead by now)
template <int AC>
__device__ __forceinline__ void finalize_pair(const TrParams& p, SpanState& sp, const GroupState& gs, const OneLds<AC>& L, int lane) {
    const int g = lane / 32;
    for (int h = 0; h < 2; h++) {
        const int src = h * 32;
        if (!read_lane_i32((int)gs.has, src)) continue;
        const uint32_t clip = (uint32_t)read_lane_i32((int)gs.clip, src), seg = (uint32_t)read_lane_i32((int)gs.seg, src);
        if (read_lane_i32((int)gs.redo, src)) {
            if (lane == 0) { const uint32_t k = atomicAdd(p.redo_count, 1u); p.redo[k] = make_uint2(clip, seg); }
            continue;
        }
        sp.begin(p, clip, (int)seg); sp.load_segment(p, true);
        sp.n_tr = read_lane_i32(gs.ntr, src); sp.n_pt = read_lane_i32(gs.npt, src); sp.n_act = 0;
        sp.stale_d = read_lane_i32(gs.stale_d, src); sp.stale_p1 = read_lane_i32(gs.stale_p1, src);
        sp.accG = read_lane_f64(gs.accG, src);
        sp.accL = g == h ? gs.accL : 0.0;
        sp.overflow = read_lane_i32((int)gs.ovf, src) != 0; sp.act_overflow = false;
        sp.W = carve_ws(p.ws + ((uint64_t)blockIdx.x * 2 + (uint32_t)h) * p.ws_stride, p.tcap, p.pcap, p.fcap, 0, nullptr);
        if (!sp.overflow) finish_span<AC, false, false>(p, sp, L, lane);
        if (sp.overflow && lane == 0) atomicOr(&p.shared[1], 1u);
        wsync();
    }
}
// ---- one turn of a group kernel: NGR spans tracked in lock step, then their headers (SPLIT = 1) or their finalizes (the unsplit pair)
template <int AC, int GW, int SPLIT>
__device__ __forceinline__ void track_group(const TrParams& p, SpanState& sp, const OneLds<AC, GW == 16>& L, int lane, const SpanTurn& t) {
    static_assert(GW == 32 || (GW == 16 && SPLIT == 1), "four spans per wave only as the accumulate half of the split tracker");
    static_assert(GW <= GW_MAX, "the SPLIT kernels' span regions are sized for at most GW_MAX new tracks / points per frame (see tracker_pool_bpf)");
    static_assert(GroupLds<GW>::NGR * GroupLds<GW>::GSZ <= OneLds<AC, GW == 16>::BYTES, "the groups fit the block");
    const int gl = lane % GW;
    const GroupLds<GW> G(L.big, lane / GW);
    GroupState gs;
    group_begin<GW, SPLIT>(p, gs, G, lane, t);
    const unsigned long long ptk0 = WSA_TUNE(DBG_CYCLES) ? __builtin_readcyclecounter() : 0ull;
    const int nsteps = group_accumulate<GW, SPLIT>(p, gs, G, lane, sp.gen);
    const unsigned long long ptk1 = WSA_TUNE(DBG_CYCLES) ? __builtin_readcyclecounter() : 0ull;
    // ---- both spans are through: the live tracks hand their summaries over, then one finalize after the other with the whole wave
    for (int j = gl; j < gs.nact; j += GW) { const int gi = G.t_gid[j]; gs.W.tr_len[gi] = G.t_len[j]; gs.W.tr_sumE[gi] = G.t_sumE[j]; gs.W.tr_sumEbin[gi] = G.t_sumEbin[j]; }
    wsync();
    if constexpr (SPLIT == 1) write_span_headers<GW>(p, gs, lane);
    else finalize_pair<AC>(p, sp, gs, L, lane);
    if (WSA_TUNE(DBG_CYCLES) && lane == 0 && p.trace) {      // tuning: per-pair cycle counts into the trace buffer
        double* tr = p.trace + (uint64_t)atomicAdd(&p.shared[0], 1u) * 12;
        tr[0] = (double)(ptk1 - ptk0); tr[1] = (double)(__builtin_readcyclecounter() - ptk1); tr[2] = nsteps; tr[3] = gs.pn_on; tr[4] = gs.pn_chunk2; tr[5] = gs.pn_pass; tr[6] = blockIdx.x;
        tr[7] = (double)gs.clk.cy[0]; tr[8] = (double)gs.clk.cy[1]; tr[9] = (double)gs.clk.cy[2]; tr[10] = (double)gs.clk.cy[3]; tr[11] = (double)gs.clk.cy[4];
    }
}

}  // namespace wsa
