/*
 * backend.c — ORACLE (test infrastructure only; see wsa_oracle.h).
 *
 * Plain-C restatement of the reference's pinned half: u32 spectrum frame -> peak scan -> voiced
 * state machine + auto noise gate -> formant track association -> segment finalize ->
 * straighten -> (syllable split) -> 53-feature vector.  Every function cites the site in
 * /root/reference/dist/main.js (two-line minified bundle; "@B<n>" = byte offset in the file,
 * SURVEY.md §0.2) that it follows.  All scalars are IEEE doubles exactly as JavaScript Numbers;
 * Float32Array stores are explicit (float) casts.  Build with -ffp-contract=off.
 *
 * Math.log10 / Math.pow are the fdlibm forms in jsmath.c (see DESIGN.md "JS-engine math").
 */
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include "wsa_oracle.h"

#define VEC(T) struct { T *p; int32_t n, cap; }
#define VPUSH(v, x) do { if ((v).n == (v).cap) { (v).cap = (v).cap ? 2 * (v).cap : 16; \
    (v).p = realloc((v).p, sizeof(*(v).p) * (size_t)(v).cap); } (v).p[(v).n++] = (x); } while (0)
#define VFREE(v) do { free((v).p); (v).p = NULL; (v).n = (v).cap = 0; } while (0)

/* parseInt(x) for the positive finite doubles that occur here (>= 1e-6, < 1e21): truncation. */
static double js_trunc(double x) { return trunc(x); }

/* one formant track: the 18-field record of accumulate_fm (@B35952; field map SURVEY.md App. A) */
typedef struct {
    double start, end, last_frame, vel, last_bin, last_amp;   /* [0] [1] [2]=[3] [4] [5] [6] */
    VEC(double) frames, starts, ends, bins, amps, energies;   /* [7] .. [12] */
    double sumE, count, sumEbin, sumW;                         /* [13] [14] [15] [17] */
} track_t;

typedef struct { int32_t i, s, l; } peak_t;

typedef struct {
    int32_t start, len, syl0, nsyl, has_feat;
    double feat[53];
    float *fr;              /* len x 9, level >= 4 */
    float *sm;              /* len x 3 (sum f*E, sum E, sum w*E), level >= 4 */
    int32_t max_peaks, max_live;  /* the span's load (see wsa_or_segment_load) */
    int32_t fbegin, fend, cci;    /* the span of frames whose tracks it owns, c_ci at finalize (wsa_or_gate_segment) */
    double g_ctx_max, g_floor;    /* ctx_max and the floor at finalize */
    double *trk; int32_t trk_n;   /* level 3: the ranked tracks the reference stores (`s.push(i)` @B28273), flattened:
                                   * n_tracks, then per track 10 scalars ([0] [1] [2] [4] [5] [6] [13] [14] [15] [17]) and
                                   * its six per-point arrays ([7] .. [12], `count` numbers each) */
} segment_t;

typedef struct { int32_t seg, start, len; double feat[53]; } syllable_t;

/* the arms of the gate's state machine that tests/gate_cases.py aims at (wsa_or_gate_arm_*): bumped where the arm is taken, read only by tests */
#define GATE_ARMS(X) \
    X(start_pass) X(start_n4) X(start_n5) X(start_p7) X(start_p8) X(start_pmax) X(start_pmax_m1) X(start_r_equal) X(start_r_above) \
    X(voiced_n0) X(voiced_p0) X(voiced_p6) X(voiced_p7) X(voiced_pmax_m1) X(voiced_pmax) \
    X(d_equal) X(d_below) X(d_n3) X(d_g_equals_d) X(mx_covers) X(mx_short_n3) X(mx_short_d_covers) \
    X(hdr_eos_largest) X(hdr_tie) \
    X(unvoiced_at_0) X(unvoiced_at_1) X(unvoiced_at_2) X(voiced_at_0) X(voiced_at_1) \
    X(gate_raise_above) X(gate_raise_equal_w) X(gate_decay) X(gate_decay_edge) X(gate_decay_refused_equal) X(gate_neither) X(gate_w40) X(gate_w41) \
    X(floor_t7) X(floor_t6) X(floor_t4) X(floor_t2) X(floor_t1) X(floor_one) \
    X(tk_reset_voiced) X(tk_reset_unvoiced) X(tk_equal) \
    X(decay_first_w21) X(decay_stop) X(decay_clamp10) X(decay_zero_step) \
    X(pause_int) X(pause_frac) X(breaker_rule_250) \
    X(fin_len_min) X(fin_len_min1) X(fin_end_unstarted) X(fin_truncate_open) \
    X(cand_16) X(cand_17) X(cand_64) X(late_n4) X(late_n3) X(late_d) \
    X(ring_cut)
#define X(a) ARM_##a,
enum { GATE_ARMS(X) ARM_COUNT };
#undef X
#define X(a) #a,
static const char *const arm_names[ARM_COUNT] = { GATE_ARMS(X) };
#undef X
#define ARM(S, a) ((S)->arms[ARM_##a]++)

/* the arms of accumulate_fm and finalize that tests/tracker_rule_cases.py aims at (wsa_or_track_arm_*): one per side of every comparison, bumped where
 * the arm is taken, read only by tests.  win<gap>_{lo,hi}_{in,out}: a peak below / above the track's bin at dist == win - 1 / dist == win (four per gap, in
 * this order: accumulate_fm indexes them) */
#define TRACK_ARMS(X) \
    X(acc_no_peak) X(acc_called) \
    X(gap_neg) X(gap0_in) X(gap1_in) X(gap2_in) X(gap3_in) X(gap4_in) \
    X(win0_lo_in) X(win0_lo_out) X(win0_hi_in) X(win0_hi_out) X(win1_lo_in) X(win1_lo_out) X(win1_hi_in) X(win1_hi_out) \
    X(win2_lo_in) X(win2_lo_out) X(win2_hi_in) X(win2_hi_out) X(win3_lo_in) X(win3_lo_out) X(win3_hi_in) X(win3_hi_out) \
    X(score_pamp_le0) X(score_zero) X(score_le1) X(score_first) X(score_replaces) X(score_below_best) X(score_tie_kept) X(score_inf) \
    X(multi_en_raised) X(multi_st_lowered) X(multi_pb_moved) X(multi_pb_equal_kept) \
    X(upd_above) X(upd_equal) X(upd_below) X(upd_quirk) \
    X(vel_h1) X(vel_h2) X(vel_h3) \
    X(new_above) X(new_equal) X(new_below) \
    X(rank_count1) X(rank_count2) X(rank_mb_lt7) X(rank_mb_eq7) X(rank_mb_tie) \
    X(slot_first_le20) X(slot_first_gt20) X(slot_diff_eq20) X(slot_step) X(slot_fourth) \
    X(str_bump) X(str_bump_int_above) X(str_bump_frac_above) X(str_ref_floor) X(str_ref_floor_eq) X(str_ref_frac_below) X(str_ref_floor_256) \
    X(str_ref_f_eq) X(str_ref_l2) X(str_twice) \
    X(syl_a_u20) X(syl_a_u21) X(syl_b_u10) X(syl_b_u11) X(syl_c_c4) X(syl_c_c5) X(syl_d_u4) X(syl_d_u5) X(syl_short) X(syl_sm_eq_floor)
#define X(a) TARM_##a,
enum { TRACK_ARMS(X) TARM_COUNT };
#undef X
#define X(a) #a,
static const char *const tarm_names[TARM_COUNT] = { TRACK_ARMS(X) };
#undef X
#define TARM(S, a) ((S)->tarms[TARM_##a]++)

/* the arms of the peak scan that tests/peak_cases.py aims at (wsa_or_peak_arm_*; the same names in the same order as tests/peak_ref.py ARMS): one per
 * side of every comparison of the scan and of the shrink, bumped where the arm is taken, read only by tests */
#define PEAK_PRED(X, p) X(p##true_a1) X(p##true_a2) X(p##true_a3plus) X(p##eq_1) X(p##eq_2_alone) X(p##eq_3_alone) X(p##wrong_2) X(p##wrong_3)
#define PEAK_ARMS(X) \
    PEAK_PRED(X, R_) PEAK_PRED(X, F_) \
    X(rise_from_idle) X(rise_closes_candidate) X(rise_leaves_c_1) X(rise_leaves_c_2) X(rise_while_rising) X(close_guard_fails) \
    X(fall_from_rising) X(fall_moves_s) X(fall_while_idle) \
    X(flat_counts_1) X(flat_counts_2) X(flat_timeout) X(flat_timeout_carried_1) X(flat_timeout_carried_2) \
    X(creep_moves_l) X(creep_equal_kept) X(creep_below_kept) X(idle_neither) \
    X(eos_emit) X(eos_after_creep) X(eos_while_falling) X(eos_rise_on_last_bin) X(eos_guard_fails) \
    X(floor_equal_refused) X(floor_below_refused) X(h_2v_not_above) \
    X(shrink_left_0) X(shrink_left_1) X(shrink_left_2) X(shrink_left_3) X(shrink_left_4) X(shrink_left_5plus) X(shrink_left_to_l) \
    X(shrink_right_0) X(shrink_right_1) X(shrink_right_2) X(shrink_right_3) X(shrink_right_4) X(shrink_right_5plus) X(shrink_right_to_l) \
    X(shrink_equal_stops) X(shrink_10k1_floor_goes_on) X(shrink_10k1_ceil_stops) X(shrink_10k9_floor_goes_on) X(shrink_10k9_ceil_stops) X(shrink_big) \
    X(shrink_left_outlasts_right) X(shrink_right_outlasts_left) \
    X(largest_tie_first_kept) X(largest_eos_excluded) X(largest_none) \
    X(g_above_2_32) X(p_cross_inside_shoulder) X(p_cross_at_i_minus_1) X(p_cross_at_s) X(p_high_byte_255) X(cand_64) X(cand_65)
#define X(a) PARM_##a,
enum { PEAK_ARMS(X) PARM_COUNT };
#undef X
#define X(a) #a,
static const char *const parm_names[PARM_COUNT] = { PEAK_ARMS(X) };
#undef X

struct wsa_or_seg {
    wsa_or_cfg cfg;
    /* segmenter state `o` (@B23439) */
    int32_t bands, max_voiced_bin;
    double breaker, min_frames, step_s;
    double cur_frame, no_fm, c_ci;
    int32_t c_started;
    /* noise gate state y, v, x, _, w, T, k (@B24629) */
    double ctx_max, floor_, last_max, last_floor, w, T, k;
    /* tracker module state l, s, c (@B31818) */
    VEC(track_t) tracks;
    double accS, accC;
    int32_t max_peaks, max_live;       /* load of the tracks held now, since clear_fm (wsa_or_segment_load) */
    /* outputs */
    VEC(segment_t) segs;
    VEC(syllable_t) syls;
    int32_t trace_on;
    VEC(double) trace;
    /* what the gate decided (test access, wsa_or_gate_*): per frame the accumulate_fm call, the span bookkeeping of csrc/gate.hip, the arm counters */
    VEC(wsa_or_gate_frame) gframes;
    /* the tracker's table as csrc/tracker_one.hpp holds it between frames (test access, wsa_or_track_frames): entries left by the last accumulate_fm call
     * (tracks not yet 4 filing indices old then, the frame's new ones included), the smallest last_frame among them, whether a stale filing index is set */
    int32_t tbl_n, tbl_min_lf, tbl_stale;
    VEC(int32_t) tframes;
    int32_t span_begin, reset0_in_frame, voiced_now;
    int64_t arms[ARM_COUNT];
    int64_t tarms[TARM_COUNT];
    int64_t parms[PARM_COUNT];
};

static void track_free(track_t *t) {
    VFREE(t->frames); VFREE(t->starts); VFREE(t->ends); VFREE(t->bins); VFREE(t->amps); VFREE(t->energies);
}

/* clear_fm @B35919 */
static void clear_fm(wsa_or_seg *s) {
    for (int32_t i = 0; i < s->tracks.n; i++) track_free(&s->tracks.p[i]);
    s->tracks.n = 0; s->accS = 0; s->accC = 0;
    s->max_peaks = 0; s->max_live = 0;
    s->tbl_n = 0; s->tbl_min_lf = 0; s->tbl_stale = 0;
}

/* L(e) reset_segment @B25649 */
static void reset_segment(wsa_or_seg *s, int32_t started) {
    s->c_ci = 0; s->c_started = started; s->no_fm = 0; clear_fm(s);
    if (started == 0) s->reset0_in_frame = 1;
}

wsa_or_seg *wsa_or_seg_new(const wsa_or_cfg *cfg) {
    wsa_or_seg *s = calloc(1, sizeof(*s));
    s->cfg = *cfg;
    s->bands = cfg->bands;
    s->max_voiced_bin = (int32_t)js_trunc(0.7 * cfg->bands);                 /* @B25136 */
    s->step_s = cfg->window_step / 1e3;
    s->breaker = cfg->pause_length > 2 * cfg->window_step ? cfg->pause_length / cfg->window_step
                                                         : 250 / cfg->window_step;  /* @B25188 */
    s->min_frames = js_trunc(cfg->min_seg_length / cfg->window_step);        /* @B25218 */
    s->c_started = -1;
    if (!(cfg->pause_length > 2 * cfg->window_step)) ARM(s, breaker_rule_250);
    if (cfg->auto_noise_gate) { s->ctx_max = 50; s->floor_ = 2; }           /* @B25471 */
    else {
        s->ctx_max = wsa_or_pow(10, cfg->voiced_max_dB / 20);
        s->floor_ = wsa_or_pow(10, cfg->voiced_min_dB / 20);
    }
    s->last_max = s->ctx_max; s->last_floor = s->floor_;
    return s;
}

void wsa_or_seg_free(wsa_or_seg *s) {
    if (!s) return;
    clear_fm(s); VFREE(s->tracks);
    for (int32_t i = 0; i < s->segs.n; i++) { free(s->segs.p[i].fr); free(s->segs.p[i].sm); free(s->segs.p[i].trk); }
    VFREE(s->segs); VFREE(s->syls); VFREE(s->trace); VFREE(s->gframes); VFREE(s->tframes);
    free(s);
}

/* match score `_` @B37340: (gap, dist, track length, track bin, peak bin, track amp, peak amp, velocity) */
static double match_score(double gap, double dist, double n, double tbin, double pbin, double tamp,
                          double pamp, double vel) {
    double s;
    if (tamp >= pamp) s = pamp / tamp;
    else { if (!(pamp > 0)) return 0; s = tamp / pamp; }
    if (gap == 0) return s > .1 ? 300 * s / dist : 0;
    if (s < .001) return 0;
    if (s >= 1) s = 10; else if (s < .1) s = 1; else s *= 10;
    double t = 10 - fabs(pbin - tbin - vel);
    if (t < 0) return 0;
    if (t < 1) t = 1;
    double i = n;
    if (i > 10) i = 10;
    return 10 / gap * (t * t + i * s);
}

/* test access to the module-private score (fixture tests/golden/score_expected.json) */
double wsa_or_match_score(double gap, double dist, double n, double tbin, double pbin, double tamp, double pamp, double vel) {
    return match_score(gap, dist, n, tbin, pbin, tamp, pamp, vel);
}

/* accumulate_fm `x(e,t,n,r,a)` @B35952 */
static void accumulate_fm(wsa_or_seg *S, const uint32_t *e, const peak_t *pk, int32_t U, double n,
                          double energy, double floor_) {
    static const double win[4] = {3, 4, 6, 9};                                /* @B32325 */
    if (U < 1) { TARM(S, acc_no_peak); return; }
    TARM(S, acc_called);
    int32_t *asg = malloc(sizeof(int32_t) * (size_t)U);
    double *best = malloc(sizeof(double) * (size_t)U);
    for (int32_t o = 0; o < U; o++) { asg[o] = -1; best[o] = 0; }
    S->accS += energy;
    int32_t ntr = S->tracks.n;
    for (int32_t r = 0; r < ntr; r++) {
        track_t *tr = &S->tracks.p[r];
        double gap = n - tr->last_frame;
        if (gap < 0) TARM(S, gap_neg);
        if (gap == 4) for (int32_t o = 0; o < U; o++) if (fabs(tr->last_bin - pk[o].l) < win[3]) TARM(S, gap4_in);
        if (gap >= 0 && gap < 4) {
            double len = tr->frames.n;
            for (int32_t o = 0; o < U; o++) {
                double dist = fabs(tr->last_bin - pk[o].l);
                const int32_t wa = TARM_win0_lo_in + 4 * (int32_t)gap + (pk[o].l > tr->last_bin ? 2 : 0);
                if (dist == win[(int32_t)gap] - 1) S->tarms[wa]++;
                if (dist == win[(int32_t)gap]) S->tarms[wa + 1]++;
                if (dist < win[(int32_t)gap]) {
                    double sc = match_score(gap, dist, len, tr->last_bin, pk[o].l, tr->last_amp,
                                            (double)e[pk[o].l], tr->vel);
                    S->tarms[TARM_gap0_in + (int32_t)gap]++;
                    if (tr->last_amp < (double)e[pk[o].l] && !((double)e[pk[o].l] > 0)) TARM(S, score_pamp_le0);
                    if (sc == 0) TARM(S, score_zero); else if (sc <= 1) TARM(S, score_le1);
                    else if (best[o] == 0) TARM(S, score_first);
                    else if (sc > best[o]) TARM(S, score_replaces);
                    else if (sc == best[o]) TARM(S, score_tie_kept);
                    else TARM(S, score_below_best);
                    if (sc > 1 && isinf(sc)) TARM(S, score_inf);
                    if (sc > 1 && sc > best[o]) { best[o] = sc; asg[o] = r; }
                }
            }
        }
    }
    for (int32_t r = 0; r < ntr; r++) {
        int32_t first = -1;
        for (int32_t o = 0; o < U; o++) if (asg[o] == r) { first = o; break; }
        if (first < 0) continue;
        track_t *tr = &S->tracks.p[r];
        int32_t pb = pk[first].l;
        double amp = e[pb];                              /* read before the arg-max loop (quirk 3) */
        if (amp > floor_) TARM(S, upd_above);
        else {
            if (amp == floor_) TARM(S, upd_equal); else TARM(S, upd_below);
            for (int32_t o = first + 1; o < U; o++) if (asg[o] == r && e[pk[o].l] > floor_) { TARM(S, upd_quirk); break; }
        }
        if (amp > floor_) {
            int32_t st = pk[first].i, en = pk[first].s;
            for (int32_t o = first; o < U; o++) if (asg[o] == r) {
                if (pk[o].s > en) { en = pk[o].s; TARM(S, multi_en_raised); }
                if (pk[o].i < st) { st = pk[o].i; TARM(S, multi_st_lowered); }
                if (o > first && e[pk[o].l] == e[pb]) TARM(S, multi_pb_equal_kept);
                if (e[pk[o].l] > e[pb]) { pb = pk[o].l; TARM(S, multi_pb_moved); }
            }
            double be = 0;
            for (int32_t t = st; t <= en; t++) be += e[t];
            int32_t h = tr->bins.n;
            const double *P = tr->bins.p;
            if (h >= 3) TARM(S, vel_h3); else if (h == 2) TARM(S, vel_h2); else if (h == 1) TARM(S, vel_h1);
            if (h >= 3) tr->vel = (pb - P[h - 1] + (P[h - 2] - P[h - 1]) + (P[h - 3] - P[h - 2])) / 3;
            else if (h == 2) tr->vel = (pb - P[h - 1] + (P[h - 2] - P[h - 1])) / 2;
            else if (h == 1) tr->vel = pb - P[h - 1];
            tr->start = st; tr->end = en; tr->last_frame = n; tr->last_bin = pb; tr->last_amp = amp;
            VPUSH(tr->frames, n); VPUSH(tr->starts, (double)st); VPUSH(tr->ends, (double)en);
            VPUSH(tr->bins, (double)pb); VPUSH(tr->amps, amp); VPUSH(tr->energies, be);
            tr->sumE += be; tr->count += 1; tr->sumEbin += be * pb; tr->sumW += en - st + 1;
            S->accS -= be; S->accC += be;
        }
    }
    for (int32_t o = 0; o < U; o++) if (asg[o] == -1) {
        int32_t pb = pk[o].l;
        double amp = e[pb];
        if (amp > floor_) TARM(S, new_above); else if (amp == floor_) TARM(S, new_equal); else TARM(S, new_below);
        if (amp > floor_) {
            int32_t st = pk[o].i, en = pk[o].s;
            double be = 0;
            for (int32_t t = st; t <= en; t++) be += e[t];
            track_t tr; memset(&tr, 0, sizeof(tr));
            tr.start = st; tr.end = en; tr.last_frame = n; tr.vel = 0; tr.last_bin = pb; tr.last_amp = amp;
            VPUSH(tr.frames, n); VPUSH(tr.starts, (double)st); VPUSH(tr.ends, (double)en);
            VPUSH(tr.bins, (double)pb); VPUSH(tr.amps, amp); VPUSH(tr.energies, be);
            tr.sumE = be; tr.count = 1; tr.sumEbin = be * pb; tr.sumW = en - st + 1;
            VPUSH(S->tracks, tr);
        }
    }
    free(asg); free(best);
    /* the load the device tracker's tables see: peaks handed in, and tracks not yet 4 filing indices old once the frame's new ones are in */
    int32_t live = 0, min_lf = 0;
    for (int32_t r = 0; r < S->tracks.n; r++) if (n - S->tracks.p[r].last_frame < 4) { if (!live || S->tracks.p[r].last_frame < min_lf) min_lf = (int32_t)S->tracks.p[r].last_frame; live++; }
    S->tbl_n = live; S->tbl_min_lf = min_lf;
    if (U > S->max_peaks) S->max_peaks = U;
    if (live > S->max_live) S->max_live = live;
}

/* stats helpers: array_mean_NZ @B2203, only_std_NZ @B1978 / mean_std_NZ @B2089 (= src/stats.js:29-55) */
static double mean_nz(const double *v, int32_t n) {
    double t = 0, c = 0;
    for (int32_t i = 0; i < n; i++) if (v[i] > 0) { t += v[i]; c++; }
    return t / c;
}
static double std_nz(const double *v, int32_t n, double m) {
    double t = 0;
    for (int32_t i = 0; i < n; i++) { double d = v[i] - m; t += d * d; }
    return sqrt(t / n);
}
static double arr_sum(const double *v, int32_t n) {
    double t = 0;
    for (int32_t i = 0; i < n; i++) t += v[i];
    return t;
}

/* formant_features `u(e,t,n)` @B32369; output order @B33436 */
void wsa_or_formant_features(const float *fr, int32_t a, double ctx_max, double floor_, double cs,
                             double x[53]) {
    for (int32_t i = 0; i < 53; i++) x[i] = 0;
    double *c = malloc(sizeof(double) * 6 * (size_t)(a > 0 ? a : 1));
    double *w = c + a, *M = w + a, *T = M + a, *K = T + a, *A = K + a;
    for (int32_t n = 0; n < 3; n++) {
        int32_t b = 5 + 16 * n;
        int32_t prev = 0, m = 0, nA = 0;
        double S = 0, L = 0, cnt = 0, runs = 0, up = 0, dn = 0;
        for (int32_t t = 0; t < a; t++) {
            double r = fr[9 * t + 3 * n], E = fr[9 * t + 3 * n + 1];
            if (r > 0 && E > 0) {
                double wd = fr[9 * t + 3 * n + 2], dB = 20 * wsa_or_log10(E);
                c[m] = r * dB; w[m] = r; M[m] = wd * dB; T[m] = E; K[m] = dB; m++;
                if (prev) {
                    double dl = r - fr[9 * (t - 1) + 3 * n];
                    if (dl > 1) up += dl; else if (dl < -1) dn += -1 * dl;
                    if (E > L) { L = E; S = 1; }
                    else if (S == 1 && E < L / 2) { if (L > 10) A[nA++] = dB; L = 0; S = -1; }
                }
                if (!prev) runs += 1;
                prev = 1; cnt += 1;
            } else { prev = 0; S = 0; L = 0; }
        }
        if (runs > 0) {
            double sT = arr_sum(T, m);
            x[b + 4] = sT / a * 100 / ctx_max;
            x[b + 5] = sT / cnt * 100 / ctx_max;
            double sK = arr_sum(K, m);
            x[b + 0] = arr_sum(c, m) / sK;
            x[b + 1] = std_nz(w, m, mean_nz(w, m));
            x[b + 6] = arr_sum(M, m) / sK;
            double mk = mean_nz(K, m);
            x[b + 2] = mk; x[b + 3] = std_nz(K, m, mk);
            x[b + 11] = nA;
            if (nA > 0) {
                double ma = mean_nz(A, nA);
                x[b + 12] = ma; x[b + 13] = std_nz(A, nA, ma);
                x[b + 14] = 100 * (x[b + 12] / (sK / m) - 1);
            }
        }
        x[b + 7] = cnt; x[b + 8] = runs; x[b + 9] = up; x[b + 10] = dn;
        x[b + 15] = 100 * cnt / a;
    }
    x[0] = a; x[1] = sqrt((double)a); x[2] = cs; x[3] = wsa_or_log10(ctx_max); x[4] = floor_;
    free(c);
}

/* O(e) finalize @B27088 with get_ranked_formants @B35670, straighten_formants @B35074,
 * sep_syllables @B34757, make_syl_features @B34407 */
static void finalize(wsa_or_seg *S, double e) {
    double len_d = e - S->no_fm;
    if (S->c_started >= 2 && len_d == S->min_frames) ARM(S, fin_len_min);
    if (S->c_started >= 2 && len_d == S->min_frames + 1) ARM(S, fin_len_min1);
    if (!(len_d > S->min_frames && S->c_started >= 2)) return;
    int32_t len = (int32_t)len_d;
    int32_t start = (int32_t)(S->cur_frame - len_d);
    int32_t level = S->cfg.level;
    /* ranked(): tracks with count>=2 and mean bin >= 7, stable ascending by mean bin */
    int32_t ntr = S->tracks.n, nr = 0;
    int32_t *rk = malloc(sizeof(int32_t) * (size_t)(ntr > 0 ? ntr : 1));
    for (int32_t t = 0; t < ntr; t++) {
        track_t *tr = &S->tracks.p[t];
        if (tr->count == 1) TARM(S, rank_count1);
        if (tr->count == 2) TARM(S, rank_count2);
        if (tr->count >= 2) {
            double mb = tr->sumEbin / tr->sumE;
            if (mb < 7) TARM(S, rank_mb_lt7);
            if (mb == 7) TARM(S, rank_mb_eq7);
            if (mb >= 7) {
                int32_t r = 0;
                while (r < nr) {
                    track_t *q = &S->tracks.p[rk[r]];
                    if (q->sumEbin / q->sumE > mb) break;
                    if (q->sumEbin / q->sumE == mb) TARM(S, rank_mb_tie);
                    r++;
                }
                memmove(rk + r + 1, rk + r, sizeof(int32_t) * (size_t)(nr - r));
                rk[r] = t; nr++;
            }
        }
    }
    segment_t seg; memset(&seg, 0, sizeof(seg));
    seg.start = start; seg.len = len; seg.syl0 = S->syls.n;
    seg.max_peaks = S->max_peaks; seg.max_live = S->max_live;
    seg.fbegin = S->span_begin; seg.fend = (int32_t)S->cur_frame; seg.cci = (int32_t)S->c_ci;
    seg.g_ctx_max = S->ctx_max; seg.g_floor = S->floor_;
    if (level == 3) {            /* ref @B28273: `u.push([e,a]), ..., s.push(i)` with i = get_ranked_formants() */
        size_t words = 1;
        for (int32_t t = 0; t < nr; t++) words += 10 + 6 * (size_t)S->tracks.p[rk[t]].frames.n;
        double *o = malloc(sizeof(double) * words); size_t w = 0;
        o[w++] = nr;
        for (int32_t t = 0; t < nr; t++) {
            const track_t *tr = &S->tracks.p[rk[t]];
            o[w++] = tr->start; o[w++] = tr->end; o[w++] = tr->last_frame; o[w++] = tr->vel; o[w++] = tr->last_bin; o[w++] = tr->last_amp;
            o[w++] = tr->sumE; o[w++] = tr->count; o[w++] = tr->sumEbin; o[w++] = tr->sumW;
            const int32_t c = tr->frames.n;
            for (int32_t q = 0; q < c; q++) o[w++] = tr->frames.p[q];
            for (int32_t q = 0; q < c; q++) o[w++] = tr->starts.p[q];
            for (int32_t q = 0; q < c; q++) o[w++] = tr->ends.p[q];
            for (int32_t q = 0; q < c; q++) o[w++] = tr->bins.p[q];
            for (int32_t q = 0; q < c; q++) o[w++] = tr->amps.p[q];
            for (int32_t q = 0; q < c; q++) o[w++] = tr->energies.p[q];
        }
        seg.trk = o; seg.trk_n = (int32_t)words;
        VPUSH(S->segs, seg); free(rk); return;
    }
    /* straighten(): the reference pushes segments_ci BEFORE straighten can throw (@B27240); a frame
     * index >= len would be a TypeError there -> segment kept in segments_ci without results.
     * Provably unreachable; flagged through has_feat = -1 if it ever happens. */
    float *fr = calloc((size_t)len * 9, sizeof(float));
    float *sm = calloc((size_t)len * 3, sizeof(float));
    double last = 0; int32_t slot = 0, bad = 0;
    for (int32_t t = 0; t < nr && !bad; t++) {
        track_t *tr = &S->tracks.p[rk[t]];
        double mb = tr->sumEbin / tr->sumE;
        if (t == 0) { if (mb <= 20) TARM(S, slot_first_le20); else TARM(S, slot_first_gt20); }
        else if (fabs(mb - last) == 20) TARM(S, slot_diff_eq20);
        else if (fabs(mb - last) > 20) TARM(S, slot_step);
        if (fabs(mb - last) > 20 && slot + 1 >= 3) TARM(S, slot_fourth);
        if (fabs(mb - last) > 20) { last = mb; slot++; if (slot >= 3) break; }
        for (int32_t i = 0; i < (int32_t)tr->count; i++) {
            int32_t l = slot;
            double f = tr->bins.p[i];
            if (f > 0) {
                double E = tr->energies.p[i];
                int32_t d = (int32_t)tr->frames.p[i];
                double wd = tr->ends.p[i] - tr->starts.p[i] + 1;
                if (d >= len || d < 0) { bad = 1; break; }
                {
                    const double cur = fr[9 * d + 3 * l], fl = S->floor_;
                    if (cur > fl && cur < f && l < 2) {
                        TARM(S, str_bump);
                        if (fl == floor(fl) && cur == fl + 1) TARM(S, str_bump_int_above);
                        if (fl != floor(fl) && cur == floor(fl) + 1) TARM(S, str_bump_frac_above);
                    } else if (cur > 0) {
                        if (cur <= fl && cur < f && l < 2) {
                            TARM(S, str_ref_floor);
                            if (cur == fl) TARM(S, str_ref_floor_eq);
                            if (fl != floor(fl) && cur == floor(fl)) TARM(S, str_ref_frac_below);
                            if (fl >= 256) TARM(S, str_ref_floor_256);
                        }
                        if (cur > fl && cur == f && l < 2) TARM(S, str_ref_f_eq);
                        if (cur > fl && cur < f && l == 2) TARM(S, str_ref_l2);
                    }
                }
                if (fr[9 * d + 3 * l] > S->floor_ && fr[9 * d + 3 * l] < f && l < 2) l++;
                if (fr[9 * d + 3 * l] != 0) TARM(S, str_twice);
                fr[9 * d + 3 * l] = (float)f; fr[9 * d + 3 * l + 1] = (float)E; fr[9 * d + 3 * l + 2] = (float)wd;
                sm[3 * d + 0] = (float)((double)sm[3 * d + 0] + f * E);
                sm[3 * d + 1] = (float)((double)sm[3 * d + 1] + E);
                sm[3 * d + 2] = (float)((double)sm[3 * d + 2] + wd * E);
            }
        }
    }
    free(rk);
    if (bad) { seg.has_feat = -1; free(fr); free(sm); VPUSH(S->segs, seg); return; }
    double cs = S->accC / S->accS;
    if (level == 5) {
        wsa_or_formant_features(fr, len, S->ctx_max, S->floor_, cs, seg.feat);
        seg.has_feat = 1;
    }
    if (level == 10 || level == 13) {
        int32_t i = -1; double c = 0, u = 0;
        for (int32_t e2 = 0; e2 < len; e2++) {
            if (sm[3 * e2 + 1] == S->floor_) TARM(S, syl_sm_eq_floor);
            if (sm[3 * e2 + 1] > S->floor_) { c = 0; u++; if (i < 0) i = e2; } else c++;
            if (e2 < len - 1) {               /* each close condition at its two boundary values, where no other condition closes */
                if (c == 1 && u == 20) TARM(S, syl_a_u20);
                if (c == 1 && u == 21) TARM(S, syl_a_u21);
                if (c == 2 && u == 10) TARM(S, syl_b_u10);
                if (c == 2 && u == 11) TARM(S, syl_b_u11);
                if (c == 4 && u > 0 && u <= 10) TARM(S, syl_c_c4);
                if (c == 5 && u > 0 && u <= 10) TARM(S, syl_c_c5);
            } else if (c == 0) {
                if (u == 4) TARM(S, syl_d_u4);
                if (u == 5) TARM(S, syl_d_u5);
            }
            if ((u > 20 && c > 0) || (u > 10 && c > 1) || (u > 0 && c > 4) || (e2 >= len - 1 && u > 4)) {
                int32_t t = e2 - (int32_t)c;
                if (!(t - i > 1)) TARM(S, syl_short);
                if (t - i > 1) {
                    syllable_t sy; memset(&sy, 0, sizeof(sy));
                    sy.seg = S->segs.n; sy.start = i; sy.len = t - i;
                    if (level == 13)
                        wsa_or_formant_features(fr + 9 * i, t - i, S->ctx_max, S->floor_, cs, sy.feat);
                    VPUSH(S->syls, sy);
                    i = -1; u = 0;
                }
            }
        }
        seg.nsyl = S->syls.n - seg.syl0;
    }
    seg.fr = fr; seg.sm = sm;
    VPUSH(S->segs, seg);
}

/* auto noise gate C(h) @B28506 */
static void noise_gate(wsa_or_seg *S, double h) {
    S->w++;
    if (S->w == 40 && h <= S->ctx_max && h > 2 * S->floor_) ARM(S, gate_w40);
    if (h > S->ctx_max || (S->w > 40 && h > 2 * S->floor_)) {
        if (!(h > S->ctx_max) && S->w == 41) ARM(S, gate_w41);
        if (h >= S->ctx_max) {
            if (h > S->ctx_max) ARM(S, gate_raise_above); else ARM(S, gate_raise_equal_w);
            S->w = 0; S->last_max = S->ctx_max = h;
        }
        else if (h > S->last_max / 100) {
            ARM(S, gate_decay);
            if (100 * h == S->last_max + 1) ARM(S, gate_decay_edge);
            S->ctx_max -= js_trunc(S->ctx_max / 8); S->w = 35;
        } else {
            ARM(S, gate_neither);
            if (100 * h == S->last_max) ARM(S, gate_decay_refused_equal);
        }
        double y = S->ctx_max, t = wsa_or_log10(y), v;
        if (t > 7) { v = js_trunc(wsa_or_pow(10, t - 3) / 20); ARM(S, floor_t7); }
        else if (t > 6) { v = js_trunc(wsa_or_pow(10, t - 3) / 2); ARM(S, floor_t6); }
        else if (t > 4) { v = js_trunc(wsa_or_pow(10, t - 2) / 2); ARM(S, floor_t4); }
        else if (t > 2) { v = js_trunc(wsa_or_pow(10, t / 3)); ARM(S, floor_t2); }
        else if (t > 1) { v = js_trunc(y / 10); ARM(S, floor_t1); }
        else { v = 1; ARM(S, floor_one); }
        S->floor_ = v; S->last_floor = v;
        if (S->k > 0 && S->T / S->k == 30 * v) ARM(S, tk_equal);
        if (S->k > 0 && S->T / S->k < 30 * v) {
            if (S->voiced_now) ARM(S, tk_reset_voiced); else ARM(S, tk_reset_unvoiced);
            reset_segment(S, 0); S->k = 0; S->T = 0;
        }
        S->T += S->ctx_max; S->k += 1;
    } else if (S->floor_ > 10 && S->floor_ > S->last_floor / 10 && S->w > 20) {
        if (S->w == 21) ARM(S, decay_first_w21);
        if (js_trunc(S->last_floor / 20) == 0) ARM(S, decay_zero_step);
        S->floor_ -= js_trunc(S->last_floor / 20);
        if (S->floor_ < 10) { S->floor_ = 10; ARM(S, decay_clamp10); }
    } else if (S->w > 20 && S->floor_ < S->last_floor) ARM(S, decay_stop);      /* a decay that has run into max(10, last_floor / 10) */
}

/* The scan of the frame loop D() @B25827 on its own: the candidates [i, s, l] of frame e that pass `e[l] > v`, after the /10 shoulder shrink, and
 * n, p, h, d, g as the loop hands them on.  A negative v keeps every candidate (amplitudes are unsigned), which is the table csrc/peaks.hip writes.
 * `last` (may be NULL) marks the end-of-spectrum emission, psum (may be NULL) takes the exact P[i - 1] and P[s] per candidate, A the arm counts. */
typedef struct { int32_t n, p, raw, n_early; double h, d, g, d_early; } scan_t;

static void scan_count_pred(const uint32_t *e, int32_t a, int above, int64_t *A) {
    const uint32_t ea = e[a];
#define CMP(x, y) (above ? (x) > (y) : (x) < (y))
    if (ea == e[a - 1]) { A[3]++; return; }
    if (!CMP(ea, e[a - 1])) return;
    const int ok2 = a < 2 || CMP(ea, e[a - 2]), ok3 = a < 3 || CMP(ea, e[a - 3]);
    if (a >= 2 && !ok2) { if (ea != e[a - 2]) A[6]++; else if (ok3) A[4]++; }
    if (ok2 && !ok3) A[ea == e[a - 3] ? 5 : 7]++;
    if (ok2 && ok3) A[a == 1 ? 0 : a == 2 ? 1 : 2]++;
#undef CMP
}

/* the arms of one step of the shrink's walk: e[x] against e[l] / 10 */
static void scan_count_shrink(const uint32_t *e, int32_t x, int32_t l, int64_t *A) {
    const uint32_t ex = e[x], el = e[l], k = el / 10, m = el % 10;
    if (ex >= 429496730u) A[PARM_shrink_big]++;
    if (m == 0 && ex == k) A[PARM_shrink_equal_stops]++;
    if (m == 1 && ex == k) A[PARM_shrink_10k1_floor_goes_on]++;
    if (m == 1 && ex == k + 1) A[PARM_shrink_10k1_ceil_stops]++;
    if (m == 9 && ex == k) A[PARM_shrink_10k9_floor_goes_on]++;
    if (m == 9 && ex == k + 1) A[PARM_shrink_10k9_ceil_stops]++;
}

static void scan_frame(const uint32_t *e, int32_t B, double v, peak_t *pk, uint8_t *last, uint64_t *psum, scan_t *o, int64_t *A) {
    int32_t n = 0, i = 0, l = 0, s = 0, c = 0, u = 0, p = 0, c0 = 0;
    double d = 0, h = v < 0 ? 0 : 2 * v, g = 0;            /* (every candidate kept: the largest starts from 0, as the device's header does) */
    int32_t raw = 0, n_early = 0; double d_early = 0;     /* tests only: candidates by geometry alone (the device's table order); accepted ones among the first 16 */
    uint64_t *P = malloc(sizeof(uint64_t) * (size_t)(B > 0 ? B : 1));
    { uint64_t t = 0; for (int32_t a = 0; a < B; a++) { t += e[a]; P[a] = t; } }
#define PA(a) (A[PARM_##a]++)
#define EMIT(upd) do { \
        if (!(e[l] > v)) { if (e[l] == v) PA(floor_equal_refused); else PA(floor_below_refused); break; } \
        if (raw - 1 < 16) { n_early++; d_early += e[l]; } \
        if (upd) { if (p > 0 && e[l] == h) PA(largest_tie_first_kept); if (v >= 0 && p == 0 && !(e[l] > h)) PA(h_2v_not_above); } \
        else if (e[l] > h) PA(largest_eos_excluded); \
        if ((upd) && e[l] > h) { h = e[l]; p = l; } \
        double thr = e[l] / 10.0; int32_t nl = 0, nr = 0; \
        while (i < l && (scan_count_shrink(e, i, l, A), e[i] < thr)) { i++; nl++; } \
        while (s > l && (scan_count_shrink(e, s, l, A), e[s] < thr)) { s--; nr++; } \
        A[PARM_shrink_left_0 + (nl < 5 ? nl : 5)]++; if (i == l) PA(shrink_left_to_l); \
        A[PARM_shrink_right_0 + (nr < 5 ? nr : 5)]++; if (s == l) PA(shrink_right_to_l); \
        if (nl > nr) PA(shrink_left_outlasts_right); else if (nr > nl) PA(shrink_right_outlasts_left); \
        { const uint64_t pi = i > 0 ? P[i - 1] : 0, ps = P[s]; \
          if (ps >> 32 != pi >> 32) PA(p_cross_inside_shoulder); \
          if (i > 0 && pi >> 32 != (i > 1 ? P[i - 2] : 0) >> 32) PA(p_cross_at_i_minus_1); \
          if (ps >> 32 != P[s - 1] >> 32) PA(p_cross_at_s); \
          if (ps >> 32 == 255) PA(p_high_byte_255); \
          if (psum) { psum[2 * n] = pi; psum[2 * n + 1] = ps; } } \
        if (last) last[n] = !(upd); \
        pk[n].i = i; pk[n].s = s; pk[n].l = l; n++; d += e[l]; } while (0)
    for (int32_t a = 1; a < B; a++) {                                          /* @B25827 */
        g += e[a];
        scan_count_pred(e, a, 1, A + PARM_R_true_a1);
        if (e[a] > e[a - 1] && (a < 2 || e[a] > e[a - 2]) && (a < 3 || e[a] > e[a - 3])) {
            if (a == B - 1) PA(eos_rise_on_last_bin);
            if (u == -1 || u == 0) {
                if (u == 0) PA(rise_from_idle);
                else if (i <= l && l < s) { PA(rise_closes_candidate); if (c == 1) PA(rise_leaves_c_1); else if (c == 2) PA(rise_leaves_c_2); }
                else PA(close_guard_fails);
                if (u == -1 && i <= l && l < s) { raw++; EMIT(1); }
                i = a - 1; l = a;
            } else if (u == 1) { l = a; PA(rise_while_rising); }
            u = 1;
        } else if (scan_count_pred(e, a, 0, A + PARM_F_true_a1), e[a] < e[a - 1] && (a < 2 || e[a] < e[a - 2]) && (a < 3 || e[a] < e[a - 3])) {
            if (u == 1) { PA(fall_from_rising); c0 = c; } else if (u == -1) PA(fall_moves_s); else PA(fall_while_idle);
            if (u == 1 || u == -1) { s = a; u = -1; }
        } else if (u == -1) {
            c++;
            if (c == 1) PA(flat_counts_1); else if (c == 2) PA(flat_counts_2);
            if (c > 2) {
                c = 0;
                if (i <= l && l < s) { PA(flat_timeout); if (c0 == 1) PA(flat_timeout_carried_1); else if (c0 == 2) PA(flat_timeout_carried_2); } else PA(close_guard_fails);
                if (i <= l && l < s) { raw++; EMIT(1); }
                u = 0;
            }
        } else if (u == 1 && e[a] > e[a - 1]) { l = a; PA(creep_moves_l); }
        else if (u == 1) { if (e[a] == e[a - 1]) PA(creep_equal_kept); else PA(creep_below_kept); }
        else PA(idle_neither);
        if (a == B - 1 && u == -1) PA(eos_while_falling);
        if (a == B - 1 && u == 1) {
            const int crept = l != a && e[l] > e[a];
            s = a; l = a;
            if (i < l && l <= s) { PA(eos_emit); if (crept) PA(eos_after_creep); } else PA(eos_guard_fails);
            if (i < l && l <= s) { raw++; EMIT(0); }
        }
    }
#undef EMIT
    if (g >= 4294967296.0) PA(g_above_2_32);
    if (p == 0) PA(largest_none);
    if (n == 64) PA(cand_64);
    if (n > 64) PA(cand_65);
#undef PA
    free(P);
    o->n = n; o->p = p; o->raw = raw; o->n_early = n_early; o->h = h; o->d = d; o->g = g; o->d_early = d_early;
}

/* spectrum_push I(e,t) @B30392 (levels > 2) followed by one pass of the frame loop D() @B25717 */
void wsa_or_seg_push(wsa_or_seg *S, const uint32_t *e) {
    const int32_t B = S->bands;
    S->cur_frame++;
    double t = S->c_ci;                           /* captured before the start test (quirk 1) */
    double v = S->floor_;
    peak_t *pk = malloc(sizeof(peak_t) * (size_t)(B > 0 ? B : 1));
    scan_t sc;
    scan_frame(e, B, v, pk, NULL, NULL, &sc, S->parms);
    const int32_t n = sc.n, p = sc.p, n_early = sc.n_early;
    const double d = sc.d, h = sc.h, g = sc.g, d_early = sc.d_early;
    /* ---- what the arms below are counted from (tests only; nothing here feeds the state) */
    const double mvb = S->max_voiced_bin;
    const double d16 = d_early; const int32_t n16 = n_early;
    int32_t ties = 0;                                      /* (a candidate sits on bin B - 1 only as the end-of-spectrum emission, which is not in h / p) */
    for (int32_t o = 0; o < n; o++) if (p > 0 && pk[o].l != B - 1 && e[pk[o].l] == h) ties++;
    if (n > 0 && pk[n - 1].l == B - 1 && e[B - 1] > h) ARM(S, hdr_eos_largest);
    if (ties > 1) ARM(S, hdr_tie);
    if (n == 16) ARM(S, cand_16);
    if (n == 17) ARM(S, cand_17);
    if (n == 64) ARM(S, cand_64);
    S->reset0_in_frame = 0;
    wsa_or_gate_frame rec = {0, (int32_t)t, 0, v, v};
    if (S->c_started < 0) {                                                    /* @B26527 */
        double r = d > h ? h * (n - 1) / (d - h) : 0;
        const int c_n = n > 4, c_lo = p > 7, c_hi = p < S->max_voiced_bin, c_r = r > 4;
        if (n > 0 && c_lo && c_hi && c_n && c_r) {
            ARM(S, start_pass);
            if (n == 5) ARM(S, start_n5);
            if (p == 8) ARM(S, start_p8);
            if (p == mvb - 1) ARM(S, start_pmax_m1);
            if (h * (n - 1) - 4 * (d - h) == 1) ARM(S, start_r_above);
            if (n16 <= 4) ARM(S, late_n4);
        } else {
            if (n == 4 && c_lo && c_hi && d > h && h * (n - 1) > 4 * (d - h)) ARM(S, start_n4);
            if (p == 7 && c_n && c_r) ARM(S, start_p7);
            if (p == mvb && c_n && c_r) ARM(S, start_pmax);
            if (c_n && c_lo && c_hi && d > h && h * (n - 1) == 4 * (d - h)) ARM(S, start_r_equal);
        }
        if (n > 0 && p > 7 && p < S->max_voiced_bin && n > 4 && r > 4) { reset_segment(S, 0); S->span_begin = (int32_t)S->cur_frame - 1; }
        else S->no_fm++;
    }
    int32_t do_reset = 0, gate_reset = 0;
    if (S->c_started >= 0) {                                                   /* @B26646 */
        const int unv = n == 0 || p < 7 || p >= S->max_voiced_bin || (n > 3 && d / (g - d) < .1);
        if (n == 0) ARM(S, voiced_n0);
        else if (p == 0) ARM(S, voiced_p0);
        else if (p == 6) ARM(S, voiced_p6);
        else if (p == mvb) ARM(S, voiced_pmax);
        else if (p >= 7 && p < mvb) {
            if (p == 7 && !unv) ARM(S, voiced_p7);
            if (p == mvb - 1 && !unv) ARM(S, voiced_pmax_m1);
            if (n > 3 && 11 * d == g) ARM(S, d_equal);
            if (n > 3 && 11 * d == g - 1) ARM(S, d_below);
            if (n == 3 && 11 * d < g) ARM(S, d_n3);
            if (n > 3 && g == d) ARM(S, d_g_equals_d);
            if (11 * h >= g) ARM(S, mx_covers);
            else if (n <= 3) ARM(S, mx_short_n3);
            else if (g <= 11 * d) ARM(S, mx_short_d_covers);
            if (n > 3 && n16 <= 3 && unv) ARM(S, late_n3);
            if (n > 3 && n > n16 && 11 * h < g && 11 * d16 < g && g <= 11 * d) ARM(S, late_d);
        }
        if (unv) S->arms[ARM_unvoiced_at_0 + S->c_started]++;          /* c_started is 0, 1 or 2 here */
        else if (S->c_started < 2) S->arms[ARM_voiced_at_0 + S->c_started]++;
        S->voiced_now = !unv;
        if (n == 0 || p < 7 || p >= S->max_voiced_bin || (n > 3 && d / (g - d) < .1)) {
            S->no_fm++;
            if (S->c_started < 2) S->c_started--;
            else if (S->no_fm >= S->breaker) {
                if (S->breaker == trunc(S->breaker)) ARM(S, pause_int); else ARM(S, pause_frac);
                finalize(S, S->c_ci + 1); do_reset = 1;
            }
            else if (S->cfg.auto_noise_gate) { noise_gate(S, h); if (S->reset0_in_frame) { S->span_begin = (int32_t)S->cur_frame; gate_reset = 1; } }
        } else {
            if (S->cfg.auto_noise_gate) { const int32_t before = S->reset0_in_frame; noise_gate(S, h); if (S->reset0_in_frame && !before) { S->span_begin = (int32_t)S->cur_frame - 1; gate_reset = 1; } }
            rec.called = 1; rec.stale = S->reset0_in_frame; rec.fl = S->floor_;
            accumulate_fm(S, e, pk, n, t, g, S->floor_);
            if (rec.stale) S->tbl_stale = 1;
            if (S->c_started < 2) S->c_started++; else S->no_fm = 0;
        }
    }
    if (!rec.called) rec.fl = S->floor_;
    VPUSH(S->gframes, rec);
    if (S->trace_on) {
        double row[10] = {S->c_ci, (double)S->c_started, S->no_fm, S->ctx_max, S->floor_, (double)n,
                          (double)p, h, d, g};
        for (int k = 0; k < 10; k++) VPUSH(S->trace, row[k]);
    }
    S->c_ci++;
    /* the reference resets in the Promise .then microtask, i.e. after the frame completes (quirk 8) */
    if (do_reset) { reset_segment(S, -1); S->span_begin = (int32_t)S->cur_frame; }
    { const int32_t row[5] = {S->tbl_n, S->tbl_min_lf, S->tbl_stale, S->tracks.n, gate_reset}; for (int k = 0; k < 5; k++) VPUSH(S->tframes, row[k]); }
    free(pk);
}

/* segment_truncate N() @B30757 -> D() with play_end -> O(c_ci) -> L(1) */
void wsa_or_seg_finish(wsa_or_seg *S) {
    const int32_t before = S->segs.n;
    if (S->c_started < 2 && S->c_started >= 0 && S->c_ci - S->no_fm > S->min_frames) ARM(S, fin_end_unstarted);
    finalize(S, S->c_ci);
    if (S->segs.n > before) ARM(S, fin_truncate_open);
    reset_segment(S, 1); S->span_begin = (int32_t)S->cur_frame;
}

/* What csrc/gate.hip does when a stream's open span would outgrow its ring (DESIGN.md "streams"; our own rule, not the reference's): the body of
 * segment_truncate, O(c_ci) then L(1), after which pushes go on */
void wsa_or_seg_cut(wsa_or_seg *S) {
    ARM(S, ring_cut);
    finalize(S, S->c_ci);
    reset_segment(S, 1); S->span_begin = (int32_t)S->cur_frame;
}

int32_t wsa_or_gate_n_frames(const wsa_or_seg *s) { return s->gframes.n; }
const wsa_or_gate_frame *wsa_or_gate_frames(const wsa_or_seg *s) { return s->gframes.p; }
void wsa_or_gate_segment(const wsa_or_seg *s, int32_t i, int32_t out3[3], double out2[2]) {
    const segment_t *g = &s->segs.p[i];
    out3[0] = g->fbegin; out3[1] = g->fend; out3[2] = g->cci; out2[0] = g->g_ctx_max; out2[1] = g->g_floor;
}
void wsa_or_gate_state(const wsa_or_seg *s, double out[12]) {
    out[0] = s->cur_frame; out[1] = s->no_fm; out[2] = s->c_ci; out[3] = s->c_started; out[4] = s->ctx_max; out[5] = s->floor_;
    out[6] = s->last_max; out[7] = s->last_floor; out[8] = s->w; out[9] = s->T; out[10] = s->k; out[11] = s->span_begin;
}
int32_t wsa_or_gate_n_arms(void) { return ARM_COUNT; }
const char *wsa_or_gate_arm_name(int32_t i) { return i >= 0 && i < ARM_COUNT ? arm_names[i] : NULL; }
int64_t wsa_or_gate_arm_count(const wsa_or_seg *s, int32_t i) { return i >= 0 && i < ARM_COUNT ? s->arms[i] : -1; }

int32_t wsa_or_track_n_arms(void) { return TARM_COUNT; }
const char *wsa_or_track_arm_name(int32_t i) { return i >= 0 && i < TARM_COUNT ? tarm_names[i] : NULL; }
int64_t wsa_or_track_arm_count(const wsa_or_seg *s, int32_t i) { return i >= 0 && i < TARM_COUNT ? s->tarms[i] : -1; }
const int32_t *wsa_or_track_frames(const wsa_or_seg *s) { return s->tframes.p; }

int32_t wsa_or_peak_n_arms(void) { return PARM_COUNT; }
const char *wsa_or_peak_arm_name(int32_t i) { return i >= 0 && i < PARM_COUNT ? parm_names[i] : NULL; }
int64_t wsa_or_peak_arm_count(const wsa_or_seg *s, int32_t i) { return i >= 0 && i < PARM_COUNT ? s->parms[i] : -1; }

/* the scan of one frame without a segmenter (tests/peak_cases.py): cand [bands][4] = i, s, l, last; out5 = n, p, h, d, g; psum [bands][2] = P[i - 1], P[s];
 * arms [wsa_or_peak_n_arms()] is added to.  v < 0 keeps every candidate.  Returns n. */
int32_t wsa_or_scan_frame(const uint32_t *e, int32_t bands, double v, int32_t *cand, double *out5, uint64_t *psum, int64_t *arms) {
    int64_t own[PARM_COUNT] = {0};
    peak_t *pk = malloc(sizeof(peak_t) * (size_t)(bands > 0 ? bands : 1));
    uint8_t *last = calloc((size_t)(bands > 0 ? bands : 1), 1);
    scan_t sc;
    scan_frame(e, bands, v, pk, last, psum, &sc, arms ? arms : own);
    for (int32_t k = 0; cand && k < sc.n; k++) { cand[4 * k] = pk[k].i; cand[4 * k + 1] = pk[k].s; cand[4 * k + 2] = pk[k].l; cand[4 * k + 3] = last[k]; }
    if (out5) { out5[0] = sc.n; out5[1] = sc.p; out5[2] = sc.h; out5[3] = sc.d; out5[4] = sc.g; }
    free(pk); free(last);
    return sc.n;
}

int32_t wsa_or_n_segments(const wsa_or_seg *s) { return s->segs.n; }
void wsa_or_segment(const wsa_or_seg *s, int32_t i, int32_t out[5]) {
    const segment_t *g = &s->segs.p[i];
    out[0] = g->start; out[1] = g->len; out[2] = g->syl0; out[3] = g->nsyl; out[4] = g->has_feat;
}
void wsa_or_segment_load(const wsa_or_seg *s, int32_t i, int32_t out[2]) {
    out[0] = s->segs.p[i].max_peaks; out[1] = s->segs.p[i].max_live;
}
const double *wsa_or_segment_features(const wsa_or_seg *s, int32_t i) { return s->segs.p[i].feat; }
const float *wsa_or_segment_formants(const wsa_or_seg *s, int32_t i) { return s->segs.p[i].fr; }
const float *wsa_or_segment_sums(const wsa_or_seg *s, int32_t i) { return s->segs.p[i].sm; }
const double *wsa_or_segment_tracks(const wsa_or_seg *s, int32_t i, int32_t *n) { *n = s->segs.p[i].trk_n; return s->segs.p[i].trk; }
int32_t wsa_or_n_syllables(const wsa_or_seg *s) { return s->syls.n; }
void wsa_or_syllable(const wsa_or_seg *s, int32_t j, int32_t out[3]) {
    const syllable_t *y = &s->syls.p[j];
    out[0] = y->seg; out[1] = y->start; out[2] = y->len;
}
const double *wsa_or_syllable_features(const wsa_or_seg *s, int32_t j) { return s->syls.p[j].feat; }
int32_t wsa_or_trace_len(const wsa_or_seg *s) { return s->trace.n / 10; }
const double *wsa_or_trace(const wsa_or_seg *s) { return s->trace.p; }
void wsa_or_enable_trace(wsa_or_seg *s, int32_t on) { s->trace_on = on; }

wsa_or_seg *wsa_or_run_clip(const wsa_or_cfg *cfg, const uint32_t *spectra, int32_t frames) {
    wsa_or_seg *s = wsa_or_seg_new(cfg);
    for (int32_t f = 0; f < frames; f++) wsa_or_seg_push(s, spectra + (size_t)f * (size_t)cfg->bands);
    wsa_or_seg_finish(s);
    return s;
}
