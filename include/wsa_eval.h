/*
 * wsa_eval.h — C ABI of libwsa, the evaluation of a labelled feature DB (additions within version 5 of wsa.h: probe for
 * wsa_dbstats_confusion).  Specification EV-1 and kernels K8e of DESIGN.md (csrc/dbeval.hip).
 *
 * wsa_dbstats_table (wsa.h, DS-1) gives what the application's results panel gives.  These entries give, on the same wsa_dbstats object
 * and from the same columns, what the panel cannot say: which class is taken for which (a confusion matrix per categorical head) and how
 * well an ordinal head's predictions agree with its labels (means, variances, covariance, Lin's concordance correlation coefficient and
 * Pearson's r).  The arithmetic of the agreement is the reference's own: only_mean, variance and covariance of src/stats.js:80-113
 * (two passes, population forms) and the CCC expression of calc_ccc (src/neuralmodel.js:488), which the reference leaves "under
 * construction" with its call commented out; calc_ccc passes covariance(y1, y1), EV-1 uses (y1, y2).
 * Counts are integers and exact.  Every f64 sum is "rows of a chunk of WSA_DBSTATS_CHUNK_ROWS consecutive rows in row order, then chunks
 * in chunk order", no product is fused into an addition, and there are no floating-point atomics: a run is reproducible bit for bit and a
 * CPU restatement gives the same bits.  The entries change no column and nothing wsa_dbstats_table reads or writes.  Pass the SAME
 * stream as to every other call on the object.
 * These declarations live beside wsa.h, not in it: the set of entries wsa.h declares is pinned, name by name and by count
 * (tests/test_abi.py against capi.ABI_TABLE); this header is held to capi.EVAL_TABLE in the same way (tests/test_dbeval_host.py).
 */
#ifndef WSA_EVAL_H
#define WSA_EVAL_H
#include "wsa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* one ordinal head.  A row takes part when its true AND its predicted value pass DS-1's device rule (v == v && v != 0), so n is
 * wsa_dbstats_ord.pred_n.  mean = sum / n; var = sum (a - mean)^2 / n; cov = sum (t - mean_true)(p - mean_pred) / n;
 * ccc = 2 cov / (var_true + var_pred + (mean_pred - mean_true)^2); pearson = cov / sqrt(var_true var_pred).
 * n == 0 leaves every double NaN; 0 / 0 stays NaN (zero variance: pearson, and ccc when the means are equal too). */
typedef struct { uint64_t n; double mean_true, mean_pred, var_true, var_pred, cov, ccc, pearson; } wsa_dbstats_agree;

/* the confusion matrix of categorical head `head`, m [V][V + 1] (host): over the rows DS-1 counts (true_idx >= 0), m[t][p] = the rows
 * of true class t predicted as p; column V collects the blank predictions.  Row t sums to cls[t].count, m[t][t] = cls[t].correct, the
 * rest of columns 0 .. V - 1 sums to cls[t].wrong, column V sums to cat.blank.  Two launches; synchronises `stream`.  The first call
 * allocates the workspace. */
wsa_status wsa_dbstats_confusion(wsa_dbstats *db, uint32_t head, void *stream, uint64_t *m);
/* the agreement of every ordinal head, out [n_ord] (host).  Four launches (the sums, the means, the central sums, the quotients); the
 * third reads the means from device memory.  Synchronises `stream`.  The first call allocates the workspace.  WSA_ERR_INVALID: a DB
 * without an ordinal head. */
wsa_status wsa_dbstats_agreement(wsa_dbstats *db, void *stream, wsa_dbstats_agree *out);

/*
 * ---- Per file.  The labels of the corpora these DBs hold belong to a file, and the application's own answer for a file is the
 * per-launch fold of src/prediction.js:86-169: Label_conf_all (the gauges) and, for V / A / D, the running value.  K6b and RG-1 (wsa.h)
 * implement that fold for batches and streams; these entries run the same device code (csrc/classify_fold.hpp, csrc/regress_fold.hpp)
 * over the rows of a stored DB, with a file where a batch has a clip, and then evaluate the files as rows: table, confusion, agreement.
 */
/* host [n_rows] columns: file_of_row -1 (the row belongs to no file) or 0 .. n_files - 1, non-decreasing over the rows that have a file
 * (a DB holds a file's rows together, in insertion order); callback_of_row the integer part of the row's `seg` tag, the callback (si)
 * the row came from: consecutive rows of a file with the same value form one callback.  The fold takes its weights from whole
 * milliseconds: a duration k / 1000 is reproduced exactly (every level-12 / 13 DB: durations are toFixed(3) strings).  A file's duration
 * is the sum of its rows' durations in row order.  Creates the file-level tables; synchronous; set once.
 * WSA_ERR_INVALID with a message, the object left as it was: a file outside -1 .. n_files - 1 or a decreasing file (naming the first
 * offending row), a duration of a row with a file that is not a whole number of milliseconds (naming the row), n_files 0, a second call. */
wsa_status wsa_dbstats_set_files(wsa_dbstats *db, const int32_t *file_of_row, const int32_t *callback_of_row, uint32_t n_files);
/* host [n_files]: a file's true class (-1: the file does not count) / true value (NaN: missing) of head `head`.  Which label a file
 * has is the host's rule (webspeechanalyzer_amd.dbstats: the label of the file's first counted row).  The predicted column stays. */
wsa_status wsa_dbstats_set_file_classes(wsa_dbstats *db, uint32_t head, const int32_t *true_idx);
wsa_status wsa_dbstats_set_file_values(wsa_dbstats *db, uint32_t head, const double *true_value);
/* after wsa_dbstats_predict_classes(db, head, ..), on the probabilities that call kept: per file what K6b leaves for a clip whose rows
 * are the file's rows — fold_callback per callback; acc_all (Label_conf_all) per class at the file's end are the file's meter sums.
 * The file's predicted class is ours: the largest sum above 0, the first in the fold's own key order (Object.keys) on a tie, through
 * that call's legend_to_vocab; blank when no sum is above 0.  Only enqueues (the first call allocates).
 * WSA_ERR_INVALID: no files, no kept prediction, or the kept one is another head's. */
wsa_status wsa_dbstats_fold_files(wsa_dbstats *db, uint32_t head, void *stream);
/* ordinal head `head`'s predicted column (wsa_dbstats_predict_values or _set_values) per file: RG-1's running value at the file's end,
 * sum v sqrt(d) / sum sqrt(d) over the file's rows with a finite v; NaN for a file without one.  Only enqueues. */
wsa_status wsa_dbstats_fold_file_values(wsa_dbstats *db, uint32_t head, void *stream);
/* wsa_dbstats_table, _confusion and _agreement with a file as the row: [n_files] columns, the same kernels */
wsa_status wsa_dbstats_file_table(wsa_dbstats *db, void *stream, wsa_dbstats_cat *cat, wsa_dbstats_class *cls, wsa_dbstats_ord *ord);
wsa_status wsa_dbstats_file_confusion(wsa_dbstats *db, uint32_t head, void *stream, uint64_t *m);
wsa_status wsa_dbstats_file_agreement(wsa_dbstats *db, void *stream, wsa_dbstats_agree *out);
/* for the host to write back: a folded head's meter sums [n_files][n_classes] f64 (n_classes must be the folding model's), the files'
 * predicted classes [n_files] and values [n_files]; each synchronises `stream` */
wsa_status wsa_dbstats_copy_file_sums(wsa_dbstats *db, uint32_t head, void *stream, double *sums, uint32_t n_classes);
wsa_status wsa_dbstats_copy_file_classes(wsa_dbstats *db, uint32_t head, void *stream, int32_t *pred_idx);
wsa_status wsa_dbstats_copy_file_values(wsa_dbstats *db, uint32_t head, void *stream, double *pred_value);

#ifdef __cplusplus
}
#endif
#endif
