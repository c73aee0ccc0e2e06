/*
 * wsa_crossval.h — C ABI of libwsa, cross-validating the app's models on a labelled feature DB (additions within version 5 of wsa.h:
 * probe for wsa_dbstats_set_folds).  Specification CV-1 and kernel K6f of DESIGN.md (csrc/crossval.hip, csrc/classify.hip).
 *
 * wsa_dbstats_predict_classes / _values (wsa.h, DS-1) run ONE model over every row of a wsa_dbstats object, the rows it was trained on
 * included.  These entries run K models in one launch, each over the rows of the fold it did not see: every row of the DB is given a
 * fold (the host's rule: webspeechanalyzer_amd.crossval, a file's rows stay together), model k is the one trained without fold k, and
 * row i of fold k gets model k's output, in the bits wsa_classify_rows / wsa_regress_rows give for that model on that row.  What they
 * leave is what wsa_dbstats_predict_classes / _values leave, so the decision, wsa_dbstats_table, the entries of wsa_eval.h (confusion,
 * agreement, the per-file fold and its tables) and the copies work on it unchanged.  Pass the SAME stream as to every other call on the
 * object.
 * These declarations live beside wsa.h, not in it, for the reason wsa_eval.h gives; this header is held to capi.CROSSVAL_TABLE
 * (tests/test_crossval_host.py).
 */
#ifndef WSA_CROSSVAL_H
#define WSA_CROSSVAL_H
#include "wsa.h"

#ifdef __cplusplus
extern "C" {
#endif

/* folds of one cross-validation, 2 .. WSA_CROSSVAL_MAX_FOLDS: one model per fold, and the K models of a head train as one group */
#define WSA_CROSSVAL_MAX_FOLDS 32
#if WSA_CROSSVAL_MAX_FOLDS != WSA_TRAIN_GROUP_MAX
#error "a cross-validation's models train as one training group"
#endif

/* host [n_rows]: the fold of every row, -1 (the row is never held out and never predicted) or 0 .. n_folds - 1.  Builds the rows of
 * every fold, ascending, on the device, and K6f's table.  Synchronous; set once.
 * WSA_ERR_INVALID with a message, the object left as it was: n_folds outside 2 .. 32 (naming it), a fold outside -1 .. n_folds - 1
 * (naming the first offending row), a second call, a DB created without feature rows. */
wsa_status wsa_dbstats_set_folds(wsa_dbstats *db, const int32_t *fold_of_row, uint32_t n_folds);
/* wsa_dbstats_predict_classes with models[k] over the rows of fold k: the probability table is zeroed, K6f writes every row that has a
 * fold, DS-1's decision runs over all rows (a row without a fold has no probability above 0 and stays blank).  All members share one
 * legend: the same class count and the same key ranks (Object.keys order), which legend_to_vocab [C] maps into the head's vocabulary.
 * Leaves the kept probabilities, their head, map and key ranks as wsa_dbstats_predict_classes does.  Only enqueues (it waits for the
 * previous call's launch to have read the table); the first call allocates the probability table, later ones nothing.
 * WSA_ERR_INVALID: no folds set, n_models != n_folds, a NULL member, a member of another context, a regression model, a member whose
 * input count is not the DB's width, a member whose class count or key ranks differ from member 0's (each naming the member), a bad
 * legend_to_vocab. */
wsa_status wsa_dbstats_predict_classes_folds(wsa_dbstats *db, uint32_t head, const wsa_model *const *models, uint32_t n_models,
                                             const int32_t *legend_to_vocab, void *stream);
/* wsa_dbstats_predict_values with models[k] and its own range out_min[k] .. out_max[k] over the rows of fold k: ordinal head `head`'s
 * predicted column is filled with NaN, K6f writes every row that has a fold.  Only enqueues; allocates nothing.
 * WSA_ERR_INVALID: as above, and per member (naming it) what wsa_regress_rows refuses: a classifier, a non-finite or empty range. */
wsa_status wsa_dbstats_predict_values_folds(wsa_dbstats *db, uint32_t head, const wsa_model *const *models, uint32_t n_models,
                                            const double *out_min, const double *out_max, void *stream);
/* pure, needs no device: the (member, tile) pairs of one K6f launch over lists of rows_per_fold[k] rows whose members have the row-block
 * factor rb[k] (1, 2 or 4: a tile is 16 rb rows; a model's own factor follows from its widest layer) — the sum of
 * ceil(rows_per_fold[k] / (16 rb[k])).  0: nothing is launched.  WSA_ERR_INVALID: a null argument, n outside 1 .. 32, an rb that is
 * not 1, 2 or 4. */
wsa_status wsa_crossval_tiles(const uint32_t *rows_per_fold, const int32_t *rb, uint32_t n, uint64_t *tiles);

#ifdef __cplusplus
}
#endif
#endif
