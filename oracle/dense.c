/* dense.c — ORACLE (test infrastructure only; never linked into the product).
 * One Dense layer as K6 (csrc/classify.hip classify_tile) computes it, restated literally: mfma_f32_16x16x4f32 is a k-ordered f32 fmaf
 * chain, one rounding per product and no wider accumulator, so
 *     out[r][c] = fl32(fmaf(a[r][kp-1], w[kp-1][c], ... fmaf(a[r][0], w[0][c], +0) ...) + bias[c])
 * over ALL kp padded k (wsa_model_create pads K and N with zeros to multiples of 16: a padded k adds +-0 or, beside a non-finite
 * activation, NaN — as on the device), the bias added with a rounding of its own.  The Makefile's -mfma makes fmaf the hardware's,
 * -ffp-contract=off keeps the bias add apart.  tests/k6_ref.py builds the network around it. */
#include <math.h>
#include <stddef.h>
#include "wsa_oracle.h"

/* the wrong orders tests/test_k6_reference.py must be able to tell from the right one */
enum { DENSE_RIGHT = 0, DENSE_K_DESCENDING = 1, DENSE_PAIRS = 2, DENSE_BIAS_FIRST = 3 };

static float dense_unit(const float *a, const float *w, uint32_t kp, uint32_t np, float bias, int32_t order) {
    float acc = order == DENSE_BIAS_FIRST ? bias : 0.f;
    if (order == DENSE_K_DESCENDING) {
        for (uint32_t k = kp; k-- > 0;) acc = fmaf(a[k], w[(size_t)k * np], acc);
    } else if (order == DENSE_PAIRS) {                     /* (a0 b0 + a1 b1) + acc: a two-term dot product rounded once, then added */
        for (uint32_t k = 0; k + 1 < kp; k += 2) {
            const float pair = fmaf(a[k + 1], w[(size_t)(k + 1) * np], a[k] * w[(size_t)k * np]);
            acc = pair + acc;
        }
    } else {
        for (uint32_t k = 0; k < kp; k++) acc = fmaf(a[k], w[(size_t)k * np], acc);
    }
    return order == DENSE_BIAS_FIRST ? acc : acc + bias;
}

void wsa_or_dense_f32_order(const float *a, const float *w, const float *bias, uint32_t rows, uint32_t kp, uint32_t np, int32_t order, float *out) {
    for (uint32_t r = 0; r < rows; r++)
        for (uint32_t c = 0; c < np; c++) out[(size_t)r * np + c] = dense_unit(a + (size_t)r * kp, w + c, kp, np, bias[c], order);
}

void wsa_or_dense_f32(const float *a, const float *w, const float *bias, uint32_t rows, uint32_t kp, uint32_t np, float *out) {
    wsa_or_dense_f32_order(a, w, bias, rows, kp, np, DENSE_RIGHT, out);
}

/* ml5 unnormalizeValue on K6's regression output: p * span + min in doubles, two roundings; fused != 0: the contracted form (one rounding) */
double wsa_or_unnormalise(float p, double out_min, double out_span, int32_t fused) {
    if (fused) return fma((double)p, out_span, out_min);
    const double scaled = (double)p * out_span;
    return scaled + out_min;
}
