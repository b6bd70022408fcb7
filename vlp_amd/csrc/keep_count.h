// Host-only helper of the masked-LM loss launchers (loss.hip): how many samples the drop-worst selection keeps.
#pragma once
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

// The reference computes int(loss.size(0) * (1 - drop_worst_ratio)) with the Python float (a double) the caller typed
// (modeling.py:1083-1093).  The ABI carries the ratio as a float, and widening that float is not the caller's double: 0.2f is
// 0.2 + 3e-9, 1 - 0.2f falls 1.2e-8 short of 0.8 and B = 40 truncates to 31 where Python keeps 32.  No tolerance before the
// truncation repairs that, because Python's own product is not always on the integer (90 * (1 - 0.3) = 62.99999999999999 keeps 62):
// the count is right only if the arithmetic runs on the caller's double itself.  So the double is recovered from the float:
//   1. the double nearest to the float's shortest decimal that rounds back to the same float, when that decimal has at most 6
//      significant digits (0.2f -> "0.2" -> 0.2: every ratio typed with up to 6 digits is recovered exactly; at 7 digits a decimal and a
//      fraction can share a float, 0.6666667f is 2 / 3);
//   2. otherwise the float is not a short decimal, and the simplest fraction p / q inside its rounding interval, divided in double,
//      is taken (0.33333334f -> 1 / 3, as Python evaluates 1 / 3);
// and then the reference's expression is evaluated as Python does: double difference, double product, truncation.
// the fraction p / q with the smallest denominator strictly inside (lo, hi), by continued fractions
static inline void vlp_simplest_fraction(double lo, double hi, int depth, double* p, double* q) {
    const double fl = floor(lo);
    if (fl + 1.0 < hi || depth == 0) { *p = fl + 1.0; *q = 1.0; return; }
    double p1, q1;
    vlp_simplest_fraction(1.0 / (hi - fl), 1.0 / (lo - fl), depth - 1, &p1, &q1);
    *p = fl * p1 + q1;
    *q = p1;
}

static inline double vlp_ratio_as_typed(float f) {
    char buf[64];       // snprintf and strtod follow LC_NUMERIC, but the same one: whatever the decimal point, the text reads back as written
    for (int digits = 1; digits <= 6; ++digits) {
        snprintf(buf, sizeof buf, "%.*e", digits - 1, (double)f);
        const double d = strtod(buf, nullptr);
        if ((float)d == f) return d;
    }
    // (lo, hi): the doubles that round to f
    const double lo = 0.5 * ((double)f + (double)nextafterf(f, -INFINITY)), hi = 0.5 * ((double)f + (double)nextafterf(f, INFINITY));
    double p, q;
    vlp_simplest_fraction(lo, hi, 32, &p, &q);
    const double d = p / q;
    return (float)d == f ? d : (double)f;
}

static inline int vlp_drop_worst_keep_count(int B, float drop_worst_ratio) {
    return (int)((double)B * (1.0 - vlp_ratio_as_typed(drop_worst_ratio)));
}
