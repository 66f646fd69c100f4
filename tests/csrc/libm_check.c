/* Test helper (CPU): holds slidingwindowdecoder_amd/csrc/swd_libm.h to the host C library, bit for bit.
 * Built by tests/test_libm_restatement.py with gcc; returns the number of arguments where the results differ.
 * swd_eval_header / swd_eval_libm (below) evaluate the ops of swd_diag_libm (include/swd.h) on arrays: the host build of the header
 * that tests/test_gpu_libm.py holds the device build to, and the C library's own exp / log1p under the same composites. */
#include <float.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "swd_libm.h"

static uint64_t rng_state;
static double urand(void) { /* splitmix64 -> [0, 1) */
    uint64_t z = (rng_state += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1p-53;
}
static int same(double a, double b) {
    uint64_t x, y;
    memcpy(&x, &a, 8); memcpy(&y, &b, 8);
    return x == y || (a != a && b != b);
}

long swd_check_exp(long n, uint64_t seed, double *first_bad) {
    long bad = 0;
    rng_state = seed;
    for (long i = 0; i < n; ++i) {
        double x;
        switch (i % 6) {
        case 0: x = (urand() - 0.5) * 100.0; break;
        case 1: x = (urand() - 0.5) * 2.0; break;
        case 2: x = -urand() * 760.0; break;          /* down to the subnormal results and underflow */
        case 3: x = urand() * 712.0; break;           /* up to overflow */
        case 4: x = (urand() - 0.5) * 1e-3; break;
        default: x = (urand() - 0.5) * exp((urand() - 0.5) * 100.0); break;
        }
        if (!same(exp(x), swd_exp(x))) { if (!bad && first_bad) *first_bad = x; ++bad; }
    }
    const double special[] = {0.0, -0.0, 1.0, -1.0, INFINITY, -INFINITY, NAN, 1e308, -1e308, 709.782712893384, -745.2, 0x1p-60, 512.0, -512.0, 1023.9, -1023.9};
    for (unsigned i = 0; i < sizeof special / sizeof special[0]; ++i)
        if (!same(exp(special[i]), swd_exp(special[i]))) { if (!bad && first_bad) *first_bad = special[i]; ++bad; }
    return bad;
}

long swd_check_log1p(long n, uint64_t seed, double *first_bad) {
    long bad = 0;
    rng_state = seed;
    for (long i = 0; i < n; ++i) {
        double x;
        switch (i % 6) {
        case 0: x = urand() * 2.0 - 0.999; break;
        case 1: x = exp((urand() - 0.5) * 1400.0); break;
        case 2: x = -exp(-urand() * 700.0); break;
        case 3: x = (urand() - 0.5) * 1e-6; break;
        case 4: x = exp((urand() - 0.5) * 80.0); break;
        default: x = urand() * 100.0; break;
        }
        if (!same(log1p(x), swd_log1p(x))) { if (!bad && first_bad) *first_bad = x; ++bad; }
    }
    const double special[] = {0.0, -0.0, -1.0, -2.0, INFINITY, NAN, 1e308, 0x1p-60, 0x1p-30, 0x1p53, 0x1p52, -0.2929, 0.41422, 1.0};
    for (unsigned i = 0; i < sizeof special / sizeof special[0]; ++i)
        if (!same(log1p(special[i]), swd_log1p(special[i]))) { if (!bad && first_bad) *first_bad = special[i]; ++bad; }
    return bad;
}

/* log1pexp / logaddexp in the BRANCHING form of the reference (src/include/bpgd.cpp:399-416, oracle/swd_oracle.c log1pexp_ /
 * logaddexp_), over the header's exp / log1p: what the device's branch-free bp4_log1pexp / bp4_logaddexp must equal */
static double hdr_log1pexp(double x) {
    if (x > 36.04365338911715) return x + swd_log1p(swd_exp(-x));
    return swd_log1p(swd_exp(x));
}
static double hdr_logaddexp(double x, double y) {
    double const tmp = x - y;
    if (x == y) return x + M_LN2;
    if (tmp > 0) return x + hdr_log1pexp(-tmp);
    else if (tmp <= 0) return y + hdr_log1pexp(tmp);
    return tmp;
}
/* the same two over the C library, the threshold spelled as the reference spells it */
static double libm_log1pexp(double x) {
    if (x > -log(DBL_EPSILON)) return x + log1p(exp(-x));
    return log1p(exp(x));
}
static double libm_logaddexp(double x, double y) {
    double const tmp = x - y;
    if (x == y) return x + M_LN2;
    if (tmp > 0) return x + libm_log1pexp(-tmp);
    else if (tmp <= 0) return y + libm_log1pexp(tmp);
    return tmp;
}

/* ops of swd_diag_libm: 0 / 1 exp, 2 log1p, 3 / 5 log1pexp, 4 / 6 logaddexp(x, y) (the device's ops 1, 5, 6 are other COPIES of
 * the same functions); y is read by ops 4 and 6 only.  Returns -1 for an unknown op. */
int swd_eval_header(int op, long n, const double *x, const double *y, double *out) {
    if (op < 0 || op > 6) return -1;
    for (long i = 0; i < n; ++i)
        out[i] = op <= 1 ? swd_exp(x[i]) : op == 2 ? swd_log1p(x[i]) : (op == 3 || op == 5) ? hdr_log1pexp(x[i]) : hdr_logaddexp(x[i], y[i]);
    return 0;
}
int swd_eval_libm(int op, long n, const double *x, const double *y, double *out) {
    if (op < 0 || op > 6) return -1;
    for (long i = 0; i < n; ++i)
        out[i] = op <= 1 ? exp(x[i]) : op == 2 ? log1p(x[i]) : (op == 3 || op == 5) ? libm_log1pexp(x[i]) : libm_logaddexp(x[i], y[i]);
    return 0;
}
