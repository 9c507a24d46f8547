// Host-only check of sc_mixture_fit / sc_mixture_predict (csrc/sc_mixture.hip), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_mixture` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the argument checks and the walk over the
// caller's arrays -- sized exactly, so a read past an end is caught.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "sc_permgen.h"   // completes sc_ctx (its pipeline member) for a host-side instance

static int failures = 0;

static void expect(const char *what, int rc, int want, const char *fragment)
{
    const char *msg = sc_last_error();
    const bool ok = rc == want && (!fragment || strstr(msg, fragment));
    if (!ok) {
        ++failures;
        printf("FAIL %s: rc=%d (want %d), message \"%s\" (want \"%s\")\n", what, rc, want, msg, fragment ? fragment : "");
    }
}

int main()
{
    sc_ctx ctx;
    sc_ctx *c = &ctx;
    // six cells, two columns, two components, one run: L = 2 + int(log 2) = 2, so 1 + (K - 1) L = 3 draws
    double X[12] = {0, 0, 1, 0, 0, 1, 9, 9, 8, 9, 9, 8};
    float Xf[12] = {0, 0, 1, 0, 0, 1, 9, 9, 8, 9, 9, 8};
    const double xm[2] = {4.5, 4.5}, u[3] = {0.1, 0.5, 0.9};
    double w[2], mu[4], cov[8], lb[1], ll;
    int32_t it[1], cv[1], best, lab[6];
    const int F = SC_MIX_FULL, Dg = SC_MIX_DIAG;

#define FIT(X_, dt, n, D, K, ct, R, kmi, kmt, xm_, u_, mi, tol, reg, w_, lab_, ll_) \
    sc_mixture_fit(c, X_, dt, n, D, K, ct, R, kmi, kmt, xm_, u_, mi, tol, reg, w_, mu, cov, lb, it, cv, &best, lab_, nullptr, ll_)

    // ---- sc_mixture_fit ----
    expect("fit null ctx", sc_mixture_fit(nullptr, X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, mu, cov, lb, it, cv, &best, lab, nullptr, &ll),
           SC_ERR_INVALID, "sc_mixture_fit: null pointer");
    expect("fit null X", FIT(nullptr, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "sc_mixture_fit: null pointer");
    expect("fit null weights", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, nullptr, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("fit null labels", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, nullptr, &ll), SC_ERR_INVALID, "null pointer");
    expect("fit null loglik", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, nullptr), SC_ERR_INVALID, "null pointer");
    expect("fit dtype", FIT(X, 7, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "dtype must be SC_F32 or SC_F64");
    expect("fit n = 0", FIT(X, SC_F64, 0, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got 0");
    expect("fit n = 2^31", FIT(X, SC_F64, (int64_t)1 << 31, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID,
           "need 1 <= n <= 2^31 - 1, got 2147483648");   // refused on n: nothing is read
    expect("fit D = 0", FIT(X, SC_F64, 6, 0, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= D <= 256, got 0");
    expect("fit D = 257", FIT(X, SC_F64, 6, 257, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= D <= 256, got 257");
    expect("fit K = 0", FIT(X, SC_F64, 6, 2, 0, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= K <= min(64, n)");
    expect("fit K = 65", FIT(X, SC_F64, 100, 2, 65, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= K <= min(64, n)");
    expect("fit K > n", FIT(X, SC_F64, 6, 2, 7, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "(K = 7, n = 6)");
    expect("fit cov_type", FIT(X, SC_F64, 6, 2, 2, 2, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID,
           "cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got 2");
    expect("fit null x_mean", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, nullptr, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("fit null uniforms", FIT(X, SC_F64, 6, 2, 2, Dg, 1, 300, 1e-4, xm, nullptr, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("fit n_init = 0", FIT(X, SC_F64, 6, 2, 2, F, 0, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= n_init <= 10, got 0");
    expect("fit n_init = 11", FIT(X, SC_F64, 6, 2, 2, F, 11, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "need 1 <= n_init <= 10, got 11");
    expect("fit km_max_iter", FIT(X, SC_F64, 6, 2, 2, F, 1, 0, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "km_max_iter and max_iter must be >= 1");
    expect("fit max_iter", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 0, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "km_max_iter and max_iter must be >= 1");
    expect("fit km_tol", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, -1.0, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "must be finite and >= 0");
    expect("fit tol", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, NAN, 1e-6, w, lab, &ll), SC_ERR_INVALID, "must be finite and >= 0");
    expect("fit reg_covar", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, -1e-6, w, lab, &ll), SC_ERR_INVALID, "must be finite and >= 0");
    expect("fit reg_covar inf", FIT(X, SC_F64, 6, 2, 2, Dg, 1, 300, 1e-4, xm, u, 100, 1e-3, INFINITY, w, lab, &ll), SC_ERR_INVALID, "must be finite and >= 0");
    X[11] = NAN;   // the very last value
    expect("fit nan", FIT(X, SC_F64, 6, 2, 2, F, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "value 11 is not finite");
    X[11] = 8;
    Xf[11] = INFINITY;
    expect("fit inf float32", FIT(Xf, SC_F32, 6, 2, 2, Dg, 1, 300, 1e-4, xm, u, 100, 1e-3, 1e-6, w, lab, &ll), SC_ERR_INVALID, "value 11 is not finite");
    Xf[11] = 8;

    // ---- sc_mixture_predict ----
    const double pw[2] = {0.5, 0.5}, pm[4] = {0.3, 0.3, 8.7, 8.7};
    double pc[8] = {1, 0, 0, 1, 1, 0, 0, 1}, pd[4] = {1, 1, 1, 1};
#define PRED(X_, dt, n, D, K, ct, w_, m_, c_, lab_, ll_) sc_mixture_predict(c, X_, dt, n, D, K, ct, w_, m_, c_, lab_, nullptr, ll_)
    expect("predict null ctx", sc_mixture_predict(nullptr, X, SC_F64, 6, 2, 2, F, pw, pm, pc, lab, nullptr, &ll), SC_ERR_INVALID,
           "sc_mixture_predict: null pointer");
    expect("predict null X", PRED(nullptr, SC_F64, 6, 2, 2, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "sc_mixture_predict: null pointer");
    expect("predict null weights", PRED(X, SC_F64, 6, 2, 2, F, nullptr, pm, pc, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("predict null means", PRED(X, SC_F64, 6, 2, 2, F, pw, nullptr, pc, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("predict null covariances", PRED(X, SC_F64, 6, 2, 2, F, pw, pm, nullptr, lab, &ll), SC_ERR_INVALID, "null pointer");
    expect("predict null labels", PRED(X, SC_F64, 6, 2, 2, F, pw, pm, pc, nullptr, &ll), SC_ERR_INVALID, "null pointer");
    expect("predict null loglik", PRED(X, SC_F64, 6, 2, 2, F, pw, pm, pc, lab, nullptr), SC_ERR_INVALID, "null pointer");
    expect("predict dtype", PRED(X, -1, 6, 2, 2, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "dtype must be SC_F32 or SC_F64");
    expect("predict n = 0", PRED(X, SC_F64, 0, 2, 2, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got 0");
    expect("predict D = 257", PRED(X, SC_F64, 6, 257, 2, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "need 1 <= D <= 256, got 257");
    expect("predict K = 0", PRED(X, SC_F64, 6, 2, 0, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "need 1 <= K <= 64, got 0");
    expect("predict K = 65", PRED(X, SC_F64, 6, 2, 65, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "need 1 <= K <= 64, got 65");
    expect("predict cov_type", PRED(X, SC_F64, 6, 2, 2, -1, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got -1");
    {
        const double bad[2] = {1.0, 0.0};
        expect("predict weight 0", PRED(X, SC_F64, 6, 2, 2, F, bad, pm, pc, lab, &ll), SC_ERR_INVALID, "weight 1 must be finite and > 0");
    }
    {
        const double bad[4] = {0.3, 0.3, 8.7, NAN};
        expect("predict mean nan", PRED(X, SC_F64, 6, 2, 2, Dg, pw, bad, pd, lab, &ll), SC_ERR_INVALID, "mean 3 is not finite");
    }
    pc[7] = INFINITY;   // the very last entry of the full covariances
    expect("predict covariance inf", PRED(X, SC_F64, 6, 2, 2, F, pw, pm, pc, lab, &ll), SC_ERR_INVALID, "covariance 7 is not finite");
    pc[7] = 1;
    pd[3] = NAN;        // the very last entry of the diagonal ones: only four are read
    expect("predict variance nan", PRED(X, SC_F64, 6, 2, 2, Dg, pw, pm, pd, lab, &ll), SC_ERR_INVALID, "covariance 3 is not finite");
    pd[3] = 1;
    X[11] = INFINITY;
    expect("predict inf", PRED(X, SC_F64, 6, 2, 2, Dg, pw, pm, pd, lab, &ll), SC_ERR_INVALID, "value 11 is not finite");

    // ---- sc_mixture_slice_rows: host only ----
    int64_t rows = -1;
    expect("slice null", sc_mixture_slice_rows(6, 2, 2, F, nullptr), SC_ERR_INVALID, "sc_mixture_slice_rows: null pointer");
    expect("slice n = 0", sc_mixture_slice_rows(0, 2, 2, F, &rows), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got 0");
    expect("slice D = 257", sc_mixture_slice_rows(6, 257, 2, F, &rows), SC_ERR_INVALID, "need 1 <= D <= 256, got 257");
    expect("slice K = 65", sc_mixture_slice_rows(6, 2, 65, F, &rows), SC_ERR_INVALID, "need 1 <= K <= 64, got 65");
    expect("slice cov_type", sc_mixture_slice_rows(6, 2, 2, 5, &rows), SC_ERR_INVALID, "cov_type must be SC_MIX_FULL or SC_MIX_DIAG, got 5");
    if (rows != -1) {
        ++failures;
        printf("FAIL a refused sc_mixture_slice_rows wrote its output\n");
    }
    expect("slice small", sc_mixture_slice_rows(6, 2, 2, F, &rows), SC_OK, nullptr);
    if (rows != 1024) {
        ++failures;
        printf("FAIL slice rows of a small shape: %lld\n", (long long)rows);
    }
    expect("slice 1e6 x 200", sc_mixture_slice_rows(1000000, 200, 20, F, &rows), SC_OK, nullptr);
    if (rows != 25024) {
        ++failures;
        printf("FAIL slice rows at 10^6 x 200, K = 20: %lld\n", (long long)rows);
    }

    printf(failures ? "%d checks FAILED\n" : "mixture host checks ok\n", failures);
    return failures ? 1 : 0;
}
