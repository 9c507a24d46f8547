// Host-only check of sc_nmf_fit_graph's argument validation (csrc/sc_nmf.hip), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_nmf` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's
// arrays -- the CSR walks of the matrix and of the graph, the mirror search -- on inputs sized exactly, so a read past
// an end is caught.
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
    // three cells over four genes, K = 2; the graph 0 -- 1 (weight 0.5), 1 -- 2 (weight 2); then one defect at a time
    const int64_t xp[4] = {0, 2, 2, 5};
    const int32_t xi[5] = {0, 3, 1, 2, 3};
    const double xv[5] = {1.0, 2.0, 0.5, 3.0, 4.0};
    const int64_t gp[4] = {0, 1, 3, 4};
    const int32_t gi[4] = {1, 0, 2, 1};
    const double gv[4] = {0.5, 0.5, 2.0, 2.0};
    double W[6] = {1, 1, 1, 1, 1, 1}, H[8] = {1, 1, 1, 1, 1, 1, 1, 1};
    double obj[2], err[2], recon, pen;   // 1 + max_iter / 10 slots with max_iter = 10
    int32_t checks, iters;
    auto graph = [&](const int64_t *p, const int32_t *i, const double *v, double lambda) {
        return sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, p, i, v, lambda, 10, 1e-4, W, H, obj, err, &checks, &iters, &recon, &pen);
    };
    auto matrix = [&](const int64_t *p, const int32_t *i, const void *v, int dtype, int64_t n, int32_t G, int32_t K, int32_t max_iter,
                      double tol) {
        return sc_nmf_fit_graph(c, p, i, v, dtype, n, G, K, gp, gi, gv, 1.0, max_iter, tol, W, H, obj, err, &checks, &iters, &recon, &pen);
    };

    // ---- null pointers ----
    expect("null ctx", sc_nmf_fit_graph(nullptr, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, err, &checks, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null indptr", matrix(nullptr, xi, xv, SC_F64, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "null pointer");
    expect("null indices", matrix(xp, nullptr, xv, SC_F64, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "null pointer");
    expect("null data", matrix(xp, xi, nullptr, SC_F64, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "null pointer");
    expect("null gptr", graph(nullptr, gi, gv, 1.0), SC_ERR_INVALID, "null pointer");
    expect("null gidx", graph(gp, nullptr, gv, 1.0), SC_ERR_INVALID, "null pointer");
    expect("null gval", graph(gp, gi, nullptr, 1.0), SC_ERR_INVALID, "null pointer");
    expect("null W", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, nullptr, H, obj, err, &checks, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null H", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, nullptr, obj, err, &checks, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null obj trace", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, nullptr, err, &checks, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null err trace", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, nullptr, &checks, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null checks", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, err, nullptr, &iters, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null iters", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, err, &checks, nullptr, &recon, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null recon", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, err, &checks, &iters, nullptr, &pen),
           SC_ERR_INVALID, "null pointer");
    expect("null penalty", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, W, H, obj, err, &checks, &iters, &recon, nullptr),
           SC_ERR_INVALID, "null pointer");

    // ---- scalars and the matrix (sc_nmf_fit's gates under this entry's name) ----
    expect("dtype", matrix(xp, xi, xv, 7, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "dtype");
    expect("n = 0", matrix(xp, xi, xv, SC_F64, 0, 4, 2, 10, 1e-4), SC_ERR_INVALID, "1 <= n <= 2^31 - 1");
    expect("G = 0", matrix(xp, xi, xv, SC_F64, 3, 0, 2, 10, 1e-4), SC_ERR_INVALID, "1 <= n_genes <= 32768");
    expect("K = 0", matrix(xp, xi, xv, SC_F64, 3, 4, 0, 10, 1e-4), SC_ERR_INVALID, "1 <= K <= 64");
    expect("K = 65", matrix(xp, xi, xv, SC_F64, 3, 4, 65, 10, 1e-4), SC_ERR_INVALID, "1 <= K <= 64");
    expect("max_iter = 0", matrix(xp, xi, xv, SC_F64, 3, 4, 2, 0, 1e-4), SC_ERR_INVALID, "max_iter must be >= 1");
    expect("tol < 0", matrix(xp, xi, xv, SC_F64, 3, 4, 2, 10, -1.0), SC_ERR_INVALID, "tol must be finite and >= 0");
    expect("tol nan", matrix(xp, xi, xv, SC_F64, 3, 4, 2, 10, NAN), SC_ERR_INVALID, "tol must be finite and >= 0");
    expect("lambda < 0", graph(gp, gi, gv, -1.0), SC_ERR_INVALID, "lambda must be finite and >= 0");
    expect("lambda nan", graph(gp, gi, gv, NAN), SC_ERR_INVALID, "lambda must be finite and >= 0");
    expect("lambda inf", graph(gp, gi, gv, INFINITY), SC_ERR_INVALID, "lambda must be finite and >= 0");
    {
        const int32_t i[5] = {0, 4, 1, 2, 3};
        expect("matrix column = G", matrix(xp, i, xv, SC_F64, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "sc_nmf_fit_graph: row 0 is not canonical");
    }
    {
        const double v[5] = {1.0, 2.0, 0.5, 3.0, -4.0};
        expect("matrix negative", matrix(xp, xi, v, SC_F64, 3, 4, 2, 10, 1e-4), SC_ERR_INVALID, "stored value 4 is negative");
    }
    {
        double Wbad[6] = {1, 1, 1, 1, 1, -1};
        expect("W0 negative", sc_nmf_fit_graph(c, xp, xi, xv, SC_F64, 3, 4, 2, gp, gi, gv, 1.0, 10, 1e-4, Wbad, H, obj, err, &checks, &iters, &recon, &pen),
               SC_ERR_INVALID, "W0 must be finite and >= 0");
    }

    // ---- the graph, one defect at a time ----
    {
        const int64_t p[4] = {1, 1, 3, 4};
        expect("gptr[0]", graph(p, gi, gv, 1.0), SC_ERR_INVALID, "indptr[0]");
    }
    {
        const int64_t p[4] = {0, 3, 1, 4};
        expect("gptr decreases", graph(p, gi, gv, 1.0), SC_ERR_INVALID, "indptr decreases at row 1");
    }
    {
        const int64_t p[4] = {0, 1, 3, ((int64_t)1 << 32)};   // refused on the count: no entry is read
        expect("too many graph entries", graph(p, gi, gv, 1.0), SC_ERR_INVALID, "stored graph entries <= 2^32 - 1");
    }
    {
        const int64_t p[4] = {0, 1, 2, 3};
        const int32_t i[3] = {1, 0, 1};                       // 2 -> 1 has no mirror: the very last entry
        const double v[3] = {0.5, 0.5, 2.0};
        expect("asymmetric structure", graph(p, i, v, 1.0), SC_ERR_INVALID, "graph entry 2 (row 2, column 1) has no mirror entry");
    }
    {
        const int64_t p[4] = {0, 1, 1, 1};
        const int32_t i[1] = {2};                             // the mirror row is empty
        const double v[1] = {1.0};
        expect("mirror row empty", graph(p, i, v, 1.0), SC_ERR_INVALID, "graph entry 0 (row 0, column 2) has no mirror entry");
    }
    {
        const double v[4] = {0.5, 0.5, 2.0, 2.5};
        expect("asymmetric value", graph(gp, gi, v, 1.0), SC_ERR_INVALID, "graph entry 2 (row 1, column 2) and its mirror differ in weight");
    }
    {
        const int64_t p[4] = {0, 1, 4, 5};
        const int32_t i[5] = {1, 0, 1, 2, 1};
        const double v[5] = {0.5, 0.5, 1.0, 2.0, 2.0};
        expect("diagonal", graph(p, i, v, 1.0), SC_ERR_INVALID, "graph entry 2 is on the diagonal (row 1)");
    }
    {
        const int32_t i[4] = {1, 2, 0, 1};
        expect("non-ascending column", graph(gp, i, gv, 1.0), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const int32_t i[4] = {1, 0, 0, 1};
        expect("repeated column", graph(gp, i, gv, 1.0), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const int32_t i[4] = {1, 0, 2, 3};                    // column = n, the very last entry
        expect("column out of range", graph(gp, i, gv, 1.0), SC_ERR_INVALID, "row 2 is not canonical");
    }
    {
        const int32_t i[4] = {-1, 0, 2, 1};
        expect("negative column", graph(gp, i, gv, 1.0), SC_ERR_INVALID, "row 0 is not canonical");
    }
    {
        const double v[4] = {0.5, 0.5, 2.0, 0.0};
        expect("zero weight", graph(gp, gi, v, 1.0), SC_ERR_INVALID, "graph weight 3 (row 2, column 1) must be finite and > 0");
    }
    {
        const double v[4] = {-0.5, -0.5, 2.0, 2.0};
        expect("negative weight", graph(gp, gi, v, 1.0), SC_ERR_INVALID, "graph weight 0 (row 0, column 1) must be finite and > 0");
    }
    {
        const double v[4] = {0.5, 0.5, 2.0, NAN};
        expect("nan weight", graph(gp, gi, v, 1.0), SC_ERR_INVALID, "graph weight 3 (row 2, column 1) must be finite and > 0");
    }
    {
        const double v[4] = {0.5, 0.5, INFINITY, INFINITY};
        expect("inf weight", graph(gp, gi, v, 1.0), SC_ERR_INVALID, "graph weight 2 (row 1, column 2) must be finite and > 0");
    }

    printf(failures ? "%d checks FAILED\n" : "nmf graph host checks ok\n", failures);
    return failures ? 1 : 0;
}
