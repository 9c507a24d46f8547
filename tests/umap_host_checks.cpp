// Host-only check of sc_umap_layout's and sc_fuzzy_graph's argument validation (csrc/sc_umap.hip) and of the layout's firing
// schedule (csrc/sc_umap.h), meant for the sanitizer build: `make -C spatialcore_amd/csrc asan_umap` links this program (its
// own main, nothing preloaded) against the AddressSanitizer + UBSan objects and runs it.  The context is constructed on the
// host and every call below is refused before its first HIP call, so no device is needed or touched: what runs is the host
// code that reads the caller's arrays -- the CSR and position checks -- on inputs sized exactly, so a read past an end is caught.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "sc_permgen.h"   // completes sc_ctx (its pipeline member) for a host-side instance
#include "sc_umap.h"

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
    // a path on four vertices: 0 - 1 - 2 - 3
    std::vector<int64_t> indptr = {0, 1, 3, 5, 6};
    std::vector<int32_t> indices = {1, 0, 2, 1, 3, 2};
    std::vector<double> w = {1.0, 1.0, 0.5, 0.5, 0.25, 0.25};
    std::vector<double> Y = {0.0, 0.0, 1.0, 0.5, 2.0, -0.5, 3.0, 0.25};
    const std::vector<double> Y0 = Y;
    auto lay = [&](sc_ctx *cc, const int64_t *ip, const int32_t *ix, const double *ww, int64_t n, double *y, int32_t C, double a, double b,
                   double gamma, double alpha0, int32_t neg, int32_t n_epochs, int32_t e0, int32_t e1) {
        return sc_umap_layout(cc, ip, ix, ww, n, y, C, a, b, gamma, alpha0, neg, n_epochs, 7u, e0, e1);
    };
    const int64_t *ip = indptr.data();
    const int32_t *ix = indices.data();
    const double *ww = w.data();
    double *y = Y.data();

    expect("null ctx", lay(nullptr, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "null pointer");
    expect("null Y", lay(c, ip, ix, ww, 4, nullptr, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "null pointer");
    expect("half a graph", lay(c, ip, nullptr, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "all be given or all be NULL");
    expect("n = 0", lay(c, ip, ix, ww, 0, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "1 <= n <= 2^31 - 1");
    expect("n = 2^31", lay(c, ip, ix, ww, (int64_t)1 << 31, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "1 <= n <= 2^31 - 1");
    expect("C = 1", lay(c, ip, ix, ww, 4, y, 1, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "2 or 3 components");
    expect("C = 4", lay(c, ip, ix, ww, 4, y, 4, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "2 or 3 components");
    expect("a = 0", lay(c, ip, ix, ww, 4, y, 2, 0, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "a and b");
    expect("b = nan", lay(c, ip, ix, ww, 4, y, 2, 1, NAN, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "a and b");
    expect("gamma < 0", lay(c, ip, ix, ww, 4, y, 2, 1, 1, -1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "gamma");
    expect("alpha0 = inf", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, INFINITY, 5, 10, 0, 10), SC_ERR_INVALID, "alpha0");
    expect("neg = -1", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, -1, 10, 0, 10), SC_ERR_INVALID, "0 <= neg <= 16");
    expect("neg = 17", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 17, 10, 0, 10), SC_ERR_INVALID, "0 <= neg <= 16");
    expect("n_epochs = 0", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 0, 0, 0), SC_ERR_INVALID, "n_epochs >= 1");
    expect("e0 < 0", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, -1, 10), SC_ERR_INVALID, "epoch range");
    expect("e0 > e1", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 6, 5), SC_ERR_INVALID, "epoch range");
    expect("e1 > n_epochs", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 11), SC_ERR_INVALID, "epoch range");
    Y[7] = NAN;            // the very last value: the check reads all n * C of them and no more
    expect("nan position", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "position value 7");
    Y[7] = 0.25;
    indptr[0] = 1;
    expect("indptr[0]", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "indptr[0] must be 0");
    indptr[0] = 0;
    indptr[2] = 0;
    expect("descending indptr", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "indptr descends at row 1");
    indptr[2] = 3;
    indices[5] = 4;        // the very last index
    expect("column = n", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "row 3 is not canonical");
    indices[5] = -1;
    expect("column < 0", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "row 3 is not canonical");
    indices[5] = 2;
    indices[2] = 2;
    indices[1] = 2;
    expect("unsorted row", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "row 1 is not canonical");
    indices[1] = 0;
    w[5] = 0.0;            // the very last value
    expect("w = 0", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "stored value 5");
    w[5] = INFINITY;
    expect("w = inf", lay(c, ip, ix, ww, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_INVALID, "stored value 5");
    w[5] = 0.25;
    expect("no resident graph", lay(c, nullptr, nullptr, nullptr, 4, y, 2, 1, 1, 1, 1, 5, 10, 0, 10), SC_ERR_STATE, "no graph is resident");
    if (Y != Y0) {
        ++failures;
        printf("FAIL a refused call wrote to the positions\n");
    }

    int64_t ne = -1, nc = -1;
    expect("fuzzy: null ctx", sc_fuzzy_graph(nullptr, nullptr, nullptr, &ne, &nc), SC_ERR_INVALID, "null pointer");
    expect("fuzzy: null counts", sc_fuzzy_graph(c, nullptr, nullptr, nullptr, &nc), SC_ERR_INVALID, "null pointer");
    expect("fuzzy: no lists", sc_fuzzy_graph(c, nullptr, nullptr, &ne, &nc), SC_ERR_STATE, "no neighbour lists are resident");
    if (ne != -1 || nc != -1 || ctx.lg.valid) {
        ++failures;
        printf("FAIL a refused sc_fuzzy_graph wrote its counts or claimed a resident graph\n");
    }

    // the schedule: over n_epochs epochs an entry fires floor(n_epochs * r) times, evenly spread; r = 1 fires always
    const int n_epochs = 200;
    for (int step = 0; step <= 1000; ++step) {
        const double wt = step / 1000.0 * 3.0, w_max = 3.0, r = wt / w_max;
        int fired = 0, longest_gap = 0, gap = 0;
        for (int e = 0; e < n_epochs; ++e) {
            if (um_fires(wt, w_max, (uint32_t)e)) {
                ++fired;
                gap = 0;
            } else if (++gap > longest_gap) {
                longest_gap = gap;
            }
        }
        const int want = (int)floor((double)n_epochs * r);
        if (fired != want || (step == 1000 && fired != n_epochs) || (r > 0.0 && want > 0 && longest_gap > (int)ceil(1.0 / r))) {
            ++failures;
            printf("FAIL schedule: r=%g fired %d times (want %d), longest gap %d\n", r, fired, want, longest_gap);
        }
    }
    if (um_fires(0.0999, 1.0, 0) || um_fires(0.0999, 1.0, 9) || !um_fires(0.1, 1.0, 9) || um_fires(0.1, 1.0, 8)) {
        ++failures;
        printf("FAIL schedule: the weight just below w_max / 10 fired in ten epochs, or the one at it did not fire in the last\n");
    }

    printf(failures ? "%d checks FAILED\n" : "umap host checks ok\n", failures);
    return failures ? 1 : 0;
}
