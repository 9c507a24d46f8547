// Host-only check of the dense search's argument validation, sc_knn_dense and sc_knn_dense_gram (csrc/sc_neighbors.hip:
// one gate for both), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_neighbors` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's array
// -- the finite check -- on inputs sized exactly, so a read past an end is caught.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <vector>

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
    const int64_t n = 40;
    std::vector<double> X((size_t)n * 3);
    for (size_t p = 0; p < X.size(); ++p) X[p] = sin((double)p);
    std::vector<float> Xf(X.begin(), X.end());
    std::vector<int32_t> idx((size_t)n * 5);
    std::vector<double> d2((size_t)n * 5);
    int64_t info[4] = {-1, -1, -1, -1};
    auto gram = [&](sc_ctx *cc, const void *x, int dtype, int64_t rows, int32_t d, int32_t k, int32_t path, int32_t slack, int64_t *inf) {
        return sc_knn_dense_gram(cc, x, dtype, rows, d, k, path, slack, idx.data(), d2.data(), inf);
    };

    // ---- sc_knn_dense ----
    expect("knn null ctx", sc_knn_dense(nullptr, X.data(), SC_F64, n, 3, 5, 0, idx.data(), d2.data()), SC_ERR_INVALID, "null pointer");
    expect("knn null X", sc_knn_dense(c, nullptr, SC_F64, n, 3, 5, 0, idx.data(), d2.data()), SC_ERR_INVALID, "null pointer");
    expect("knn dtype", sc_knn_dense(c, X.data(), 7, n, 3, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "dtype");
    expect("knn d = 0", sc_knn_dense(c, X.data(), SC_F64, n, 0, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "1 <= d <= 64");
    expect("knn d = 65", sc_knn_dense(c, X.data(), SC_F64, n, 65, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "1 <= d <= 64");
    expect("knn k = 1", sc_knn_dense(c, X.data(), SC_F64, n, 3, 1, 0, nullptr, nullptr), SC_ERR_INVALID, "2 <= k <= 32");
    expect("knn k = 33", sc_knn_dense(c, X.data(), SC_F64, n, 3, 33, 0, nullptr, nullptr), SC_ERR_INVALID, "2 <= k <= 32");
    expect("knn n = k", sc_knn_dense(c, X.data(), SC_F64, 5, 3, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "k < n");
    expect("knn n * k", sc_knn_dense(c, X.data(), SC_F64, (int64_t)1 << 27, 3, 8, 0, nullptr, nullptr), SC_ERR_INVALID, "n * k");
    expect("knn splits", sc_knn_dense(c, X.data(), SC_F64, n, 3, 5, -1, nullptr, nullptr), SC_ERR_INVALID, "splits");
    expect("knn splits", sc_knn_dense(c, X.data(), SC_F64, n, 3, 5, 65536, nullptr, nullptr), SC_ERR_INVALID, "splits");
    X[(size_t)n * 3 - 1] = NAN;      // the very last value: the check reads all n * d of them and no more
    expect("knn nan", sc_knn_dense(c, X.data(), SC_F64, n, 3, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "feature value 119");
    X[(size_t)n * 3 - 1] = 0x1p500;
    expect("knn huge", sc_knn_dense(c, X.data(), SC_F64, n, 3, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "feature value 119");
    X[(size_t)n * 3 - 1] = 0.5;
    Xf[(size_t)n * 3 - 1] = INFINITY;
    expect("knn inf f32", sc_knn_dense(c, Xf.data(), SC_F32, n, 3, 5, 0, nullptr, nullptr), SC_ERR_INVALID, "feature value 119");
    Xf[(size_t)n * 3 - 1] = 0.5f;

    // ---- sc_knn_dense_gram ----
    for (int path = 0; path <= 2; ++path) {   // the refusals do not depend on the path asked for
        expect("null ctx", gram(nullptr, X.data(), SC_F64, n, 3, 5, path, 0, info), SC_ERR_INVALID, "null pointer");
        expect("null X", gram(c, nullptr, SC_F64, n, 3, 5, path, 0, info), SC_ERR_INVALID, "null pointer");
        expect("null info", gram(c, X.data(), SC_F64, n, 3, 5, path, 0, nullptr), SC_ERR_INVALID, "null pointer");
        expect("dtype", gram(c, X.data(), 7, n, 3, 5, path, 0, info), SC_ERR_INVALID, "dtype");
        expect("d = 0", gram(c, X.data(), SC_F64, n, 0, 5, path, 0, info), SC_ERR_INVALID, "1 <= d <= 64");
        expect("d = 65", gram(c, X.data(), SC_F64, n, 65, 5, path, 0, info), SC_ERR_INVALID, "1 <= d <= 64");
        expect("k = 1", gram(c, X.data(), SC_F64, n, 3, 1, path, 0, info), SC_ERR_INVALID, "2 <= k <= 32");
        expect("k = 33", gram(c, X.data(), SC_F64, n, 3, 33, path, 0, info), SC_ERR_INVALID, "2 <= k <= 32");
        expect("n = k", gram(c, X.data(), SC_F64, 5, 3, 5, path, 0, info), SC_ERR_INVALID, "k < n");
        expect("n * k", gram(c, X.data(), SC_F64, (int64_t)1 << 27, 3, 8, path, 0, info), SC_ERR_INVALID, "n * k");
        expect("n > 2^31 - 1", gram(c, X.data(), SC_F64, (int64_t)1 << 31, 3, 2, path, 0, info), SC_ERR_INVALID, "k < n <= 2^31 - 1");
        expect("slack = -1", gram(c, X.data(), SC_F64, n, 3, 5, path, -1, info), SC_ERR_INVALID, "0 <= slack <= 16");
        expect("slack = 17", gram(c, X.data(), SC_F64, n, 3, 5, path, 17, info), SC_ERR_INVALID, "0 <= slack <= 16");
        X[(size_t)n * 3 - 1] = NAN;      // the very last value: the check reads all n * d of them and no more
        expect("nan", gram(c, X.data(), SC_F64, n, 3, 5, path, 1, info), SC_ERR_INVALID, "feature value 119");
        X[(size_t)n * 3 - 1] = 0x1p500;
        expect("huge", gram(c, X.data(), SC_F64, n, 3, 5, path, 1, info), SC_ERR_INVALID, "feature value 119");
        X[(size_t)n * 3 - 1] = -INFINITY;
        expect("-inf", gram(c, X.data(), SC_F64, n, 3, 5, path, 1, info), SC_ERR_INVALID, "feature value 119");
        X[(size_t)n * 3 - 1] = 0.5;
        Xf[(size_t)n * 3 - 1] = INFINITY;
        expect("inf f32", gram(c, Xf.data(), SC_F32, n, 3, 5, path, 1, info), SC_ERR_INVALID, "feature value 119");
        Xf[(size_t)n * 3 - 1] = 0.5f;
    }
    expect("path = -1", gram(c, X.data(), SC_F64, n, 3, 5, -1, 0, info), SC_ERR_INVALID, "path must be 0");
    expect("path = 3", gram(c, X.data(), SC_F64, n, 3, 5, 3, 0, info), SC_ERR_INVALID, "path must be 0");
    // a refused call leaves the caller's record alone and no list claimed resident
    if (info[0] != -1 || info[3] != -1 || ctx.knn.valid) {
        ++failures;
        printf("FAIL a refused call wrote to info_out or claimed resident lists\n");
    }

    printf(failures ? "%d checks FAILED\n" : "neighbors host checks ok\n", failures);
    return failures ? 1 : 0;
}
