// Host-only check of the argument validation of sc_knn_cross (csrc/sc_neighbors.hip), sc_cross_vote and sc_cross_regress
// (csrc/sc_ingest.hip), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_ingest` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's arrays
// -- the finite checks of both feature arrays and of Y_ref, the range check of codes_ref -- on inputs sized exactly, so a
// read past an end is caught.  The two gathers need resident cross lists: their shape is written into the context here,
// which is all the refusals read.
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
    const int64_t nr = 40, nq = 7;
    const int32_t d = 3, k = 5;
    std::vector<double> R((size_t)nr * d), Q((size_t)nq * d);
    for (size_t p = 0; p < R.size(); ++p) R[p] = sin((double)p);
    for (size_t p = 0; p < Q.size(); ++p) Q[p] = cos((double)p);
    std::vector<float> Rf(R.begin(), R.end()), Qf(Q.begin(), Q.end());
    std::vector<int32_t> idx((size_t)nq * k);
    std::vector<double> d2((size_t)nq * k);
    int64_t info[4] = {-1, -1, -1, -1};
    auto cross = [&](sc_ctx *cc, const void *r, int tr, int64_t n_ref, const void *q, int tq, int64_t n_query, int32_t dd, int32_t kk,
                     int32_t path, int32_t slack, int64_t *inf) {
        return sc_knn_cross(cc, r, tr, n_ref, q, tq, n_query, dd, kk, path, slack, idx.data(), d2.data(), inf);
    };

    // ---- sc_knn_cross ----
    for (int path = 0; path <= 2; ++path) {   // the refusals do not depend on the path asked for
        expect("null ctx", cross(nullptr, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID, "null pointer");
        expect("null R", cross(c, nullptr, SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID, "null pointer");
        expect("null Q", cross(c, R.data(), SC_F64, nr, nullptr, SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID, "null pointer");
        expect("null info", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 0, nullptr), SC_ERR_INVALID, "null pointer");
        expect("dtype_r", cross(c, R.data(), 7, nr, Q.data(), SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID, "dtype_r and dtype_q");
        expect("dtype_q", cross(c, R.data(), SC_F64, nr, Q.data(), -1, nq, d, k, path, 0, info), SC_ERR_INVALID, "dtype_r and dtype_q");
        expect("d = 0", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, 0, k, path, 0, info), SC_ERR_INVALID, "1 <= d <= 64");
        expect("d = 65", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, 65, k, path, 0, info), SC_ERR_INVALID, "1 <= d <= 64");
        expect("k = 0", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, 0, path, 0, info), SC_ERR_INVALID, "1 <= k <= 32");
        expect("k = 33", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, 33, path, 0, info), SC_ERR_INVALID, "1 <= k <= 32");
        expect("n_ref < k", cross(c, R.data(), SC_F64, 4, Q.data(), SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID, "k <= n_ref");
        expect("n_ref > 2^31 - 1", cross(c, R.data(), SC_F64, (int64_t)1 << 31, Q.data(), SC_F64, nq, d, k, path, 0, info), SC_ERR_INVALID,
               "k <= n_ref <= 2^31 - 1");
        expect("n_query = 0", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, 0, d, k, path, 0, info), SC_ERR_INVALID, "1 <= n_query");
        expect("n_query * k", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, ((int64_t)1 << 29) / k + 1, d, k, path, 0, info), SC_ERR_INVALID,
               "n_query * k <= 2^29");
        expect("slack = -1", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, -1, info), SC_ERR_INVALID, "0 <= slack <= 16");
        expect("slack = 17", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 17, info), SC_ERR_INVALID, "0 <= slack <= 16");
        // the finite checks come last and read all of both arrays and no more: the very last value of each
        R[(size_t)nr * d - 1] = NAN;
        expect("R nan", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 1, info), SC_ERR_INVALID, "R: feature value 119");
        R[(size_t)nr * d - 1] = 0x1p500;
        expect("R huge", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 1, info), SC_ERR_INVALID, "R: feature value 119");
        R[(size_t)nr * d - 1] = 0.5;
        Q[(size_t)nq * d - 1] = -INFINITY;
        expect("Q -inf", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, path, 1, info), SC_ERR_INVALID, "Q: feature value 20");
        Q[(size_t)nq * d - 1] = 0.5;
        Rf[(size_t)nr * d - 1] = INFINITY;
        expect("R inf f32", cross(c, Rf.data(), SC_F32, nr, Q.data(), SC_F64, nq, d, k, path, 1, info), SC_ERR_INVALID, "R: feature value 119");
        Rf[(size_t)nr * d - 1] = 0.5f;
        Qf[(size_t)nq * d - 1] = NAN;
        expect("Q nan f32", cross(c, R.data(), SC_F64, nr, Qf.data(), SC_F32, nq, d, k, path, 1, info), SC_ERR_INVALID, "Q: feature value 20");
        Qf[(size_t)nq * d - 1] = 0.5f;
    }
    expect("path = -1", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, -1, 0, info), SC_ERR_INVALID, "path must be 0");
    expect("path = 3", cross(c, R.data(), SC_F64, nr, Q.data(), SC_F64, nq, d, k, 3, 0, info), SC_ERR_INVALID, "path must be 0");
    if (info[0] != -1 || info[3] != -1 || ctx.knn.valid || ctx.knn.cross) {
        ++failures;
        printf("FAIL a refused call wrote to info_out or claimed resident lists\n");
    }

    // ---- sc_cross_vote, sc_cross_regress ----
    std::vector<int32_t> codes((size_t)nr), label((size_t)nq);
    for (size_t j = 0; j < codes.size(); ++j) codes[j] = (int32_t)(j % 4);
    std::vector<double> conf((size_t)nq), proba((size_t)nq * 4), Y((size_t)nr * 2, 1.0), out((size_t)nq * 2);
    std::vector<float> Yf((size_t)nr * 2, 1.0f);
    expect("vote: no lists", sc_cross_vote(c, codes.data(), 4, SC_CROSS_UNIFORM, label.data(), conf.data(), nullptr), SC_ERR_STATE,
           "no cross lists are resident");
    expect("regress: no lists", sc_cross_regress(c, Y.data(), SC_F64, 2, SC_CROSS_UNIFORM, out.data()), SC_ERR_STATE,
           "no cross lists are resident");
    ctx.knn.valid = true;    // self lists are not cross lists
    expect("vote: self lists", sc_cross_vote(c, codes.data(), 4, SC_CROSS_UNIFORM, label.data(), conf.data(), nullptr), SC_ERR_STATE,
           "no cross lists are resident");
    ctx.knn.valid = false;
    ctx.knn.cross = true;    // the shape of resident cross lists: all that the refusals below read
    ctx.knn.n = nr, ctx.knn.nq = nq, ctx.knn.k = k;
    expect("vote: null ctx", sc_cross_vote(nullptr, codes.data(), 4, 0, label.data(), conf.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("vote: null codes", sc_cross_vote(c, nullptr, 4, 0, label.data(), conf.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("vote: null label", sc_cross_vote(c, codes.data(), 4, 0, nullptr, conf.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("vote: null conf", sc_cross_vote(c, codes.data(), 4, 0, label.data(), nullptr, nullptr), SC_ERR_INVALID, "null pointer");
    expect("vote: weighting", sc_cross_vote(c, codes.data(), 4, 2, label.data(), conf.data(), nullptr), SC_ERR_INVALID, "weighting must be");
    expect("vote: n_classes = 0", sc_cross_vote(c, codes.data(), 0, 0, label.data(), conf.data(), nullptr), SC_ERR_INVALID, "n_classes >= 1");
    ctx.knn.nq = (int64_t)1 << 27;
    expect("vote: proba size", sc_cross_vote(c, codes.data(), 4, 0, label.data(), conf.data(), proba.data()), SC_ERR_INVALID,
           "n_query * n_classes <= 2^28");
    ctx.knn.nq = nq;
    codes[(size_t)nr - 1] = 4;      // the very last code
    expect("vote: code = n_classes", sc_cross_vote(c, codes.data(), 4, 1, label.data(), conf.data(), proba.data()), SC_ERR_INVALID,
           "codes_ref[39] = 4");
    codes[(size_t)nr - 1] = -1;
    expect("vote: code = -1", sc_cross_vote(c, codes.data(), 4, 1, label.data(), conf.data(), nullptr), SC_ERR_INVALID, "codes_ref[39] = -1");
    codes[(size_t)nr - 1] = 0;

    expect("regress: null ctx", sc_cross_regress(nullptr, Y.data(), SC_F64, 2, 0, out.data()), SC_ERR_INVALID, "null pointer");
    expect("regress: null Y", sc_cross_regress(c, nullptr, SC_F64, 2, 0, out.data()), SC_ERR_INVALID, "null pointer");
    expect("regress: null out", sc_cross_regress(c, Y.data(), SC_F64, 2, 0, nullptr), SC_ERR_INVALID, "null pointer");
    expect("regress: weighting", sc_cross_regress(c, Y.data(), SC_F64, 2, -1, out.data()), SC_ERR_INVALID, "weighting must be");
    expect("regress: dtype", sc_cross_regress(c, Y.data(), 7, 2, 0, out.data()), SC_ERR_INVALID, "dtype");
    expect("regress: C = 0", sc_cross_regress(c, Y.data(), SC_F64, 0, 0, out.data()), SC_ERR_INVALID, "1 <= C <= 64");
    expect("regress: C = 65", sc_cross_regress(c, Y.data(), SC_F64, 65, 0, out.data()), SC_ERR_INVALID, "1 <= C <= 64");
    Y[(size_t)nr * 2 - 1] = NAN;    // the very last value
    expect("regress: nan", sc_cross_regress(c, Y.data(), SC_F64, 2, 1, out.data()), SC_ERR_INVALID, "Y_ref value 79");
    Y[(size_t)nr * 2 - 1] = 1.0;
    Yf[(size_t)nr * 2 - 1] = INFINITY;
    expect("regress: inf f32", sc_cross_regress(c, Yf.data(), SC_F32, 2, 1, out.data()), SC_ERR_INVALID, "Y_ref value 79");
    ctx.knn.cross = false;   // nothing is resident: the context's destructor frees no list

    printf(failures ? "%d checks FAILED\n" : "ingest host checks ok\n", failures);
    return failures ? 1 : 0;
}
