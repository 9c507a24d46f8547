// Host-only check of the gate a caller's CSR passes in sc_nmf_fit, sc_annot_predict and sc_annot_train_begin
// (csrc/sc_csr_input.h), meant for the sanitizer build: `make -C spatialcore_amd/csrc asan_sparse` links this program (its
// own main, nothing preloaded) against the AddressSanitizer + UBSan objects and runs it.  The context is constructed on
// the host and every call below is refused before its first HIP call, so no device is needed or touched: what runs is the
// host code that reads the caller's arrays -- the offsets, the column walk, the value check -- on inputs sized exactly, so
// a read past an end is caught.  Every case names the return code and the message, entry point included.
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <string>
#include <vector>

#include "sc_permgen.h"   // completes sc_ctx (its pipeline member) for a host-side instance

static int failures = 0;

static void expect(const std::string &what, int rc, int want, const std::string &fragment)
{
    const char *msg = sc_last_error();
    if (rc != want || !strstr(msg, fragment.c_str())) {
        ++failures;
        printf("FAIL %s: rc=%d (want %d), message \"%s\" (want \"%s\")\n", what.c_str(), rc, want, msg, fragment.c_str());
    }
}

// one entry point with everything but the matrix fixed: three cells over four genes
typedef std::function<int(const int64_t *, const int32_t *, const void *, int)> Entry;

static void gate(const std::string &who, const Entry &call, bool needs_entries)
{
    const int64_t good_ptr[4] = {0, 2, 2, 5};
    const int32_t good_idx[5] = {0, 3, 1, 2, 3};
    const double good_val[5] = {1.0, 2.0, 0.5, 3.0, 4.0};
    const float good_f32[5] = {1.f, 2.f, 0.5f, 3.f, 4.f};
    auto bad = [&](const char *what, int rc, const char *fragment) { expect(who + " " + what, rc, SC_ERR_INVALID, who + ": " + fragment); };

    bad("null indptr", call(nullptr, good_idx, good_val, SC_F64), "null pointer");
    bad("null indices", call(good_ptr, nullptr, good_val, SC_F64), "null pointer");
    bad("null data", call(good_ptr, good_idx, nullptr, SC_F64), "null pointer");
    bad("dtype", call(good_ptr, good_idx, good_val, 7), "dtype must be SC_F32 or SC_F64");
    {
        const int64_t p[4] = {1, 2, 2, 5};
        bad("indptr[0]", call(p, good_idx, good_val, SC_F64), "indptr[0] must be 0");
    }
    {
        const int64_t p[4] = {0, 2, 1, 5};
        bad("decreasing offset", call(p, good_idx, good_val, SC_F64), "indptr decreases at row 1");
    }
    {
        const int32_t i[5] = {0, 4, 1, 2, 3};
        bad("column = n_genes", call(good_ptr, i, good_val, SC_F64), "row 0 is not canonical (columns must ascend strictly inside [0, n_genes))");
    }
    {
        const int32_t i[5] = {0, 3, 1, 2, -1};      // the very last entry: the walk reads all five and no more
        bad("negative column", call(good_ptr, i, good_f32, SC_F32), "row 2 is not canonical (columns must ascend strictly inside [0, n_genes))");
    }
    {
        const int32_t i[5] = {0, 3, 2, 2, 3};
        bad("repeated column", call(good_ptr, i, good_val, SC_F64), "row 2 is not canonical");
    }
    {
        const int32_t i[5] = {3, 0, 1, 2, 3};
        bad("unsorted row", call(good_ptr, i, good_f32, SC_F32), "row 0 is not canonical");
    }
    {
        const double v[5] = {1.0, 2.0, 0.5, 3.0, NAN};
        bad("nan f64", call(good_ptr, good_idx, v, SC_F64), "stored value 4 is not finite");
    }
    {
        const float v[5] = {1.f, 2.f, 0.5f, 3.f, NAN};
        bad("nan f32", call(good_ptr, good_idx, v, SC_F32), "stored value 4 is not finite");
    }
    {
        const float v[5] = {INFINITY, 2.f, 0.5f, 3.f, 4.f};
        bad("inf f32", call(good_ptr, good_idx, v, SC_F32), "stored value 0 is not finite");
    }
    {
        const double v[5] = {1.0, -2.0, 0.5, 3.0, 4.0};
        bad("negative f64", call(good_ptr, good_idx, v, SC_F64), "stored value 1 is negative");
    }
    {
        const float v[5] = {1.f, 2.f, 0.5f, 3.f, -4.f};
        bad("negative f32", call(good_ptr, good_idx, v, SC_F32), "stored value 4 is negative");
    }
    {
        const int32_t i[5] = {0, 4, 1, 2, 3};      // two defects: the column is reported, not the value behind it
        const double v[5] = {NAN, 2.0, 0.5, 3.0, 4.0};
        bad("column before value", call(good_ptr, i, v, SC_F64), "row 0 is not canonical");
    }
    if (needs_entries) {
        const int64_t p[4] = {0, 0, 0, 0};      // no stored entry: refused before indices and data are looked at
        bad("no stored entry", call(p, nullptr, nullptr, SC_F64), "need 1 <= stored entries <= 2^32 - 1, got 0");
    }
}

int main()
{
    sc_ctx ctx;
    sc_ctx *c = &ctx;
    const int64_t n = 3;
    const int32_t G = 4, K = 2, T = 2;

    std::vector<double> W((size_t)n * K, 1.0), H((size_t)K * G, 1.0), trace(8);
    int32_t n_checks = 0, n_iter = 0;
    double err = 0.0;
    gate("sc_nmf_fit", [&](const int64_t *p, const int32_t *i, const void *v, int dtype) {
        return sc_nmf_fit(c, p, i, v, dtype, n, G, K, 2, 1, 1, 0.0, W.data(), H.data(), trace.data(), &n_checks, &n_iter, &err);
    }, true);

    std::vector<double> coef((size_t)T * G, 0.5), intercept(T, 0.0), mean(G, 0.0), scale(G, 1.0), conf((size_t)n * 5);
    std::vector<float> scores((size_t)n * T);
    std::vector<int32_t> labels(n, 0);
    gate("sc_annot_predict", [&](const int64_t *p, const int32_t *i, const void *v, int dtype) {
        return sc_annot_predict(c, p, i, v, dtype, n, G, 0, T, coef.data(), intercept.data(), mean.data(), scale.data(), scores.data(),
                                labels.data(), conf.data());
    }, false);      // a batch of empty cells is legal there

    std::vector<double> weights(n, 1.0), mean_out(G), scale_out(G);
    gate("sc_annot_train_begin", [&](const int64_t *p, const int32_t *i, const void *v, int dtype) {
        return sc_annot_train_begin(c, p, i, v, dtype, n, G, 0, T, labels.data(), weights.data(), mean_out.data(), scale_out.data());
    }, true);

    printf(failures ? "%d checks FAILED\n" : "sparse host checks ok\n", failures);
    return failures ? 1 : 0;
}
