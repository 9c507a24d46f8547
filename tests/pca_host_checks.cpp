// Host-only check of the sc_pca_* entry points' argument validation (csrc/sc_pca.hip), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_pca` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's
// arrays -- the CSR walk, the finite checks, the state checks -- on inputs sized exactly, so a read past an end is caught.
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
    // three cells over four genes, then one defect at a time
    const int64_t good_ptr[4] = {0, 2, 2, 5};
    const int32_t good_idx[5] = {0, 3, 1, 2, 3};
    const double good_val[5] = {1.0, -2.0, 0.5, 3.0, 4.0};
    const float good_f32[5] = {1.f, 2.f, 0.5f, 3.f, 4.f};
    auto begin = [&](const int64_t *p, const int32_t *i, const void *v, int dtype, int64_t n, int32_t G, int32_t norm, double ts) {
        return sc_pca_begin(c, p, i, v, dtype, n, G, norm, ts);
    };

    // ---- sc_pca_begin ----
    expect("begin null ctx", sc_pca_begin(nullptr, good_ptr, good_idx, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "null pointer");
    expect("begin null indptr", begin(nullptr, good_idx, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "null pointer");
    expect("begin null indices", begin(good_ptr, nullptr, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "null pointer");
    expect("begin null data", begin(good_ptr, good_idx, nullptr, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "null pointer");
    expect("begin dtype", begin(good_ptr, good_idx, good_val, 7, 3, 4, 0, 1e4), SC_ERR_INVALID, "dtype");
    expect("begin n = 1", begin(good_ptr, good_idx, good_val, SC_F64, 1, 4, 0, 1e4), SC_ERR_INVALID, "2 <= n <= 2^31 - 1");
    expect("begin n = 2^31", begin(good_ptr, good_idx, good_val, SC_F64, (int64_t)1 << 31, 4, 0, 1e4), SC_ERR_INVALID, "2 <= n <= 2^31 - 1");
    expect("begin G = 0", begin(good_ptr, good_idx, good_val, SC_F64, 3, 0, 0, 1e4), SC_ERR_INVALID, "1 <= n_genes <= 4096");
    expect("begin G = 4097", begin(good_ptr, good_idx, good_val, SC_F64, 3, 4097, 0, 1e4), SC_ERR_INVALID, "1 <= n_genes <= 4096");
    expect("begin target_sum = 0", begin(good_ptr, good_idx, good_f32, SC_F32, 3, 4, 1, 0.0), SC_ERR_INVALID, "target_sum");
    expect("begin target_sum nan", begin(good_ptr, good_idx, good_f32, SC_F32, 3, 4, 1, NAN), SC_ERR_INVALID, "target_sum");
    {
        const int64_t p[4] = {1, 2, 2, 5};
        expect("begin indptr[0]", begin(p, good_idx, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "indptr[0]");
    }
    {
        const int64_t p[4] = {0, 2, 1, 5};
        expect("begin decreasing", begin(p, good_idx, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "indptr decreases at row 1");
    }
    {
        const int32_t i[5] = {0, 4, 1, 2, 3};
        expect("begin index = G", begin(good_ptr, i, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "row 0 is not canonical");
    }
    {
        const int32_t i[5] = {0, 3, 1, 2, -1};
        expect("begin negative index", begin(good_ptr, i, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "row 2 is not canonical");
    }
    {
        const int32_t i[5] = {0, 3, 2, 2, 3};
        expect("begin repeated column", begin(good_ptr, i, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "row 2 is not canonical");
    }
    {
        const int32_t i[5] = {3, 0, 1, 2, 3};
        expect("begin unsorted", begin(good_ptr, i, good_val, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "row 0 is not canonical");
    }
    {
        const double v[5] = {1.0, -2.0, 0.5, 3.0, NAN};      // the very last value: the check reads all five and no more
        expect("begin nan", begin(good_ptr, good_idx, v, SC_F64, 3, 4, 0, 1e4), SC_ERR_INVALID, "stored value 4 is not finite");
    }
    {
        const float v[5] = {1.f, 2.f, 0.5f, 3.f, INFINITY};
        expect("begin inf f32", begin(good_ptr, good_idx, v, SC_F32, 3, 4, 0, 1e4), SC_ERR_INVALID, "stored value 4 is not finite");
    }
    expect("begin negative with normalize", begin(good_ptr, good_idx, good_val, SC_F64, 3, 4, 1, 1e4), SC_ERR_INVALID, "stored value 1 is negative");

    // ---- sc_pca_gram / _project / _end: nothing is resident ----
    std::vector<double> colsum(4), gram(16), V(2 * 4, 0.5), off(2, 0.0), out(3 * 2);
    expect("gram null ctx", sc_pca_gram(nullptr, colsum.data(), gram.data()), SC_ERR_INVALID, "null pointer");
    expect("gram null colsum", sc_pca_gram(c, nullptr, gram.data()), SC_ERR_INVALID, "null pointer");
    expect("gram null gram", sc_pca_gram(c, colsum.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("gram before begin", sc_pca_gram(c, colsum.data(), gram.data()), SC_ERR_STATE, "no matrix is resident");
    expect("values null", sc_pca_values(c, nullptr), SC_ERR_INVALID, "null pointer");
    expect("values before begin", sc_pca_values(c, colsum.data()), SC_ERR_STATE, "no matrix is resident");
    expect("project null ctx", sc_pca_project(nullptr, V.data(), off.data(), 2, SC_F64, out.data()), SC_ERR_INVALID, "null pointer");
    expect("project null V", sc_pca_project(c, nullptr, off.data(), 2, SC_F64, out.data()), SC_ERR_INVALID, "null pointer");
    expect("project null offset", sc_pca_project(c, V.data(), nullptr, 2, SC_F64, out.data()), SC_ERR_INVALID, "null pointer");
    expect("project null out", sc_pca_project(c, V.data(), off.data(), 2, SC_F64, nullptr), SC_ERR_INVALID, "null pointer");
    expect("project K = 0", sc_pca_project(c, V.data(), off.data(), 0, SC_F64, out.data()), SC_ERR_INVALID, "1 <= K <= 64");
    expect("project K = 65", sc_pca_project(c, V.data(), off.data(), 65, SC_F64, out.data()), SC_ERR_INVALID, "1 <= K <= 64");
    expect("project out_dtype", sc_pca_project(c, V.data(), off.data(), 2, 9, out.data()), SC_ERR_INVALID, "out_dtype");
    expect("project before begin", sc_pca_project(c, V.data(), off.data(), 2, SC_F64, out.data()), SC_ERR_STATE, "no matrix is resident");
    expect("end null ctx", sc_pca_end(nullptr), SC_ERR_INVALID, "null pointer");
    expect("end without begin", sc_pca_end(c), SC_OK, nullptr);

    printf(failures ? "%d checks FAILED\n" : "pca host checks ok\n", failures);
    return failures ? 1 : 0;
}
