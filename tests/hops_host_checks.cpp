// Host-only check of the sc_hop_* entry points (csrc/sc_hops.hip), meant for the sanitizer build:
// `make -C spatialcore_amd/csrc asan_hops` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is sc_hop_begin's walk over the caller's CSR --
// on arrays sized exactly, so a read past an end is caught -- and the call-order checks of the other entry points.
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
    // four cells: 0 -> 1, 2; 1 -> 0; 2 -> nothing; 3 -> 0, 1, 2 (directed on purpose); then one defect at a time
    const int64_t p[5] = {0, 2, 3, 3, 6};
    const int32_t i[6] = {1, 2, 0, 0, 1, 2};

    // ---- null pointers and n ----
    expect("null ctx", sc_hop_begin(nullptr, p, i, 4), SC_ERR_INVALID, "sc_hop_begin: null pointer");
    expect("null indptr", sc_hop_begin(c, nullptr, i, 4), SC_ERR_INVALID, "sc_hop_begin: null pointer");
    expect("null indices", sc_hop_begin(c, p, nullptr, 4), SC_ERR_INVALID, "sc_hop_begin: null pointer");
    expect("n = 0", sc_hop_begin(c, p, i, 0), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got 0");
    expect("n < 0", sc_hop_begin(c, p, i, -3), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got -3");
    expect("n = 2^31", sc_hop_begin(c, p, i, (int64_t)1 << 31), SC_ERR_INVALID, "need 1 <= n <= 2^31 - 1, got 2147483648");   // refused on n: nothing is read

    // ---- indptr ----
    {
        const int64_t q[5] = {1, 2, 3, 3, 6};
        expect("indptr[0]", sc_hop_begin(c, q, i, 4), SC_ERR_INVALID, "indptr[0] must be 0, got 1");
    }
    {
        const int64_t q[5] = {0, 2, 1, 3, 6};
        expect("indptr decreases", sc_hop_begin(c, q, i, 4), SC_ERR_INVALID, "indptr decreases at row 1");
    }
    {
        const int64_t q[5] = {0, 2, 3, 3, 2};   // the very last entry; no column is read
        expect("indptr decreases at the end", sc_hop_begin(c, q, i, 4), SC_ERR_INVALID, "indptr decreases at row 3");
    }

    // ---- the columns, one defect at a time ----
    {
        const int32_t j[6] = {2, 1, 0, 0, 1, 2};
        expect("unsorted", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 0: columns are not strictly ascending");
    }
    {
        const int32_t j[6] = {1, 2, 0, 0, 2, 2};   // the very last entry repeats the one before
        expect("duplicate", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 3: columns are not strictly ascending");
    }
    {
        const int32_t j[6] = {1, 2, 1, 0, 1, 2};
        expect("diagonal", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 1 holds a diagonal entry");
    }
    {
        const int32_t j[6] = {1, 2, 0, 0, 1, 3};   // the very last entry
        expect("diagonal at the end", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 3 holds a diagonal entry");
    }
    {
        const int32_t j[6] = {1, 4, 0, 0, 1, 2};
        expect("column = n", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 0: column 4 is outside 0 .. n - 1");
    }
    {
        const int32_t j[6] = {-1, 2, 0, 0, 1, 2};
        expect("negative column", sc_hop_begin(c, p, j, 4), SC_ERR_INVALID, "row 0: column -1 is outside 0 .. n - 1");
    }
    {
        const int64_t q[2] = {0, 1};             // one cell: its only possible column is the diagonal
        const int32_t j[1] = {0};
        expect("one cell", sc_hop_begin(c, q, j, 1), SC_ERR_INVALID, "row 0 holds a diagonal entry");
    }

    // ---- out of order: nothing is resident (every refused sc_hop_begin above left it so) ----
    int64_t nnz = -1, empty = -1, ptr_out[5];
    int32_t longest = -1, idx_out[6];
    double X[8] = {0, 1, 2, 3, 4, 5, 6, 7}, out[8], ms[4];
    expect("next before begin", sc_hop_next(c, &nnz, &longest, &empty), SC_ERR_STATE, "sc_hop_next: no graph is resident (sc_hop_begin)");
    expect("get before begin", sc_hop_get(c, ptr_out, idx_out), SC_ERR_STATE, "sc_hop_get: no graph is resident (sc_hop_begin)");
    expect("aggregate before begin", sc_hop_aggregate(c, X, SC_F64, 2, SC_HOP_MEAN, out), SC_ERR_STATE,
           "sc_hop_aggregate: no graph is resident (sc_hop_begin)");
    expect("times before begin", sc_hop_times(c, ms), SC_ERR_STATE, "sc_hop_times: no graph is resident (sc_hop_begin)");
    expect("end before begin", sc_hop_end(c), SC_OK, nullptr);   // nothing to free is no error, as with the other _end calls
    if (nnz != -1 || longest != -1 || empty != -1) {
        ++failures;
        printf("FAIL a refused sc_hop_next wrote its outputs\n");
    }

    // ---- the other entry points' arguments (checked before the state) ----
    expect("next null", sc_hop_next(c, nullptr, &longest, &empty), SC_ERR_INVALID, "sc_hop_next: null pointer");
    expect("next null ctx", sc_hop_next(nullptr, &nnz, &longest, &empty), SC_ERR_INVALID, "sc_hop_next: null pointer");
    expect("get null", sc_hop_get(c, ptr_out, nullptr), SC_ERR_INVALID, "sc_hop_get: null pointer");
    expect("aggregate null X", sc_hop_aggregate(c, nullptr, SC_F64, 2, SC_HOP_MEAN, out), SC_ERR_INVALID, "sc_hop_aggregate: null pointer");
    expect("aggregate null out", sc_hop_aggregate(c, X, SC_F64, 2, SC_HOP_MEAN, nullptr), SC_ERR_INVALID, "sc_hop_aggregate: null pointer");
    expect("aggregate dtype", sc_hop_aggregate(c, X, 7, 2, SC_HOP_MEAN, out), SC_ERR_INVALID, "dtype must be SC_F32 or SC_F64");
    expect("aggregate d = 0", sc_hop_aggregate(c, X, SC_F64, 0, SC_HOP_MEAN, out), SC_ERR_INVALID, "need 1 <= d <= 64, got 0");
    expect("aggregate d = 65", sc_hop_aggregate(c, X, SC_F64, 65, SC_HOP_MEAN, out), SC_ERR_INVALID, "need 1 <= d <= 64, got 65");
    expect("aggregate what = 0", sc_hop_aggregate(c, X, SC_F64, 2, 0, out), SC_ERR_INVALID, "what must be SC_HOP_MEAN or SC_HOP_VAR, got 0");
    expect("aggregate what = 3", sc_hop_aggregate(c, X, SC_F64, 2, 3, out), SC_ERR_INVALID, "what must be SC_HOP_MEAN or SC_HOP_VAR, got 3");
    expect("times null", sc_hop_times(c, nullptr), SC_ERR_INVALID, "sc_hop_times: null pointer");
    expect("end null", sc_hop_end(nullptr), SC_ERR_INVALID, "sc_hop_end: null pointer");

    printf(failures ? "%d checks FAILED\n" : "hops host checks ok\n", failures);
    return failures ? 1 : 0;
}
