// Host-only check of the sc_louvain_* entry points' argument validation (csrc/sc_louvain.hip), meant for the sanitizer
// build: `make -C spatialcore_amd/csrc asan_louvain` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's
// arrays -- the CSR walk, the weight range, the mirror search of the symmetry check, the state checks -- on inputs sized
// exactly, so a read past an end is caught.
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
    // a path 0 - 1 - 2 with a loop at 2 and the isolated vertex 3, then one defect at a time
    const int64_t good_ptr[5] = {0, 1, 3, 5, 5};
    const int32_t good_idx[5] = {1, 0, 2, 1, 2};
    const uint16_t good_q[5] = {7, 7, 65535, 65535, 1};
    const int32_t g1 = 1 << 16;
    auto begin = [&](const int64_t *p, const int32_t *i, const uint16_t *q, int64_t n, int32_t g, int32_t rounds) {
        return sc_louvain_begin(c, p, i, q, n, g, rounds);
    };

    // ---- sc_louvain_begin ----
    expect("begin null ctx", sc_louvain_begin(nullptr, good_ptr, good_idx, good_q, 4, g1, 500), SC_ERR_INVALID, "null pointer");
    expect("begin null indptr", begin(nullptr, good_idx, good_q, 4, g1, 500), SC_ERR_INVALID, "null pointer");
    expect("begin null indices", begin(good_ptr, nullptr, good_q, 4, g1, 500), SC_ERR_INVALID, "null pointer");
    expect("begin null weights", begin(good_ptr, good_idx, nullptr, 4, g1, 500), SC_ERR_INVALID, "null pointer");
    expect("begin n = 0", begin(good_ptr, good_idx, good_q, 0, g1, 500), SC_ERR_INVALID, "1 <= n <= 2^31 - 1");
    expect("begin n = 2^31", begin(good_ptr, good_idx, good_q, (int64_t)1 << 31, g1, 500), SC_ERR_INVALID, "1 <= n <= 2^31 - 1");
    expect("begin g = 0", begin(good_ptr, good_idx, good_q, 4, 0, 500), SC_ERR_INVALID, "resolution");
    expect("begin g = 2^23 + 1", begin(good_ptr, good_idx, good_q, 4, (1 << 23) + 1, 500), SC_ERR_INVALID, "resolution");
    expect("begin max_rounds = 0", begin(good_ptr, good_idx, good_q, 4, g1, 0), SC_ERR_INVALID, "max_rounds");
    {
        const int64_t p[5] = {1, 1, 3, 5, 5};
        expect("begin indptr[0]", begin(p, good_idx, good_q, 4, g1, 500), SC_ERR_INVALID, "indptr[0]");
    }
    {
        const int64_t p[5] = {0, 3, 1, 5, 5};
        expect("begin decreasing", begin(p, good_idx, good_q, 4, g1, 500), SC_ERR_INVALID, "indptr decreases at row 1");
    }
    {
        const int64_t p[2] = {0, (int64_t)1 << 31};
        expect("begin nnz = 2^31", begin(p, good_idx, good_q, 1, g1, 500), SC_ERR_INVALID, "stored entries <= 2^31 - 1");
    }
    {
        const int32_t i[5] = {1, 0, 2, 1, 4};
        expect("begin index = n", begin(good_ptr, i, good_q, 4, g1, 500), SC_ERR_INVALID, "row 2 is not canonical");
    }
    {
        const int32_t i[5] = {-1, 0, 2, 1, 2};
        expect("begin negative index", begin(good_ptr, i, good_q, 4, g1, 500), SC_ERR_INVALID, "row 0 is not canonical");
    }
    {
        const int32_t i[5] = {1, 2, 0, 1, 2};
        expect("begin unsorted", begin(good_ptr, i, good_q, 4, g1, 500), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const int32_t i[5] = {1, 0, 0, 1, 2};
        expect("begin repeated column", begin(good_ptr, i, good_q, 4, g1, 500), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const uint16_t q[5] = {7, 7, 65535, 65535, 0};       // the very last weight: the check reads all five and no more
        expect("begin weight 0", begin(good_ptr, good_idx, q, 4, g1, 500), SC_ERR_INVALID, "weight 4 (row 2, column 2) is 0");
    }
    {
        const int32_t i[5] = {1, 0, 3, 1, 2};                // (1, 3) is stored, row 3 is empty: the mirror search sees an empty range
        expect("begin asymmetric structure", begin(good_ptr, i, good_q, 4, g1, 500), SC_ERR_INVALID, "entry (1, 3) is stored, (3, 1) is not");
    }
    {
        const int64_t p[5] = {0, 1, 2, 4, 4};                // (2, 1) is stored, row 1 holds only (1, 0)
        const int32_t i[4] = {1, 0, 1, 2};
        const uint16_t q[4] = {7, 7, 9, 1};
        expect("begin asymmetric structure 2", begin(p, i, q, 4, g1, 500), SC_ERR_INVALID, "entry (2, 1) is stored, (1, 2) is not");
    }
    {
        const uint16_t q[5] = {7, 7, 65535, 65534, 1};
        expect("begin asymmetric value", begin(good_ptr, good_idx, q, 4, g1, 500), SC_ERR_INVALID, "entry (1, 2) weighs 65535, (2, 1) weighs 65534");
    }

    // ---- the calls that need a state: nothing is resident ----
    std::vector<int64_t> info(12);
    std::vector<int32_t> lab(4);
    std::vector<double> w(5);
    int64_t nc = 0;
    expect("resident_weights null ctx", sc_louvain_resident_weights(nullptr, w.data(), 5), SC_ERR_INVALID, "null pointer");
    expect("resident_weights null out", sc_louvain_resident_weights(c, nullptr, 5), SC_ERR_INVALID, "null pointer");
    expect("resident_weights no graph", sc_louvain_resident_weights(c, w.data(), 5), SC_ERR_STATE, "no graph is resident");
    expect("begin_resident null ctx", sc_louvain_begin_resident(nullptr, good_q, 5, g1, 500), SC_ERR_INVALID, "null pointer");
    expect("begin_resident g", sc_louvain_begin_resident(c, good_q, 5, 0, 500), SC_ERR_INVALID, "resolution");
    expect("begin_resident max_rounds", sc_louvain_begin_resident(c, good_q, 5, g1, -1), SC_ERR_INVALID, "max_rounds");
    expect("begin_resident no graph", sc_louvain_begin_resident(c, good_q, 5, g1, 500), SC_ERR_STATE, "no graph is resident");
    expect("level null ctx", sc_louvain_level(nullptr, info.data(), lab.data()), SC_ERR_INVALID, "null pointer");
    expect("level null info", sc_louvain_level(c, nullptr, lab.data()), SC_ERR_INVALID, "null pointer");
    expect("level before begin", sc_louvain_level(c, info.data(), lab.data()), SC_ERR_STATE, "no graph is resident");
    expect("labels null ctx", sc_louvain_labels(nullptr, lab.data(), &nc), SC_ERR_INVALID, "null pointer");
    expect("labels null out", sc_louvain_labels(c, nullptr, &nc), SC_ERR_INVALID, "null pointer");
    expect("labels null count", sc_louvain_labels(c, lab.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("labels before begin", sc_louvain_labels(c, lab.data(), &nc), SC_ERR_STATE, "no graph is resident");
    expect("end null ctx", sc_louvain_end(nullptr), SC_ERR_INVALID, "null pointer");
    expect("end without begin", sc_louvain_end(c), SC_OK, nullptr);

    printf(failures ? "%d checks FAILED\n" : "louvain host checks ok\n", failures);
    return failures ? 1 : 0;
}
