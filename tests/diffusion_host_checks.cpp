// Host-only check of the diffusion entry points' argument validation (csrc/sc_diffusion.hip), meant for the sanitizer
// build: `make -C spatialcore_amd/csrc asan_diffusion` links this program (its own main, nothing preloaded) against the
// AddressSanitizer + UBSan objects and runs it.  The context is constructed on the host and every call below is refused
// before its first HIP call, so no device is needed or touched: what runs is the host code that reads the caller's
// arrays -- the CSR walk, the finite checks, the state checks -- on inputs sized exactly, so a read past an end is caught.
// (sc_knn_dense's gate: tests/neighbors_host_checks.cpp, next to sc_knn_dense_gram's.)
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

    // ---- sc_diffmap_graph / _get: nothing is resident ----
    int64_t edges = 0, comps = 0;
    expect("graph null", sc_diffmap_graph(c, nullptr, nullptr, &comps), SC_ERR_INVALID, "null pointer");
    expect("graph state", sc_diffmap_graph(c, nullptr, &edges, &comps), SC_ERR_STATE, "no neighbour lists");
    std::vector<int64_t> ip(4);
    std::vector<int32_t> ix(4);
    std::vector<double> w(4);
    expect("get null", sc_diffmap_graph_get(c, nullptr, ix.data(), w.data(), nullptr), SC_ERR_INVALID, "null pointer");
    expect("get state", sc_diffmap_graph_get(c, ip.data(), ix.data(), w.data(), nullptr), SC_ERR_STATE, "no graph");

    // ---- sc_diffmap_graph_csr: a path of three cells, then one defect at a time ----
    const int64_t good_ptr[4] = {0, 1, 3, 4};
    const int32_t good_idx[4] = {1, 0, 2, 1};
    const double good_w[4] = {1.0, 1.0, 0.5, 0.5};
    auto csr = [&](const int64_t *p, const int32_t *i, const double *v, int64_t rows) {
        return sc_diffmap_graph_csr(c, p, i, v, rows, &comps);
    };
    expect("csr null", sc_diffmap_graph_csr(c, good_ptr, good_idx, good_w, 3, nullptr), SC_ERR_INVALID, "null pointer");
    expect("csr n = 1", csr(good_ptr, good_idx, good_w, 1), SC_ERR_INVALID, "2 <= n");
    {
        const int64_t p[4] = {1, 1, 3, 4};
        expect("csr indptr[0]", csr(p, good_idx, good_w, 3), SC_ERR_INVALID, "indptr[0]");
    }
    {
        const int64_t p[4] = {0, 1, 1, 4};
        expect("csr empty row", csr(p, good_idx, good_w, 3), SC_ERR_INVALID, "row 1 is empty");
    }
    {
        const int64_t p[4] = {0, 2, 1, 4};
        expect("csr decreasing", csr(p, good_idx, good_w, 3), SC_ERR_INVALID, "row 1 is empty");
    }
    {
        const int32_t i[4] = {1, 0, 3, 1};
        expect("csr column range", csr(good_ptr, i, good_w, 3), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const int32_t i[4] = {1, 2, 0, 1};
        expect("csr unsorted", csr(good_ptr, i, good_w, 3), SC_ERR_INVALID, "row 1 is not canonical");
    }
    {
        const int32_t i[4] = {-1, 0, 2, 1};
        expect("csr negative column", csr(good_ptr, i, good_w, 3), SC_ERR_INVALID, "row 0 is not canonical");
    }
    {
        const double v[4] = {1.0, 1.0, 0.5, 0.0};
        expect("csr zero value", csr(good_ptr, good_idx, v, 3), SC_ERR_INVALID, "stored value 3");
    }
    {
        const double v[4] = {1.0, 1.0, 0.5, NAN};
        expect("csr nan value", csr(good_ptr, good_idx, v, 3), SC_ERR_INVALID, "stored value 3");
    }
    {
        const double v[4] = {-1.0, 1.0, 0.5, 0.5};
        expect("csr negative value", csr(good_ptr, good_idx, v, 3), SC_ERR_INVALID, "stored value 0");
    }

    // ---- Lanczos: nothing is open ----
    std::vector<double> start((size_t)n, 1.0), alpha(8), beta(9), S(8), lam(2), vecs(2 * (size_t)n), res(2);
    int64_t m = 0;
    expect("begin null", sc_lanczos_begin(c, nullptr, 4), SC_ERR_INVALID, "null pointer");
    expect("begin state", sc_lanczos_begin(c, start.data(), 4), SC_ERR_STATE, "no transition matrix");
    expect("run null", sc_lanczos_run(c, 1, nullptr, beta.data(), &m), SC_ERR_INVALID, "null pointer");
    expect("run state", sc_lanczos_run(c, 1, alpha.data(), beta.data(), &m), SC_ERR_STATE, "no Lanczos run");
    expect("ritz null", sc_lanczos_ritz(c, nullptr, 4, 2, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "null pointer");
    expect("ritz state", sc_lanczos_ritz(c, S.data(), 4, 2, lam.data(), vecs.data(), res.data()), SC_ERR_STATE, "no Lanczos run");
    expect("end null", sc_lanczos_end(nullptr), SC_ERR_INVALID, "null context");

    // the checks behind the state checks, on a context that claims a graph and an open run of 4 steps over 40 cells
    // (claims only: each of these calls is refused before it would touch the device)
    ctx.lg.n = n;
    ctx.lg.valid = true;
    expect("begin max_basis = 0", sc_lanczos_begin(c, start.data(), 0), SC_ERR_INVALID, "1 <= max_basis <= n");
    expect("begin max_basis > n", sc_lanczos_begin(c, start.data(), n + 1), SC_ERR_INVALID, "1 <= max_basis <= n");
    start[(size_t)n - 1] = INFINITY;
    expect("begin inf", sc_lanczos_begin(c, start.data(), 4), SC_ERR_INVALID, "start value 39");
    std::fill(start.begin(), start.end(), 0.0);
    expect("begin zero", sc_lanczos_begin(c, start.data(), 4), SC_ERR_INVALID, "all zero");
    ctx.lz.valid = true;
    ctx.lz.m = 4;
    ctx.lz.max_basis = 4;
    expect("run negative", sc_lanczos_run(c, -1, alpha.data(), beta.data(), &m), SC_ERR_INVALID, "exceed the basis");
    expect("run past the basis", sc_lanczos_run(c, 1, alpha.data(), beta.data(), &m), SC_ERR_INVALID, "exceed the basis");
    expect("ritz m = 0", sc_lanczos_ritz(c, S.data(), 0, 2, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "1 <= m <= 4");
    expect("ritz m = 5", sc_lanczos_ritz(c, S.data(), 5, 2, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "1 <= m <= 4");
    expect("ritz columns = 0", sc_lanczos_ritz(c, S.data(), 4, 0, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "columns");
    expect("ritz columns = 65", sc_lanczos_ritz(c, S.data(), 4, 65, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "columns");
    S[7] = NAN;                       // the last of the m x c = 8 coefficients
    expect("ritz nan coefficient", sc_lanczos_ritz(c, S.data(), 4, 2, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID,
           "coefficient 7");
    S[7] = 0.0;
    lam[1] = INFINITY;
    expect("ritz inf lambda", sc_lanczos_ritz(c, S.data(), 4, 2, lam.data(), vecs.data(), res.data()), SC_ERR_INVALID, "lambda[1]");

    printf(failures ? "%d checks FAILED\n" : "diffusion host checks ok\n", failures);
    return failures ? 1 : 0;
}
