// sc_csr_input.h -- the gate a caller's CSR passes on the host before anything reaches the device, and the matrix as it
// then lies on the device: shared by sc_nmf.hip, sc_annotate.hip and sc_pca.hip; the
// column walk also by sc_louvain.hip, sc_diffusion.hip and sc_umap.hip.  A canonical CSR: indptr[0] == 0, offsets that
// never decrease, columns strictly ascending inside a row and inside [0, bound).  The null checks and the limits on
// the stored entries differ per entry point and stay there, between the offsets and the columns.  Every message names
// the entry point (`who`) first.
#pragma once

#include <cmath>

#include "sc_ctx.h"

namespace {

// indptr[0] == 0 and non-decreasing offsets; *nnz = indptr[n]
inline int csr_check_offsets(const char *who, const int64_t *indptr, int64_t n, int64_t *nnz)
{
    SC_REQUIRE(indptr[0] == 0, SC_ERR_INVALID, "%s: indptr[0] must be 0", who);
    for (int64_t i = 0; i < n; ++i)
        SC_REQUIRE(indptr[i + 1] >= indptr[i], SC_ERR_INVALID, "%s: indptr decreases at row %lld", who, (long long)i);
    *nnz = indptr[n];
    return SC_OK;
}

// Columns strictly ascending inside a row and inside [0, bound), rows and entries in order.  per_entry(i, p) runs after the
// column check of entry p of row i and returns SC_OK or the entry point's own refusal (a weight, a value), so that of two
// defects the earlier entry's is reported, and of one entry's the column.
template <class PerEntry>
int csr_check_columns(const char *who, const int64_t *indptr, const int32_t *indices, int64_t n, int64_t bound, const char *bound_name,
                      PerEntry per_entry)
{
    for (int64_t i = 0; i < n; ++i)
        for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) {
            SC_REQUIRE(indices[p] >= 0 && indices[p] < bound && (p == indptr[i] || indices[p] > indices[p - 1]), SC_ERR_INVALID,
                       "%s: row %lld is not canonical (columns must ascend strictly inside [0, %s))", who, (long long)i, bound_name);
            SC_TRY(per_entry(i, p));
        }
    return SC_OK;
}
inline int csr_check_columns(const char *who, const int64_t *indptr, const int32_t *indices, int64_t n, int64_t bound, const char *bound_name)
{
    return csr_check_columns(who, indptr, indices, n, bound, bound_name, [](int64_t, int64_t) { return SC_OK; });
}

// every stored value finite and, with nonneg, >= 0; `note` ends the second message
template <class V>
int csr_check_values(const char *who, const V *data, int64_t nnz, bool nonneg, const char *note)
{
    for (int64_t p = 0; p < nnz; ++p) {
        const double x = (double)data[p];
        SC_REQUIRE(std::isfinite(x), SC_ERR_INVALID, "%s: stored value %lld is not finite", who, (long long)p);
        SC_REQUIRE(!nonneg || x >= 0.0, SC_ERR_INVALID, "%s: stored value %lld is negative%s", who, (long long)p, note);
    }
    return SC_OK;
}
inline int csr_check_values(const char *who, const void *data, int dtype, int64_t nnz, bool nonneg, const char *note)
{
    return dtype == SC_F32 ? csr_check_values(who, (const float *)data, nnz, nonneg, note)
                           : csr_check_values(who, (const double *)data, nnz, nonneg, note);
}

// The matrix on the device: the CSR, the values as the caller stored them (float or double) and their fp64 form, which
// the module's own values kernel writes after upload().
struct CsrDevice {
    DBuf indptr, indices, raw, val;
    int64_t n = 0, nnz = 0;
    // sizes the four buffers (an empty matrix keeps one element each) and enqueues the three copies on c->stream; the
    // caller's arrays are in use until the stream has been waited for
    int upload(sc_ctx *c, const int64_t *h_indptr, const int32_t *h_indices, const void *h_data, int dtype, int64_t rows, int64_t entries)
    {
        n = rows, nnz = entries;
        const size_t es = dtype == SC_F32 ? sizeof(float) : sizeof(double), cap = (size_t)(nnz ? nnz : 1);
        SC_TRY(indptr.ensure(sizeof(int64_t) * (size_t)(n + 1), &c->mem));
        SC_TRY(indices.ensure(sizeof(int32_t) * cap, &c->mem));
        SC_TRY(raw.ensure(es * cap, &c->mem));
        SC_TRY(val.ensure(sizeof(double) * cap, &c->mem));
        SC_HIP(hipMemcpyAsync(indptr.p, h_indptr, sizeof(int64_t) * (size_t)(n + 1), hipMemcpyHostToDevice, c->stream));
        if (nnz) {
            SC_HIP(hipMemcpyAsync(indices.p, h_indices, sizeof(int32_t) * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
            SC_HIP(hipMemcpyAsync(raw.p, h_data, es * (size_t)nnz, hipMemcpyHostToDevice, c->stream));
        }
        return SC_OK;
    }
};

}  // namespace
