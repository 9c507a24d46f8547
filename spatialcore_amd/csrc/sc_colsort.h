// sc_colsort.h -- the column-sorted copy of a canonical CSR and its chunk table, shared by sc_nmf.hip and
// sc_annotate.hip.  A stable device sort by column keeps the rows ascending inside a column; a
// gene column's stored entries are then cut into chunks of COL_CHUNK entries, the work items of every pass over columns.
// The sort and the tables do no floating-point arithmetic: the values are carried, never combined.  k_chunk_add is
// what both files finish a chunked sum with (column chunks here, cell chunks there): the chunk sums in chunk order.
#pragma once

#include "sc_sortscan.h"

namespace {

constexpr int COL_CHUNK = 512;   // stored entries of a gene column per work item of a column pass

// column chunk c: its gene g and the range [p0, p1) of its entries in the column-sorted copy
struct ColChunk {
    int32_t g;
    int64_t p0, p1;
};
__device__ __forceinline__ ColChunk col_chunk(const int64_t *__restrict__ colptr, const int64_t *__restrict__ cptr,
                                              const int32_t *__restrict__ cgene, int64_t c)
{
    const int32_t g = cgene[c];
    const int64_t p0 = colptr[g] + (c - cptr[g]) * COL_CHUNK;
    const int64_t pe = colptr[g + 1];
    return {g, p0, p0 + COL_CHUNK < pe ? p0 + COL_CHUNK : pe};
}

// per stored entry: sort key = its column, payload = its position
__global__ __launch_bounds__(256) void k_cs_keys(const int32_t *__restrict__ indices, int64_t nnz, unsigned long long *__restrict__ keys,
                                                 uint32_t *__restrict__ pos)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    keys[p] = (unsigned long long)indices[p];
    pos[p] = (uint32_t)p;
}
// per row (one thread): the row id of its entries
__global__ __launch_bounds__(256) void k_cs_rowids(const int64_t *__restrict__ indptr, int64_t n, int32_t *__restrict__ rowid)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t p = indptr[i]; p < indptr[i + 1]; ++p) rowid[p] = (int32_t)i;
}
// the column-sorted copy (the sort is stable, so rows ascend inside a column)
__global__ __launch_bounds__(256) void k_cs_fill(const uint32_t *__restrict__ pos, const int32_t *__restrict__ rowid,
                                                 const double *__restrict__ val, int64_t nnz, int32_t *__restrict__ crow,
                                                 double *__restrict__ cval)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= nnz) return;
    const uint32_t q = pos[p];
    crow[p] = rowid[q];
    cval[p] = val[q];
}
// colptr[g] = first sorted position whose column is >= g, g = 0 .. G
__global__ __launch_bounds__(256) void k_cs_colptr(const unsigned long long *__restrict__ keys, int64_t nnz, int G,
                                                   int64_t *__restrict__ colptr)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (keys[mid] < (unsigned long long)g) lo = mid + 1; else hi = mid;
    }
    colptr[g] = lo;
}
// cptr[g] = first chunk of gene g (cptr[G] = number of chunks): one thread, G <= 32768
__global__ void k_cs_chunk_scan(const int64_t *__restrict__ colptr, int G, int64_t *__restrict__ cptr)
{
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int64_t c = 0;
    for (int g = 0; g < G; ++g) {
        cptr[g] = c;
        c += (colptr[g + 1] - colptr[g] + COL_CHUNK - 1) / COL_CHUNK;
    }
    cptr[G] = c;
}
__global__ __launch_bounds__(256) void k_cs_chunk_fill(const int64_t *__restrict__ cptr, int G, int32_t *__restrict__ cgene)
{
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= G) return;
    for (int64_t c = cptr[g]; c < cptr[g + 1]; ++c) cgene[c] = g;
}

// out[e] = part[chunk][e] added in chunk order
__global__ __launch_bounds__(256) void k_chunk_add(const double *__restrict__ part, int64_t chunks, int P, double *__restrict__ out)
{
    const int e = blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= P) return;
    double s = 0.0;
    for (int64_t c = 0; c < chunks; ++c) s = s + part[c * P + e];
    out[e] = s;
}

// The column-sorted copy of one matrix: crow / cval = row and value of the sorted entries, gene = their columns (the
// sorted keys), colptr[G + 1], cptr[G + 1] = first chunk of every gene, cgene[chunks] = gene of every chunk.
struct ColSort {
    DBuf keys, gene, pos, pos2, rowid, crow, cval, colptr, cptr, cgene;
    int64_t chunks = 0;
};

// Allocates the arrays for nnz stored entries and G genes (everything but cgene, whose size is known after the scan).
inline int colsort_alloc(sc_ctx *c, ColSort &cs, int64_t nnz, int G)
{
    typedef unsigned long long u64;
    SC_TRY(cs.keys.ensure(sizeof(u64) * (size_t)nnz, &c->mem));
    SC_TRY(cs.gene.ensure(sizeof(u64) * (size_t)nnz, &c->mem));
    SC_TRY(cs.pos.ensure(sizeof(uint32_t) * (size_t)nnz, &c->mem));
    SC_TRY(cs.pos2.ensure(sizeof(uint32_t) * (size_t)nnz, &c->mem));
    SC_TRY(cs.rowid.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem));
    SC_TRY(cs.crow.ensure(sizeof(int32_t) * (size_t)nnz, &c->mem));
    SC_TRY(cs.cval.ensure(sizeof(double) * (size_t)nnz, &c->mem));
    SC_TRY(cs.colptr.ensure(sizeof(int64_t) * (size_t)(G + 1), &c->mem));
    SC_TRY(cs.cptr.ensure(sizeof(int64_t) * (size_t)(G + 1), &c->mem));
    return SC_OK;
}
// Enqueues the sort and the chunk scan of the device CSR (indptr, indices, val) on c->stream; no host wait.
inline int colsort_enqueue(sc_ctx *c, ColSort &cs, const int64_t *indptr, const int32_t *indices, const double *val, int64_t n,
                           int G, int64_t nnz)
{
    typedef unsigned long long u64;
    hipStream_t s = c->stream;
    const dim3 per_entry((unsigned)ceil_div64(nnz, 256)), per_gene((unsigned)ceil_div64(G + 1, 256)), tpb(256);
    hipLaunchKernelGGL(k_cs_keys, per_entry, tpb, 0, s, indices, nnz, cs.keys.as<u64>(), cs.pos.as<uint32_t>());
    hipLaunchKernelGGL(k_cs_rowids, dim3((unsigned)ceil_div64(n, 256)), tpb, 0, s, indptr, n, cs.rowid.as<int32_t>());
    SC_TRY(sc_sort_pairs(c, c->rs_tmp, s, cs.keys.as<u64>(), cs.gene.as<u64>(), cs.pos.as<uint32_t>(), cs.pos2.as<uint32_t>(), nnz,
                         sc_bits_for(G)));
    hipLaunchKernelGGL(k_cs_fill, per_entry, tpb, 0, s, cs.pos2.as<uint32_t>(), cs.rowid.as<int32_t>(), val, nnz, cs.crow.as<int32_t>(),
                       cs.cval.as<double>());
    hipLaunchKernelGGL(k_cs_colptr, per_gene, tpb, 0, s, cs.gene.as<u64>(), nnz, G, cs.colptr.as<int64_t>());
    hipLaunchKernelGGL(k_cs_chunk_scan, dim3(1), dim3(64), 0, s, cs.colptr.as<int64_t>(), G, cs.cptr.as<int64_t>());
    return SC_OK;
}
// Reads the chunk count back (waits for c->stream), checks it and enqueues the chunk -> gene table.
inline int colsort_finish(sc_ctx *c, ColSort &cs, int G, int64_t nnz, const char *who)
{
    hipStream_t s = c->stream;
    int64_t chunks = 0;
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(&chunks, cs.cptr.as<int64_t>() + G, sizeof(int64_t), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    SC_REQUIRE(chunks >= 1 && chunks <= nnz / COL_CHUNK + G, SC_ERR_HIP, "%s: column chunk count %lld out of range", who,
               (long long)chunks);
    cs.chunks = chunks;
    SC_TRY(cs.cgene.ensure(sizeof(int32_t) * (size_t)chunks, &c->mem));
    hipLaunchKernelGGL(k_cs_chunk_fill, dim3((unsigned)ceil_div64(G, 256)), dim3(256), 0, s, cs.cptr.as<int64_t>(), G, cs.cgene.as<int32_t>());
    return SC_OK;
}

}  // namespace
