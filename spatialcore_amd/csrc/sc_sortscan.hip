// sc_sortscan.hip -- sc_sortscan.h: hipcub's device-wide radix sort and exclusive scan behind one size-query / ensure / call
// each, and k_run_heads.  Counts are size_t at every call.  gfx950 only.
#include <hipcub/hipcub.hpp>

#include "sc_sortscan.h"

namespace {

typedef unsigned long long u64;

__global__ __launch_bounds__(256) void k_run_heads(const u64 *__restrict__ keys, int64_t total, long long *__restrict__ heads)
{
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p > total) return;
    heads[p] = (p < total && (p == 0 || keys[p] != keys[p - 1])) ? 1 : 0;
}

}  // namespace

template <class K, class V>
int sc_sort_pairs(sc_ctx *c, DBuf &tmp, hipStream_t s, const K *k_in, K *k_out, const V *v_in, V *v_out, int64_t cnt, int end_bit)
{
    size_t bytes = 0;
    SC_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, k_in, k_out, v_in, v_out, (size_t)cnt, 0, end_bit, s));
    SC_TRY(tmp.ensure(bytes, &c->mem));
    SC_HIP(hipcub::DeviceRadixSort::SortPairs(tmp.p, bytes, k_in, k_out, v_in, v_out, (size_t)cnt, 0, end_bit, s));
    return SC_OK;
}

// ranksum's value pairs and its dense-form ids, the 64-bit keys of ranksum, the thresholds, the column sort, the list graph
// and Louvain, the bin sort of the neighbour searches
template int sc_sort_pairs<u64, uint16_t>(sc_ctx *, DBuf &, hipStream_t, const u64 *, u64 *, const uint16_t *, uint16_t *, int64_t, int);
template int sc_sort_pairs<uint32_t, uint32_t>(sc_ctx *, DBuf &, hipStream_t, const uint32_t *, uint32_t *, const uint32_t *, uint32_t *, int64_t, int);
template int sc_sort_pairs<u64, uint32_t>(sc_ctx *, DBuf &, hipStream_t, const u64 *, u64 *, const uint32_t *, uint32_t *, int64_t, int);
template int sc_sort_pairs<uint32_t, int32_t>(sc_ctx *, DBuf &, hipStream_t, const uint32_t *, uint32_t *, const int32_t *, int32_t *, int64_t, int);

int sc_exclusive_sum(sc_ctx *c, DBuf &tmp, hipStream_t s, long long *counts, long long *offsets, int64_t n_plus_1)
{
    size_t bytes = 0;
    SC_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, counts, offsets, (size_t)n_plus_1, s));
    SC_TRY(tmp.ensure(bytes, &c->mem));
    SC_HIP(hipcub::DeviceScan::ExclusiveSum(tmp.p, bytes, counts, offsets, (size_t)n_plus_1, s));
    return SC_OK;
}

void sc_run_heads(hipStream_t s, const u64 *keys, int64_t total, long long *heads)
{
    hipLaunchKernelGGL(k_run_heads, dim3((unsigned)ceil_div64(total + 1, 256)), dim3(256), 0, s, keys, total, heads);
}
