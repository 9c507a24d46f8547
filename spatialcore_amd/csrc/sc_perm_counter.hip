// ------------------------------------------------------------------------------------------------
// Counter-based permutations (r03; SURVEY 8(e) "alternative", H2) for the paths that have NO reference seed semantics
// (label-permutation enrichment, shared-permutation Lee grids): permutation p is a pure function of (seed, p), so ranks
// and batches can take disjoint ranges of p and merge integer counts.  Definition (documented, reproducible, the same
// on any number of GPUs): Fisher-Yates as numpy runs it -- for i = n-1 .. 1: j uniform on [0, i]; swap a[i], a[j] -- with
//   j = bounded(Philox4x32-10(key = (seed low word, seed high word), counter = (i, r, p low, p high)), i + 1)
// where the first two output words form a 64-bit u and bounded is Lemire's multiply-shift with its exact rejection
// (u * (i + 1) >> 64, rejected -- retry with r + 1 -- when the low half falls below 2^64 mod (i + 1): probability < 2^-43
// per draw, so r is 0 in practice and the draw stays a pure function of its counter).  No sequential stage at all: J is
// filled by the whole chip, the swaps are the generator's stage B (sc_swaps.hip).  gfx950 only.
// ------------------------------------------------------------------------------------------------
#include "sc_permgen.h"
#include "sc_philox.h"

__host__ __device__ static inline uint32_t counter_bounded(uint32_t k0, uint32_t k1, uint64_t p, uint32_t i)
{
    const uint64_t range = (uint64_t)i + 1;
    for (uint32_t r = 0;; ++r) {
        uint32_t c[4] = {i, r, (uint32_t)p, (uint32_t)(p >> 32)};
        philox4x32_10(c, k0, k1);
        const uint64_t u = ((uint64_t)c[1] << 32) | c[0];
        const u128 m = (u128)u * range;
        const uint64_t low = (uint64_t)m;
        if (low >= range || low >= (0 - range) % range) return (uint32_t)(m >> 64);
    }
}

// J[(p - p_first) * M + (M - i)] = the swap partner of step i of permutation p (the layout stage B reads)
__global__ __launch_bounds__(256) void k_counter_J(uint32_t k0, uint32_t k1, uint32_t n, uint64_t p_first, int64_t n_perm,
                                                   int32_t *__restrict__ J)
{
    const uint32_t M = n - 1;
    const int64_t total = n_perm * (int64_t)M;
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = t / M;
        const uint32_t s = (uint32_t)(t - p * M);
        J[t] = (int32_t)counter_bounded(k0, k1, p_first + (uint64_t)p, M - s);
    }
}

extern "C" int sc_perm_counter_host(uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int32_t *perm_out)
{
    SC_REQUIRE(perm_out || n_perm == 0 || n == 0, SC_ERR_INVALID, "sc_perm_counter_host: null pointer");
    SC_REQUIRE(n >= 0 && n <= 0x7fffffffLL && n_perm >= 0 && p_first >= 0, SC_ERR_INVALID, "sc_perm_counter_host: bad sizes");
    for (int64_t p = 0; p < n_perm; ++p) {
        int32_t *a = perm_out + p * n;
        for (int64_t i = 0; i < n; ++i) a[i] = (int32_t)i;
        for (int64_t i = n - 1; i >= 1; --i) {
            const uint32_t j = counter_bounded((uint32_t)seed, (uint32_t)(seed >> 32), (uint64_t)(p_first + p), (uint32_t)i);
            const int32_t t = a[j]; a[j] = a[i]; a[i] = t;
        }
    }
    return SC_OK;
}

// rows [0, n_perm) of the (already allocated, >= n_perm rows) table <- counter-based permutations p_first .., on stream s
int sc_perm_counter_rows(sc_ctx *c, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, hipStream_t s)
{
    if (n_perm <= 0) return SC_OK;
    if (n == 1) {
        SC_HIP(hipMemsetAsync(c->perm.p, 0, sizeof(int32_t) * (size_t)(c->p_stride * n_perm), s));
        return SC_OK;
    }
    const int64_t M = n - 1;
    SC_TRY(c->pg.J.ensure(sizeof(int32_t) * (size_t)(M * n_perm + 64), &c->mem));
    const int64_t total = M * n_perm;
    const unsigned grid = (unsigned)(ceil_div64(total, 256) < 65536 ? ceil_div64(total, 256) : 65536);
    hipLaunchKernelGGL(k_counter_J, dim3(grid), dim3(256), 0, s, (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)n,
                       (uint64_t)p_first, n_perm, c->pg.J.as<int32_t>());
    return swaps_launch(c, c->perm.as<int32_t>(), n, 0, n_perm, false, 1, false, s);   // (permgen_swap_chunk's A/B switches do not apply)
}

extern "C" int sc_perm_generate_counter(sc_ctx *c, uint64_t seed, int64_t n, int64_t p_first, int64_t n_perm, int32_t *perm_out)
{
    SC_REQUIRE(c, SC_ERR_INVALID, "sc_perm_generate_counter: null context");
    SC_REQUIRE(p_first >= 0, SC_ERR_INVALID, "sc_perm_generate_counter: negative first permutation");
    SC_HIP(hipSetDevice(c->device));
    SC_TRY(sc_perm_alloc(c, n, n_perm));
    {
        KernelTimerScope ts(c, SC_K_PERMGEN);
        SC_TRY(sc_perm_counter_rows(c, seed, n, p_first, n_perm, c->stream));
    }
    c->p_count = n_perm;
    c->perm_bijective = true;
    c->perm_forward_valid = true;
    if (perm_out)
        SC_HIP(hipMemcpy2DAsync(perm_out, sizeof(int32_t) * (size_t)n, c->perm.p, sizeof(int32_t) * (size_t)c->p_stride,
                                sizeof(int32_t) * (size_t)n, (size_t)n_perm, hipMemcpyDeviceToHost, c->stream));
    SC_HIP(hipStreamSynchronize(c->stream));
    return SC_OK;
}
