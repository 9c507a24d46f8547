// sc_ingest.hip -- what a query row takes from its nearest reference rows: a label by vote (sc_cross_vote) and values by
// weighted average (sc_cross_regress), both on the lists that sc_knn_cross (sc_neighbors.hip) left in ctx->knn
// (restated by tests/ingest_restated.py: vote, regress).  gfx950 only.
//
// fp64 throughout, -ffp-contract=off, no floating-point atomics: every sum runs over the k <= 32 entries of ONE row in list
// order (t ascending, the first term starts the sum), so a result is a function of the lists and the arguments alone.
// The weights have one home, k_ig_weights: uniform 1; "distance" 1 / sqrt(d2), and in a row that holds a zero distance 1
// for its zero-distance entries and 0 for the rest (sklearn's weights="distance").
#include <cmath>

#include "sc_dense_knn.h"

namespace {

constexpr int IG_QB = 64;   // queries per workgroup of the vote: their rows' classes and weights take 24 KiB of LDS
constexpr int IG_CMAX = 64; // columns of sc_cross_regress
constexpr int64_t IG_PROBA_MAX = (int64_t)1 << 28;   // entries of proba_out: 2 GiB

// w[q][t] for the nq * k list entries, one thread per query
__global__ __launch_bounds__(256) void k_ig_weights(const double *__restrict__ d2, int64_t nq, int k, int weighting, double *__restrict__ w)
{
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= nq) return;
    const double *row = d2 + q * k;
    double *out = w + q * k;
    bool zero = false;
    for (int t = 0; t < k; ++t) zero = zero || row[t] == 0.0;
    for (int t = 0; t < k; ++t) {
        double v = 1.0;
        if (weighting == SC_CROSS_DISTANCE) v = zero ? (row[t] == 0.0 ? 1.0 : 0.0) : 1.0 / sqrt(row[t]);
        out[t] = v;
    }
}

// One thread per query, its row's classes and weights in LDS ([t][thread]: conflict-free).  Entry t speaks for its class
// if no earlier entry has it; its class sum is then the weights of the later entries of the class, added in list order.
// The entries are compared among themselves, so n_classes appears only as the row stride of proba.
__global__ __launch_bounds__(IG_QB) void k_ig_vote(const int32_t *__restrict__ idx, const double *__restrict__ w, const int32_t *__restrict__ codes,
                                                   int64_t nq, int k, int64_t n_classes, int32_t *__restrict__ label, double *__restrict__ conf,
                                                   double *__restrict__ proba)
{
    __shared__ int cls[DF_KMAX * IG_QB];
    __shared__ double ws[DF_KMAX * IG_QB];
    const int th = threadIdx.x;
    const int64_t q = (int64_t)blockIdx.x * IG_QB + th;
    if (q >= nq) return;   // (no barrier below: a thread reads only what it wrote)
    double total = 0.0;
    for (int t = 0; t < k; ++t) {
        const double wt = w[q * k + t];
        cls[t * IG_QB + th] = codes[idx[q * k + t]];
        ws[t * IG_QB + th] = wt;
        total = t == 0 ? wt : total + wt;
    }
    int best = 0x7fffffff;
    double best_p = -1.0;
    for (int t = 0; t < k; ++t) {
        const int ct = cls[t * IG_QB + th];
        bool first = true;
        for (int u = 0; u < t; ++u) first = first && cls[u * IG_QB + th] != ct;
        if (!first) continue;
        double sum = ws[t * IG_QB + th];
        for (int u = t + 1; u < k; ++u)
            if (cls[u * IG_QB + th] == ct) sum = sum + ws[u * IG_QB + th];
        const double p = sum / total;
        if (proba) proba[q * n_classes + ct] = p;
        if (p > best_p || (p == best_p && ct < best)) { best_p = p; best = ct; }
    }
    label[q] = best;
    conf[q] = best_p;
}

// out[q][c] = (sum_t w_t Y[j_t][c]) / (sum_t w_t), one thread per (q, c), c fastest: a wavefront reads runs of Y's rows
template <class T>
__global__ __launch_bounds__(256) void k_ig_regress(const int32_t *__restrict__ idx, const double *__restrict__ w, const T *__restrict__ Y,
                                                    int64_t nq, int k, int C, double *__restrict__ out)
{
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= nq * C) return;
    const int64_t q = e / C;
    const int c = (int)(e % C);
    double num = 0.0, den = 0.0;
    for (int t = 0; t < k; ++t) {
        const double wt = w[q * k + t];
        const double term = wt * (double)Y[(int64_t)idx[q * k + t] * C + c];
        num = t == 0 ? term : num + term;
        den = t == 0 ? wt : den + wt;
    }
    out[e] = num / den;
}

// the gate both entry points share: the context, the weighting, the resident cross lists -- in that order
int ig_check(const char *who, sc_ctx *c, const void *ref, const void *out, int weighting)
{
    SC_REQUIRE(c && ref && out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_REQUIRE(weighting == SC_CROSS_UNIFORM || weighting == SC_CROSS_DISTANCE, SC_ERR_INVALID,
               "%s: weighting must be SC_CROSS_UNIFORM (0) or SC_CROSS_DISTANCE (1), got %d", who, weighting);
    SC_REQUIRE(c->knn.cross, SC_ERR_STATE, "%s: no cross lists are resident (call sc_knn_cross first)", who);
    return SC_OK;
}

// the weights of the resident lists into scratch_a
int ig_weights(sc_ctx *c, int weighting)
{
    const sc_ctx::DenseKnn &kn = c->knn;
    SC_TRY(c->scratch_a.ensure(sizeof(double) * (size_t)(kn.nq * kn.k), &c->mem));
    hipLaunchKernelGGL(k_ig_weights, dim3((unsigned)ceil_div64(kn.nq, 256)), dim3(256), 0, c->stream, kn.d2.as<double>(), kn.nq, kn.k,
                       weighting, c->scratch_a.as<double>());
    return SC_OK;
}

}  // namespace

extern "C" int sc_cross_vote(sc_ctx *c, const int32_t *codes_ref, int32_t n_classes, int32_t weighting, int32_t *label_out,
                             double *conf_out, double *proba_out)
{
    const char *who = "sc_cross_vote";
    SC_REQUIRE(conf_out, SC_ERR_INVALID, "%s: null pointer", who);
    SC_TRY(ig_check(who, c, codes_ref, label_out, weighting));
    const sc_ctx::DenseKnn &kn = c->knn;
    const int64_t n = kn.n, nq = kn.nq;
    SC_REQUIRE(n_classes >= 1, SC_ERR_INVALID, "%s: need n_classes >= 1, got %d", who, n_classes);
    SC_REQUIRE(!proba_out || nq * n_classes <= IG_PROBA_MAX, SC_ERR_INVALID, "%s: proba_out needs n_query * n_classes <= 2^28, got %lld", who,
               (long long)(nq * n_classes));
    for (int64_t j = 0; j < n; ++j)
        SC_REQUIRE(codes_ref[j] >= 0 && codes_ref[j] < n_classes, SC_ERR_INVALID, "%s: codes_ref[%lld] = %d is outside [0, %d)", who,
                   (long long)j, codes_ref[j], n_classes);
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t pbytes = proba_out ? sizeof(double) * (size_t)(nq * n_classes) : 0;
    SC_TRY(c->ig_ref.ensure(sizeof(int32_t) * (size_t)n, &c->mem));
    SC_TRY(c->ig_label.ensure(sizeof(int32_t) * (size_t)nq, &c->mem));
    SC_TRY(c->ig_conf.ensure(sizeof(double) * (size_t)nq, &c->mem));
    if (proba_out) SC_TRY(c->ig_out.ensure(pbytes, &c->mem));
    SC_HIP(hipMemcpyAsync(c->ig_ref.p, codes_ref, sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
    if (proba_out) SC_HIP(hipMemsetAsync(c->ig_out.p, 0, pbytes, s));   // the classes a row does not hold: +0
    {
        KernelTimerScope ts(c, SC_K_INGEST);
        SC_TRY(ig_weights(c, weighting));
        hipLaunchKernelGGL(k_ig_vote, dim3((unsigned)ceil_div64(nq, IG_QB)), dim3(IG_QB), 0, s, kn.idx.as<int32_t>(), c->scratch_a.as<double>(),
                           c->ig_ref.as<int32_t>(), nq, kn.k, (int64_t)n_classes, c->ig_label.as<int32_t>(), c->ig_conf.as<double>(),
                           proba_out ? c->ig_out.as<double>() : (double *)nullptr);
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(label_out, c->ig_label.p, sizeof(int32_t) * (size_t)nq, hipMemcpyDeviceToHost, s));
    SC_HIP(hipMemcpyAsync(conf_out, c->ig_conf.p, sizeof(double) * (size_t)nq, hipMemcpyDeviceToHost, s));
    if (proba_out) SC_HIP(hipMemcpyAsync(proba_out, c->ig_out.p, pbytes, hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}

extern "C" int sc_cross_regress(sc_ctx *c, const void *Y_ref, int dtype, int32_t C, int32_t weighting, double *out)
{
    const char *who = "sc_cross_regress";
    SC_TRY(ig_check(who, c, Y_ref, out, weighting));
    const sc_ctx::DenseKnn &kn = c->knn;
    const int64_t n = kn.n, nq = kn.nq;
    SC_REQUIRE(dtype == SC_F32 || dtype == SC_F64, SC_ERR_INVALID, "%s: dtype must be SC_F32 or SC_F64", who);
    SC_REQUIRE(C >= 1 && C <= IG_CMAX, SC_ERR_INVALID, "%s: need 1 <= C <= %d, got %d", who, IG_CMAX, C);
    for (int64_t p = 0; p < n * C; ++p) {
        const double v = dtype == SC_F32 ? (double)((const float *)Y_ref)[p] : ((const double *)Y_ref)[p];
        SC_REQUIRE(std::isfinite(v), SC_ERR_INVALID, "%s: Y_ref value %lld is not finite", who, (long long)p);
    }
    SC_HIP(hipSetDevice(c->device));
    hipStream_t s = c->stream;
    const size_t es = dtype == SC_F32 ? sizeof(float) : sizeof(double);
    SC_TRY(c->ig_raw.ensure(es * (size_t)(n * C), &c->mem));
    SC_TRY(c->ig_out.ensure(sizeof(double) * (size_t)(nq * C), &c->mem));
    SC_HIP(hipMemcpyAsync(c->ig_raw.p, Y_ref, es * (size_t)(n * C), hipMemcpyHostToDevice, s));
    {
        KernelTimerScope ts(c, SC_K_INGEST);
        SC_TRY(ig_weights(c, weighting));
        const dim3 grid((unsigned)ceil_div64(nq * C, 256)), tpb(256);
        if (dtype == SC_F32)
            hipLaunchKernelGGL(k_ig_regress<float>, grid, tpb, 0, s, kn.idx.as<int32_t>(), c->scratch_a.as<double>(), c->ig_raw.as<float>(), nq,
                               kn.k, (int)C, c->ig_out.as<double>());
        else
            hipLaunchKernelGGL(k_ig_regress<double>, grid, tpb, 0, s, kn.idx.as<int32_t>(), c->scratch_a.as<double>(), c->ig_raw.as<double>(), nq,
                               kn.k, (int)C, c->ig_out.as<double>());
    }
    SC_HIP(hipGetLastError());
    SC_HIP(hipMemcpyAsync(out, c->ig_out.p, sizeof(double) * (size_t)(nq * C), hipMemcpyDeviceToHost, s));
    SC_HIP(hipStreamSynchronize(s));
    return SC_OK;
}
