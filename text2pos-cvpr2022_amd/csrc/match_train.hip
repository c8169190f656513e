// Fine stage in train() mode: the pieces of SuperGlue.forward that are not row GEMMs or BatchNorm, and the two loss values of
// training/fine.py.
//
// Replaces (reference): MultiHeadedAttention / attention models/superglue.py:90-116 (t2p_match_attention), the score matrix,
// log_optimal_transport and the mutual-nearest-neighbour matches of SuperGlue.forward models/superglue.py:149-177, :283-322
// (t2p_match_head), MatchingLoss.forward training/losses.py:20-30 (t2p_matching_loss) and nn.MSELoss() of training/fine.py:57-59
// (t2p_mse_loss).
//
// In train() mode the BatchNorm of AttentionalPropagation takes its statistics over ALL object tokens of the batch in one call and
// over all hint tokens in a second one, so the training path (train_match.py) keeps the tokens SET-major: rows
//   [0, B M)            object tokens, sample-major (row b M + i)
//   [B M, B (M + N))    hint tokens, sample-major   (row B M + b N + j)
// and a BatchNorm call is one contiguous row segment (train_ops.bn_relu_train).  match.hip's k_attn / k_match_final address
// sample-major rows [B (M + N)] and fold BatchNorm; the kernels here address the two sets.
//
// Everything is small and latency-bound (a sample is at most 63 + 63 tokens): the kernels aim at being exact, deterministic (no
// atomics, fixed reduction orders) and in bounds at every 1 <= M, N <= 63, D in {64, 128, 256}.
//   * attention: one workgroup per (sample, target set, head), one work item per target token.  The head's key / value slices of
//     the source set sit in LDS (at most 63 x 64 x 2 floats = 32 KiB) next to the score rows (16 KiB): the whole range of sizes
//     fits the default 64 KiB, where one workgroup per sample with all q | k | v rows resident (k_attn) would need 390 KiB at
//     63 + 63 tokens and D = 256.
//   * head: one wavefront per sample, the coupling matrix in LDS.  Scores, the log-Sinkhorn iterations and the final log
//     couplings are carried in float64 - in train() mode the matcher saturates (couplings from 8 down to 1e-47 at two layers), and
//     fifty iterations of fp32 logsumexp on values of that size would spend the error budget of the whole forward.
//   * losses: one workgroup each, terms accumulated in float64 in a fixed order.
#include "t2p_common.h"

#include "../../include/t2p.h"

namespace t2p {
namespace {

constexpr int kHeads = 4;
constexpr int kMaxTokens = 63;   // per set: a wavefront's lanes cover a set plus its dustbin

__device__ __forceinline__ int64_t set_row(int set, int64_t b, int64_t B, int M, int N) {
    return set == 0 ? b * M : B * M + b * N;   // first row of sample b's tokens of that set
}

// grid = B * 2 * heads, 64 threads.  qkv rows [B (M + N)][3D] (q | k | v), channel c of a projection = d * heads + h.
template <int DH>
__global__ __launch_bounds__(64) void k_attn_sets(const float* __restrict__ qkv, int64_t B, int M, int N, int cross,
                                                  float* __restrict__ msg) {
    constexpr int D = DH * kHeads;
    extern __shared__ float sm[];
    const int h = blockIdx.x % kHeads;
    const int tset = (blockIdx.x / kHeads) % 2;              // target set: 0 objects, 1 hints
    const int64_t b = blockIdx.x / (2 * kHeads);
    const int sset = cross ? 1 - tset : tset;                // source set
    const int nt = tset == 0 ? M : N, ns = sset == 0 ? M : N;
    const int64_t t0 = set_row(tset, b, B, M, N), s0 = set_row(sset, b, B, M, N);
    const int LS = ns | 1;                                   // odd pitch: the score rows of neighbouring lanes start in different banks
    float* K = sm;                                           // [ns][DH]
    float* V = K + ns * DH;                                  // [ns][DH]
    float* sc = V + ns * DH;                                 // [64][LS]
    for (int i = threadIdx.x; i < ns * DH; i += 64) {
        const int m = i / DH, d = i % DH;
        const float* r = qkv + (s0 + m) * (int64_t)(3 * D) + d * kHeads + h;
        K[i] = r[D];
        V[i] = r[2 * D];
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= nt) return;
    float q[DH];
    {
        const float* r = qkv + (t0 + t) * (int64_t)(3 * D) + h;
#pragma unroll
        for (int d = 0; d < DH; d++) q[d] = r[d * kHeads];
    }
    const float scale = 1.0f / sqrtf((float)DH);
    float* s = sc + t * LS;
    float mx = -INFINITY;
    for (int m = 0; m < ns; m++) {
        const float* k = K + m * DH;                         // (every lane reads the same address: a broadcast)
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d++) a = fmaf(q[d], k[d], a);
        a *= scale;
        s[m] = a;
        mx = fmaxf(mx, a);
    }
    float den = 0.f;
    for (int m = 0; m < ns; m++) {
        const float e = expf(s[m] - mx);
        s[m] = e;
        den += e;
    }
    float acc[DH];
#pragma unroll
    for (int d = 0; d < DH; d++) acc[d] = 0.f;
    for (int m = 0; m < ns; m++) {
        const float p = s[m] / den;
        const float* v = V + m * DH;
#pragma unroll
        for (int d = 0; d < DH; d++) acc[d] = fmaf(p, v[d], acc[d]);
    }
    float* o = msg + (t0 + t) * (int64_t)D + h;
#pragma unroll
    for (int d = 0; d < DH; d++) o[d * kHeads] = acc[d];
}

// One wavefront per sample.  md [B (M + N)][D]: final_proj of the set-major token rows.
__global__ __launch_bounds__(64) void k_head_sets(const float* __restrict__ md, int64_t B, int M, int N, int D, float alpha_f,
                                                  int iters, float thresh, float* __restrict__ P, int64_t* __restrict__ matches0,
                                                  int64_t* __restrict__ matches1, float* __restrict__ ms0, float* __restrict__ ms1) {
    extern __shared__ double smd[];
    const int lane = threadIdx.x;
    const int M1 = M + 1, N1 = N + 1;
    double* Z = smd;                 // [M1][N1]
    double* u = Z + M1 * N1;         // [M1]
    double* v = u + M1;              // [N1]
    double* rmax = v + N1;           // [M] row maxima of the inner block, [N] column maxima
    int* ridx = (int*)(rmax + M + N);   // [M] + [N]
    const int64_t b = blockIdx.x;
    const float* m0 = md + set_row(0, b, B, M, N) * D;
    const float* m1 = md + set_row(1, b, B, M, N) * D;
    const double alpha = (double)alpha_f;
    const double inv = 1.0 / sqrt((double)D);
    for (int e = lane; e < M1 * N1; e += 64) {
        const int i = e / N1, j = e % N1;
        double a = alpha;
        if (i < M && j < N) {
            a = 0.0;
            const float* x = m0 + i * (int64_t)D;
            const float* y = m1 + j * (int64_t)D;
            for (int k = 0; k < D; k++) a = fma((double)x[k], (double)y[k], a);
            a *= inv;
        }
        Z[e] = a;
    }
    const double norm = -log((double)(M + N));
    const double lmu_bin = log((double)N) + norm, lnu_bin = log((double)M) + norm;
    if (lane < M1) u[lane] = 0.0;
    if (lane < N1) v[lane] = 0.0;
    __syncthreads();
    for (int it = 0; it < iters; it++) {
        if (lane < M1) {  // u = log_mu - logsumexp_j(Z + v)
            double mx = -INFINITY;
            for (int j = 0; j < N1; j++) mx = fmax(mx, Z[lane * N1 + j] + v[j]);
            double s = 0.0;
            for (int j = 0; j < N1; j++) s += exp(Z[lane * N1 + j] + v[j] - mx);
            u[lane] = (lane < M ? norm : lmu_bin) - (mx + log(s));
        }
        __syncthreads();
        if (lane < N1) {  // v = log_nu - logsumexp_i(Z + u)
            double mx = -INFINITY;
            for (int i = 0; i < M1; i++) mx = fmax(mx, Z[i * N1 + lane] + u[i]);
            double s = 0.0;
            for (int i = 0; i < M1; i++) s += exp(Z[i * N1 + lane] + u[i] - mx);
            v[lane] = (lane < N ? norm : lnu_bin) - (mx + log(s));
        }
        __syncthreads();
    }
    for (int e = lane; e < M1 * N1; e += 64) {
        const int i = e / N1, j = e % N1;
        const double z = Z[e] + u[i] + v[j] - norm;
        Z[e] = z;
        P[b * M1 * N1 + e] = (float)exp(z);
    }
    __syncthreads();
    // maxima over the inner (non-dustbin) block; ties -> first index
    if (lane < M) {
        double mx = -INFINITY;
        int bi = 0;
        for (int j = 0; j < N; j++)
            if (Z[lane * N1 + j] > mx) { mx = Z[lane * N1 + j]; bi = j; }
        rmax[lane] = mx;
        ridx[lane] = bi;
    }
    if (lane < N) {
        double mx = -INFINITY;
        int bi = 0;
        for (int i = 0; i < M; i++)
            if (Z[i * N1 + lane] > mx) { mx = Z[i * N1 + lane]; bi = i; }
        rmax[M + lane] = mx;
        ridx[M + lane] = bi;
    }
    __syncthreads();
    if (lane < M) {
        const int j = ridx[lane];
        const bool mutual = ridx[M + j] == lane;
        const float s = mutual ? (float)exp(rmax[lane]) : 0.f;
        ms0[b * M + lane] = s;
        matches0[b * M + lane] = (mutual && s > thresh) ? j : -1;
    }
    if (lane < N) {
        const int i = ridx[M + lane];
        const bool mutual1 = ridx[i] == lane;
        const bool mutual0 = ridx[M + ridx[i]] == i;                       // mutual0[i]
        const float s0 = mutual0 ? (float)exp(rmax[i]) : 0.f;             // mscores0[i]
        ms1[b * N + lane] = mutual1 ? s0 : 0.f;
        matches1[b * N + lane] = (mutual1 && mutual0 && s0 > thresh) ? i : -1;
    }
}

constexpr int kLossThreads = 256;

// Sum of one value per thread of the workgroup, the same tree every time: butterflies inside a wavefront, then the wavefronts'
// sums in order.  Every thread of the workgroup must call it; all of them receive the sum.
__device__ __forceinline__ double block_sum(double x, double* part /*[kLossThreads / 64]*/) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    __syncthreads();                                         // (part may still be read from the previous call)
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = x;
    __syncthreads();
    double s = 0.0;
#pragma unroll
    for (int w = 0; w < kLossThreads / 64; w++) s += part[w];
    return s;
}

// One workgroup.  Wavefront w takes samples w, w + 4, ...; its lanes stride over the sample's entries.
__global__ __launch_bounds__(kLossThreads) void k_matching_loss(const float* __restrict__ P, int64_t B, int M1, int N1,
                                                                const int32_t* __restrict__ idx, const int32_t* __restrict__ entry_ptr,
                                                                int64_t n_entries, float* __restrict__ sample_loss,
                                                                float* __restrict__ loss) {
    __shared__ double part[kLossThreads / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float nan = __builtin_nanf("");
    for (int64_t b = wave; b < B; b += kLossThreads / 64) {
        const int64_t lo = entry_ptr[b], hi = entry_ptr[b + 1];
        bool ok = lo >= 0 && hi <= n_entries && lo < hi;     // (an empty sample has no mean)
        double s = 0.0;
        if (ok)
            for (int64_t e = lo + lane; e < hi; e += 64) {
                const int i = idx[2 * e], j = idx[2 * e + 1];
                if (i < 0 || i >= M1 || j < 0 || j >= N1)
                    ok = false;                              // nothing is read through the entry
                else
                    s -= log((double)P[(b * M1 + i) * (int64_t)N1 + j]);
            }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        const bool all_ok = __all(ok);
        if (lane == 0) sample_loss[b] = all_ok ? (float)(s / (double)(hi - lo)) : nan;
    }
    __syncthreads();                                         // the workgroup's own global writes are visible to it behind the barrier
    double t = 0.0;
    for (int64_t b = threadIdx.x; b < B; b += kLossThreads) t += (double)sample_loss[b];
    t = block_sum(t, part);
    if (threadIdx.x == 0) loss[0] = (float)(t / (double)B);
}

// One workgroup: mean((a - b)^2).
__global__ __launch_bounds__(kLossThreads) void k_mse_loss(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                           float* __restrict__ loss) {
    __shared__ double part[kLossThreads / 64];
    double t = 0.0;
    for (int64_t i = threadIdx.x; i < n; i += kLossThreads) {
        const double d = (double)a[i] - (double)b[i];
        t = fma(d, d, t);
    }
    t = block_sum(t, part);
    if (threadIdx.x == 0) loss[0] = (float)(t / (double)n);
}

int check_sizes(const char* what, int64_t batch, int M, int N, int D) {
    T2P_CHECK_ARG(batch >= 0 && M >= 1 && N >= 1 && M <= kMaxTokens && N <= kMaxTokens,
                  "%s: need 1 <= n_obj, n_hints <= 63 (got %d, %d)", what, M, N);
    if (D != 64 && D != 128 && D != 256) {
        set_error("%s: embed_dim=%d not built (64, 128, 256)", what, D);
        return T2P_E_UNSUPPORTED;
    }
    T2P_CHECK_ARG(batch * 2 * kHeads <= 0x7fffffff, "%s: batch %lld too large for one launch", what, (long long)batch);
    return 0;
}

}  // namespace
}  // namespace t2p

using namespace t2p;

extern "C" {

int t2p_match_attention(const float* qkv, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim, int32_t cross,
                        float* msg, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int M = n_obj, N = n_hints, D = embed_dim;
    T2P_CHECK_ARG(qkv && msg, "match_attention: NULL argument");
    T2P_CHECK_ARG(cross == 0 || cross == 1, "match_attention: cross must be 0 (self) or 1 (got %d)", cross);
    T2P_TRY(check_sizes("match_attention", batch, M, N, D));
    if (batch == 0) return 0;
    const int S = M > N ? M : N, DH = D / kHeads;
    const size_t lds = ((size_t)2 * S * DH + (size_t)64 * (S | 1)) * sizeof(float);   // <= 48.3 KiB at S = 63, DH = 64
    auto attn = D == 64 ? k_attn_sets<16> : (D == 128 ? k_attn_sets<32> : k_attn_sets<64>);
    ProfScope ps_("match_train_attn", st);
    hipLaunchKernelGGL(attn, dim3((unsigned)(batch * 2 * kHeads)), dim3(64), lds, st, qkv, batch, M, N, cross, msg);
    T2P_CHECK_LAUNCH("match_train_attn");
    return 0;
}

int t2p_match_head(const float* mdesc, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim, float bin_score,
                   int32_t sinkhorn_iters, float match_threshold, float* P, int64_t* matches0, int64_t* matches1, float* mscores0,
                   float* mscores1, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int M = n_obj, N = n_hints, D = embed_dim;
    T2P_CHECK_ARG(mdesc && P && matches0 && matches1 && mscores0 && mscores1, "match_head: NULL argument");
    T2P_TRY(check_sizes("match_head", batch, M, N, D));
    T2P_CHECK_ARG(sinkhorn_iters >= 0, "match_head: sinkhorn_iters < 0");
    if (batch == 0) return 0;
    // Z, u, v, the maxima (doubles) and their indices: <= 35.3 KiB at 63 + 63 tokens
    const size_t lds = ((size_t)(M + 1) * (N + 1) + (M + 1) + (N + 1) + (M + N)) * sizeof(double) + (size_t)(M + N) * sizeof(int);
    ProfScope ps_("match_train_head", st);
    hipLaunchKernelGGL(k_head_sets, dim3((unsigned)batch), dim3(64), lds, st, mdesc, batch, M, N, D, bin_score, sinkhorn_iters,
                       match_threshold, P, matches0, matches1, mscores0, mscores1);
    T2P_CHECK_LAUNCH("match_train_head");
    return 0;
}

int t2p_matching_loss(const float* P, int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* idx, const int32_t* entry_ptr,
                      int64_t n_entries, float* sample_loss, float* loss, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(P && idx && entry_ptr && sample_loss && loss, "matching_loss: NULL argument");
    T2P_CHECK_ARG(batch >= 1 && n_obj >= 1 && n_hints >= 1, "matching_loss: need batch, n_obj, n_hints >= 1 (got %lld, %d, %d)",
                  (long long)batch, n_obj, n_hints);
    T2P_CHECK_ARG(n_entries >= 1 && n_entries <= 0x3fffffff, "matching_loss: need 1 <= n_entries < 2^30 (got %lld)", (long long)n_entries);
    ProfScope ps_("matching_loss", st);
    hipLaunchKernelGGL(k_matching_loss, dim3(1), dim3(kLossThreads), 0, st, P, batch, n_obj + 1, n_hints + 1, idx, entry_ptr, n_entries,
                       sample_loss, loss);
    T2P_CHECK_LAUNCH("matching_loss");
    return 0;
}

int t2p_mse_loss(const float* a, const float* b, int64_t n, float* loss, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(a && b && loss, "mse_loss: NULL argument");
    T2P_CHECK_ARG(n >= 1, "mse_loss: no elements");
    ProfScope ps_("mse_loss", st);
    hipLaunchKernelGGL(k_mse_loss, dim3(1), dim3(kLossThreads), 0, st, a, b, n, loss);
    T2P_CHECK_LAUNCH("mse_loss");
    return 0;
}

}  // extern "C"
