// The fine matcher's shared statements: what match.hip (inference, sample-major rows, BatchNorm folded) and match_train.hip
// (train() mode, set-major rows, forward and backward) both compute is written here once, so that the paths cannot drift apart.
//   * the optimal-transport head: score matrix, log-Sinkhorn iterations, log couplings, mutual nearest neighbours - float64
//     throughout, P rounded to fp32 once (|u| and |v| reach 5 to 8, where a fp32 recurrence left the dustbin couplings 2.5e-6 from
//     the float64 matcher: docs/notebook.md, "The fine matcher's forward kernels against float64").  One wavefront per sample,
//     lane i owns row i of u and lane j column j of v, the matrix sits in LDS;
//   * one softmax row of the training path's multi-head attention and its weighted sum of the values, fp32, fixed fma chains;
//   * the size limits and their refusals.
// The library is built with -ffp-contract=off and every fused operation is an explicit fma / fmaf: inlining these functions into a
// kernel changes no bit of its results.
#pragma once
#include "t2p_common.h"

namespace t2p {

constexpr int kHeads = 4;
constexpr int kMaxTokens = 63;   // per set: a wavefront's lanes cover a set plus its dustbin

// Set-major token rows (match_train.hip): first row of sample b's tokens of that set
__device__ __forceinline__ int64_t set_row(int set, int64_t b, int64_t B, int M, int N) {
    return set == 0 ? b * M : B * M + b * N;
}

// per_head_grid: the launch runs 2 * kHeads workgroups per sample (the attention of match_train.hip and every entry point that
// shares its limits); t2p_match launches one workgroup per sample and passes false.
inline int check_sizes(const char* what, int64_t batch, int M, int N, int D, bool per_head_grid = true) {
    T2P_CHECK_ARG(batch >= 0 && M >= 1 && N >= 1 && M <= kMaxTokens && N <= kMaxTokens,
                  "%s: need 1 <= n_obj, n_hints <= 63 (got %d, %d)", what, M, N);
    if (D != 64 && D != 128 && D != 256) {
        set_error("%s: embed_dim=%d not built (64, 128, 256)", what, D);
        return T2P_E_UNSUPPORTED;
    }
    if (per_head_grid)
        T2P_CHECK_ARG(batch * 2 * kHeads <= 0x7fffffff, "%s: batch %lld too large for one launch", what, (long long)batch);
    return 0;
}

// ---- the transport head ----------------------------------------------------------------------------------------------------------------

// The head's dynamic LDS: Z [M + 1][N + 1], u [M + 1], v [N + 1] (float64), and for the kernels that decide matches the maxima of
// the inner block, rmax [M] rows + [N] columns (float64), with their indices ridx (int).  `end` is where a kernel's own arrays follow.
// 35.3 KiB with the maxima at 63 + 63 tokens.
__host__ __device__ inline size_t head_lds_bytes(int M, int N, bool maxima) {
    return ((size_t)(M + 1) * (N + 1) + (M + 1) + (N + 1)) * sizeof(double) +
           (maxima ? (size_t)(M + N) * (sizeof(double) + sizeof(int)) : 0);
}
struct HeadLds {
    double *Z, *u, *v, *rmax;
    int* ridx;
    void* end;
    __device__ HeadLds(double* base, int M, int N, bool maxima)
        : Z(base), u(Z + (M + 1) * (N + 1)), v(u + M + 1), rmax(v + N + 1), ridx((int*)(rmax + (maxima ? M + N : 0))),
          end(ridx + (maxima ? M + N : 0)) {}
};

// Log marginals: every token carries `norm`, each dustbin the mass of the other set
struct LogMarginals {
    double norm, mu_bin, nu_bin;
    __device__ LogMarginals(int M, int N)
        : norm(-log((double)(M + N))), mu_bin(log((double)N) + norm), nu_bin(log((double)M) + norm) {}
};

// Z = m0 m1^T / sqrt(D) from the rows m0 [M][D], m1 [N][D] (float64 fma chain over k, scaled once), alpha in the dustbin row and column
__device__ __forceinline__ void transport_scores(const float* __restrict__ m0, const float* __restrict__ m1, int M, int N, int D,
                                                 double alpha, double* Z) {
    const int lane = threadIdx.x;
    const int M1 = M + 1, N1 = N + 1;
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
}

// u = v = 0, then `iters` times u = log_mu - logsumexp_j(Z + v), v = log_nu - logsumexp_i(Z + u); a barrier behind each half, and
// one in front of the first (Z is complete behind it).  keep(t, lane, is_v, value) sees every new u_t[lane] / v_t[lane] in the lane
// that writes it.  Returns the log marginals it iterated with: what follows needs their norm.
template <typename Keep>
__device__ __forceinline__ LogMarginals sinkhorn_iterate(const double* Z, double* u, double* v, int M, int N, int iters, Keep keep) {
    const int lane = threadIdx.x;
    const int M1 = M + 1, N1 = N + 1;
    const LogMarginals lm(M, N);
    if (lane < M1) u[lane] = 0.0;
    if (lane < N1) v[lane] = 0.0;
    __syncthreads();
    for (int t = 0; t < iters; t++) {
        if (lane < M1) {
            double mx = -INFINITY;
            for (int j = 0; j < N1; j++) mx = fmax(mx, Z[lane * N1 + j] + v[j]);
            double s = 0.0;
            for (int j = 0; j < N1; j++) s += exp(Z[lane * N1 + j] + v[j] - mx);
            const double x = (lane < M ? lm.norm : lm.mu_bin) - (mx + log(s));
            u[lane] = x;
            keep(t, lane, false, x);
        }
        __syncthreads();
        if (lane < N1) {
            double mx = -INFINITY;
            for (int i = 0; i < M1; i++) mx = fmax(mx, Z[i * N1 + lane] + u[i]);
            double s = 0.0;
            for (int i = 0; i < M1; i++) s += exp(Z[i * N1 + lane] + u[i] - mx);
            const double x = (lane < N ? lm.norm : lm.nu_bin) - (mx + log(s));
            v[lane] = x;
            keep(t, lane, true, x);
        }
        __syncthreads();
    }
    return lm;
}

// Behind the iterations: Z becomes the log couplings Z + u + v - norm, P their exponentials rounded to fp32 once; the maxima of the
// inner (non-dustbin) block, ties to the first index; a match is a mutual maximum whose score exp(max) exceeds thresh.  The output
// pointers are the sample's own: P [M + 1][N + 1], matches0 / ms0 [M], matches1 / ms1 [N].
__device__ __forceinline__ void transport_decide(const HeadLds& s, int M, int N, double norm, float thresh, float* __restrict__ P,
                                                 int64_t* __restrict__ matches0, int64_t* __restrict__ matches1,
                                                 float* __restrict__ ms0, float* __restrict__ ms1) {
    const int lane = threadIdx.x;
    const int M1 = M + 1, N1 = N + 1;
    double* Z = s.Z;
    double* rmax = s.rmax;
    int* ridx = s.ridx;
    for (int e = lane; e < M1 * N1; e += 64) {
        const int i = e / N1, j = e % N1;
        const double z = Z[e] + s.u[i] + s.v[j] - norm;
        Z[e] = z;
        P[e] = (float)exp(z);
    }
    __syncthreads();
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
        const float sc = mutual ? (float)exp(rmax[lane]) : 0.f;
        ms0[lane] = sc;
        matches0[lane] = (mutual && sc > thresh) ? j : -1;
    }
    if (lane < N) {
        const int i = ridx[M + lane];
        const bool mutual1 = ridx[i] == lane;
        const bool mutual0 = ridx[M + ridx[i]] == i;                       // mutual0[i]
        const float s0 = mutual0 ? (float)exp(rmax[i]) : 0.f;             // mscores0[i]
        ms1[lane] = mutual1 ? s0 : 0.f;
        matches1[lane] = (mutual1 && mutual0 && s0 > thresh) ? i : -1;
    }
}

// ---- one attention row -----------------------------------------------------------------------------------------------------------------

// s[m] = exp(scale q . k_m - max) over the ns source tokens and den, their sum in index order, for a q held in registers.  Key row m
// is K + m * k_pitch: a head's compact [ns][DH] slice (k_attn_sets and phase 1 of k_attn_sets_bwd; k_attn of match.hip has the
// same statements on its strided LDS rows).
template <int DH>
__device__ __forceinline__ void attention_row(const float (&q)[DH], const float* K, int k_pitch, int ns, float scale, float* s,
                                              float& den) {
    float mx = -INFINITY;
    for (int m = 0; m < ns; m++) {
        const float* k = K + m * k_pitch;
        float a = 0.f;
#pragma unroll
        for (int d = 0; d < DH; d++) a = fmaf(q[d], k[d], a);
        a *= scale;
        s[m] = a;
        mx = fmaxf(mx, a);
    }
    den = 0.f;
    for (int m = 0; m < ns; m++) {
        const float e = expf(s[m] - mx);
        s[m] = e;
        den += e;
    }
}

// acc = sum_m (s[m] / den) v_m, value rows addressed like the key rows of attention_row
template <int DH>
__device__ __forceinline__ void attention_values(const float* s, float den, const float* V, int v_pitch, int ns, float (&acc)[DH]) {
#pragma unroll
    for (int d = 0; d < DH; d++) acc[d] = 0.f;
    for (int m = 0; m < ns; m++) {
        const float p = s[m] / den;
        const float* v = V + m * v_pitch;
#pragma unroll
        for (int d = 0; d < DH; d++) acc[d] = fmaf(p, v[d], acc[d]);
    }
}

}  // namespace t2p
