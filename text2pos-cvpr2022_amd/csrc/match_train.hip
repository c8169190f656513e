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
// sample-major rows [B (M + N)] and fold BatchNorm; the kernels here address the two sets.  What the two files compute alike - the
// attention's softmax row, the transport head - is one statement in match_common.h; the kernels here and there differ in where
// their rows lie, in what they keep (the backward's iterates) and in what follows.
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
//
// Backward (t2p_*_backward, the lower half of this file): every kernel recomputes what it needs from its forward's INPUTS - the
// forward entry points and their outputs stay as they are - and writes every element of its gradient exactly once: no zero fill, no
// atomics, the same bits from call to call.  The upstream gradient of a loss is read on the device.
//   * attention backward: the forward's workgroups (sample, target set, head).  Phase 1, one work item per target token: P and dS
//     rows into LDS, dq out.  Phase 2, one work item per source token: the head's k | v slices in LDS give way to the target
//     side's q | dO slices, dk and dv are sums over the target tokens.  2 x 63 x 64 + 2 x 64 x 63 floats = 63 KiB: inside the
//     default 64 KiB.
//   * head backward: one wavefront per sample, float64.  It re-runs the forward's iterations and keeps every iterate u_t, v_t in the
//     caller's workspace (T (M + N + 2) doubles per sample; a lane reads back only what it wrote itself), then walks the unrolled
//     iterations backwards with Z0 and its gradient both in LDS (2 x 32 KiB + vectors at 63 + 63 tokens: the kernel's dynamic-LDS
//     limit is raised, gfx950 has 160 KiB per CU).
#include "match_common.h"

#include "../../include/t2p.h"

namespace t2p {
namespace {

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
    float* s = sc + t * LS;
    float den;
    attention_row<DH>(q, K, DH, ns, 1.0f / sqrtf((float)DH), s, den);   // (every lane reads the same key address: a broadcast)
    float acc[DH];
    attention_values<DH>(s, den, V, DH, ns, acc);
    float* o = msg + (t0 + t) * (int64_t)D + h;
#pragma unroll
    for (int d = 0; d < DH; d++) o[d * kHeads] = acc[d];
}

// One wavefront per sample.  md [B (M + N)][D]: final_proj of the set-major token rows.
__global__ __launch_bounds__(64) void k_head_sets(const float* __restrict__ md, int64_t B, int M, int N, int D, float alpha_f,
                                                  int iters, float thresh, float* __restrict__ P, int64_t* __restrict__ matches0,
                                                  int64_t* __restrict__ matches1, float* __restrict__ ms0, float* __restrict__ ms1) {
    extern __shared__ double smd[];
    const HeadLds s(smd, M, N, true);
    const int64_t b = blockIdx.x;
    transport_scores(md + set_row(0, b, B, M, N) * D, md + set_row(1, b, B, M, N) * D, M, N, D, (double)alpha_f, s.Z);
    const LogMarginals lm = sinkhorn_iterate(s.Z, s.u, s.v, M, N, iters, [](int, int, bool, double) {});
    transport_decide(s, M, N, lm.norm, thresh, P + b * (M + 1) * (N + 1), matches0 + b * M, matches1 + b * N, ms0 + b * M, ms1 + b * N);
}

constexpr int kLossThreads = 256;

// Sum of one value per thread of the workgroup, the same tree every time: butterflies inside a wavefront, then the wavefronts'
// sums in order.  Every thread of the workgroup must call it; all of them receive the sum.
__device__ __forceinline__ double block_sum(double x, double* part /*[kLossThreads / 64]*/) {
    x = wave_sum(x);
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
        s = wave_sum(s);
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

// ---- backward ------------------------------------------------------------------------------------------------------------------------

// grid = B * 2 * heads, 64 threads: the forward's decomposition.  dq -> the q columns of the target rows, dk / dv -> the k / v
// columns of the source rows; over the two target sets every element of dqkv [B (M + N)][3D] of head h is written once, for
// cross = 0 (source set = target set) as for cross = 1 (the other one).
template <int DH>
__global__ __launch_bounds__(64) void k_attn_sets_bwd(const float* __restrict__ qkv, const float* __restrict__ dmsg, int64_t B, int M,
                                                      int N, int cross, float* __restrict__ dqkv) {
    constexpr int D = DH * kHeads;
    extern __shared__ float sm[];
    const int h = blockIdx.x % kHeads;
    const int tset = (blockIdx.x / kHeads) % 2;
    const int64_t b = blockIdx.x / (2 * kHeads);
    const int sset = cross ? 1 - tset : tset;
    const int nt = tset == 0 ? M : N, ns = sset == 0 ? M : N;
    const int64_t t0 = set_row(tset, b, B, M, N), s0 = set_row(sset, b, B, M, N);
    const int S = M > N ? M : N;
    const int LS = ns | 1;
    float* KQ = sm;                                          // [S][DH]: the source's k, then the targets' q
    float* VO = KQ + S * DH;                                 // [S][DH]: the source's v, then the targets' dO
    float* Pm = VO + S * DH;                                 // [64][LS] softmax rows
    float* dS = Pm + 64 * LS;                                // [64][LS] dP, then dS
    for (int i = threadIdx.x; i < ns * DH; i += 64) {
        const int m = i / DH, d = i % DH;
        const float* r = qkv + (s0 + m) * (int64_t)(3 * D) + d * kHeads + h;
        KQ[i] = r[D];
        VO[i] = r[2 * D];
    }
    __syncthreads();
    const int t = threadIdx.x;
    const float scale = 1.0f / sqrtf((float)DH);
    if (t < nt) {
        float* p = Pm + t * LS;
        float* ds = dS + t * LS;
        float den;
        {   // p = exp(S - max) and den, S = scale q k^T: the forward's row
            float q[DH];
            const float* r = qkv + (t0 + t) * (int64_t)(3 * D) + h;
#pragma unroll
            for (int d = 0; d < DH; d++) q[d] = r[d * kHeads];
            attention_row<DH>(q, KQ, DH, ns, scale, p, den);
        }
        float delta = 0.f;                                   // rowsum(P o dP)
        {
            float go[DH];
            const float* r = dmsg + (t0 + t) * (int64_t)D + h;
#pragma unroll
            for (int d = 0; d < DH; d++) go[d] = r[d * kHeads];
            for (int m = 0; m < ns; m++) {
                const float* v = VO + m * DH;
                float a = 0.f;
#pragma unroll
                for (int d = 0; d < DH; d++) a = fmaf(go[d], v[d], a);
                const float pm = p[m] / den;
                p[m] = pm;
                ds[m] = a;                                   // dP = dO V^T
                delta = fmaf(pm, a, delta);
            }
        }
        float acc[DH];
#pragma unroll
        for (int d = 0; d < DH; d++) acc[d] = 0.f;
        for (int m = 0; m < ns; m++) {
            const float g = p[m] * (ds[m] - delta);          // dS = P o (dP - rowsum(P o dP))
            ds[m] = g;
            const float* k = KQ + m * DH;
#pragma unroll
            for (int d = 0; d < DH; d++) acc[d] = fmaf(g, k[d], acc[d]);
        }
        float* o = dqkv + (t0 + t) * (int64_t)(3 * D) + h;
#pragma unroll
        for (int d = 0; d < DH; d++) o[d * kHeads] = scale * acc[d];
    }
    __syncthreads();                                         // k | v are done with: the targets' q | dO take their place
    for (int i = threadIdx.x; i < nt * DH; i += 64) {
        const int tt = i / DH, d = i % DH;
        KQ[i] = qkv[(t0 + tt) * (int64_t)(3 * D) + d * kHeads + h];
        VO[i] = dmsg[(t0 + tt) * (int64_t)D + d * kHeads + h];
    }
    __syncthreads();
    const int m = threadIdx.x;
    if (m < ns) {
        float ak[DH], av[DH];
#pragma unroll
        for (int d = 0; d < DH; d++) ak[d] = av[d] = 0.f;
        for (int tt = 0; tt < nt; tt++) {
            const float pm = Pm[tt * LS + m], g = dS[tt * LS + m];
            const float* q = KQ + tt * DH;
            const float* go = VO + tt * DH;
#pragma unroll
            for (int d = 0; d < DH; d++) {
                av[d] = fmaf(pm, go[d], av[d]);              // dV[m] = sum_t P[t, m] dO[t]
                ak[d] = fmaf(g, q[d], ak[d]);                // dk[m] = scale sum_t dS[t, m] q[t]
            }
        }
        float* o = dqkv + (s0 + m) * (int64_t)(3 * D) + h;
#pragma unroll
        for (int d = 0; d < DH; d++) {
            o[D + d * kHeads] = scale * ak[d];
            o[2 * D + d * kHeads] = av[d];
        }
    }
}

// One wavefront per sample.  ws: per sample iters (M + N + 2) doubles, the iterates u_t | v_t of t = 1 .. iters.  Lane j owns
// column j of the gradient of Z0 throughout; a lane reads back from ws only what it stored itself.
__global__ __launch_bounds__(64) void k_head_sets_bwd(const float* __restrict__ md, const float* __restrict__ dP, int64_t B, int M, int N,
                                                      int D, float alpha_f, int iters, float* __restrict__ dmd,
                                                      double* __restrict__ dbin, double* ws) {
    extern __shared__ double smd[];
    const int lane = threadIdx.x;
    const int M1 = M + 1, N1 = N + 1;
    const HeadLds s(smd, M, N, false);
    double *Z = s.Z, *u = s.u, *v = s.v;   // Z0, u_t, v_t
    double* gZ = (double*)s.end;     // [M1][N1] the gradient of Z0
    double* vp = gZ + M1 * N1;       // [N1] v_{t-1}
    double* gu = vp + N1;            // [M1]
    double* gv = gu + M1;            // [N1]
    const int64_t b = blockIdx.x;
    const float* m0 = md + set_row(0, b, B, M, N) * D;
    const float* m1 = md + set_row(1, b, B, M, N) * D;
    double* it = ws + b * (int64_t)iters * (M1 + N1);
    const double inv = 1.0 / sqrt((double)D);
    // ---- the forward, every iterate kept
    transport_scores(m0, m1, M, N, D, (double)alpha_f, Z);
    const LogMarginals lm = sinkhorn_iterate(Z, u, v, M, N, iters, [=](int t, int i, bool is_v, double x) { it[t * (M1 + N1) + (is_v ? M1 : 0) + i] = x; });
    // ---- G = dP exp(Z) from the float64 log couplings; gZ0 = G, gu = rowsum(G), gv = colsum(G)
    {
        double cs = 0.0;
        for (int i = 0; i < M1; i++) {
            double g = 0.0;
            if (lane < N1) {
                const double z = Z[i * N1 + lane] + u[i] + v[lane] - lm.norm;
                g = (double)dP[(b * M1 + i) * (int64_t)N1 + lane] * exp(z);
                gZ[i * N1 + lane] = g;
                cs += g;
            }
            const double rs = wave_sum(g);
            if (lane == 0) gu[i] = rs;
        }
        if (lane < N1) gv[lane] = cs;
    }
    __syncthreads();
    // ---- the unrolled iterations, backwards
    for (int t = iters - 1; t >= 0; t--) {
        if (lane < M1) u[lane] = it[t * (M1 + N1) + lane];
        if (lane < N1) {
            v[lane] = it[t * (M1 + N1) + M1 + lane];
            vp[lane] = t > 0 ? it[(t - 1) * (M1 + N1) + M1 + lane] : 0.0;
        }
        __syncthreads();
        {   // v_t = log_nu - logsumexp_i(Z0 + u_t): W[i, j] = exp(Z0 + u_t[i] + v_t[j] - log_nu[j]), columns sum to 1
            const double lnu = lane < N ? lm.norm : lm.nu_bin;
            const double gvj = lane < N1 ? gv[lane] : 0.0;
            for (int i = 0; i < M1; i++) {
                double term = 0.0;
                if (lane < N1) {
                    term = exp(Z[i * N1 + lane] + u[i] + v[lane] - lnu) * gvj;
                    gZ[i * N1 + lane] -= term;               // gZ0 -= W diag(gv)
                }
                const double rs = wave_sum(term);
                if (lane == 0) gu[i] -= rs;                  // gu -= W gv
            }
        }
        __syncthreads();
        if (lane < N1) {  // u_t = log_mu - logsumexp_j(Z0 + v_{t-1}): R[i, j] = exp(Z0 + v_{t-1}[j] + u_t[i] - log_mu[i]), rows sum to 1
            double acc = 0.0;
            for (int i = 0; i < M1; i++) {
                const double r = exp(Z[i * N1 + lane] + vp[lane] + u[i] - (i < M ? lm.norm : lm.mu_bin));
                const double term = gu[i] * r;
                gZ[i * N1 + lane] -= term;                   // gZ0 -= diag(gu) R
                acc -= term;                                 // gv = -R^T gu
            }
            gv[lane] = acc;
        }
        __syncthreads();
        if (lane < M1) gu[lane] = 0.0;
        __syncthreads();
    }
    // ---- d_bin = the dustbin row and column of gZ0; d_m0 = gS m1, d_m1 = gS^T m0 with gS = gZ0[:M, :N] / sqrt(D)
    if (lane == 0) {
        double s = 0.0;
        for (int i = 0; i < M1; i++) s += gZ[i * N1 + N];
        for (int j = 0; j < N; j++) s += gZ[M * N1 + j];
        dbin[b] = s;
    }
    float* d0 = dmd + set_row(0, b, B, M, N) * D;
    float* d1 = dmd + set_row(1, b, B, M, N) * D;
    for (int e = lane; e < M * D; e += 64) {
        const int i = e / D, k = e % D;
        double a = 0.0;
        for (int j = 0; j < N; j++) a = fma(gZ[i * N1 + j], (double)m1[j * (int64_t)D + k], a);
        d0[e] = (float)(a * inv);
    }
    for (int e = lane; e < N * D; e += 64) {
        const int j = e / D, k = e % D;
        double a = 0.0;
        for (int i = 0; i < M; i++) a = fma(gZ[i * N1 + j], (double)m0[i * (int64_t)D + k], a);
        d1[e] = (float)(a * inv);
    }
}

// One workgroup per sample; a thread owns elements of dP[b] and counts how often the sample lists each of them: a pair listed
// twice counts twice without atomics, every other element is 0.  dP = -g / (B M_b P), in float64, rounded once.
__global__ __launch_bounds__(kLossThreads) void k_matching_loss_bwd(const float* __restrict__ P, int64_t B, int M1, int N1,
                                                                    const int32_t* __restrict__ idx, const int32_t* __restrict__ entry_ptr,
                                                                    int64_t n_entries, const float* __restrict__ gp, float* __restrict__ dP) {
    const int64_t b = blockIdx.x;
    int64_t lo = entry_ptr[b], hi = entry_ptr[b + 1];
    if (lo < 0 || hi > n_entries || lo >= hi) lo = hi = 0;   // (the forward has marked such a sample with NaN)
    const double g = (double)gp[0];
    const double denom = (double)B * (double)(hi - lo);
    for (int e = threadIdx.x; e < M1 * N1; e += kLossThreads) {
        const int i = e / N1, j = e % N1;
        int c = 0;
        for (int64_t k = lo; k < hi; k++) c += (idx[2 * k] == i && idx[2 * k + 1] == j) ? 1 : 0;
        const int64_t at = b * M1 * (int64_t)N1 + e;
        dP[at] = c ? (float)(-(g * (double)c) / (denom * (double)P[at])) : 0.f;
    }
}

// da = 2 g (a - b) / n in float64, rounded once.
__global__ __launch_bounds__(kLossThreads) void k_mse_loss_bwd(const float* __restrict__ a, const float* __restrict__ b, int64_t n,
                                                               const float* __restrict__ gp, float* __restrict__ da) {
    const double f = 2.0 * (double)gp[0] / (double)n;
    for (int64_t i = blockIdx.x * (int64_t)kLossThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kLossThreads)
        da[i] = (float)(f * ((double)a[i] - (double)b[i]));
}

// Column sums of x [rows][cols]: a workgroup per 64 columns, lane = column, wavefront w adds rows w, w + 4, ... in float64; the four
// partial sums are added in order and rounded to fp32 once.
__global__ __launch_bounds__(kLossThreads) void k_colsum(const float* __restrict__ x, int64_t rows, int cols, float* __restrict__ out) {
    __shared__ double part[kLossThreads / 64][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int c = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (c < cols)
        for (int64_t r = wave; r < rows; r += kLossThreads / 64) s += (double)x[r * cols + c];
    part[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && c < cols) {
        double t = 0.0;
#pragma unroll
        for (int w = 0; w < kLossThreads / 64; w++) t += part[w][lane];
        out[c] = (float)t;
    }
}

size_t head_bwd_ws_bytes(int64_t batch, int M, int N, int iters) {
    return (size_t)batch * (size_t)iters * (size_t)(M + N + 2) * sizeof(double);
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
    const size_t lds = head_lds_bytes(M, N, true);
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

int t2p_match_attention_backward(const float* qkv, const float* d_msg, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                                 int32_t cross, float* d_qkv, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int M = n_obj, N = n_hints, D = embed_dim;
    T2P_CHECK_ARG(qkv && d_msg && d_qkv, "match_attention_backward: NULL argument");
    T2P_CHECK_ARG(cross == 0 || cross == 1, "match_attention_backward: cross must be 0 (self) or 1 (got %d)", cross);
    T2P_TRY(check_sizes("match_attention_backward", batch, M, N, D));
    if (batch == 0) return 0;
    const int S = M > N ? M : N, DH = D / kHeads;
    const size_t lds = ((size_t)2 * S * DH + (size_t)2 * 64 * (S | 1)) * sizeof(float);   // <= 63 KiB at S = 63, DH = 64
    auto attn = D == 64 ? k_attn_sets_bwd<16> : (D == 128 ? k_attn_sets_bwd<32> : k_attn_sets_bwd<64>);
    ProfScope ps_("match_train_attn_bwd", st);
    hipLaunchKernelGGL(attn, dim3((unsigned)(batch * 2 * kHeads)), dim3(64), lds, st, qkv, d_msg, batch, M, N, cross, d_qkv);
    T2P_CHECK_LAUNCH("match_train_attn_bwd");
    return 0;
}

size_t t2p_match_head_backward_workspace_bytes(int64_t batch, int32_t n_obj, int32_t n_hints, int32_t sinkhorn_iters) {
    if (batch < 0 || n_obj < 1 || n_hints < 1 || n_obj > kMaxTokens || n_hints > kMaxTokens || sinkhorn_iters < 0) return 0;
    return head_bwd_ws_bytes(batch, n_obj, n_hints, sinkhorn_iters);
}

int t2p_match_head_backward(const float* mdesc, const float* dP, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                            float bin_score, int32_t sinkhorn_iters, float* d_mdesc, double* d_bin, void* workspace,
                            size_t workspace_bytes, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int M = n_obj, N = n_hints, D = embed_dim;
    T2P_CHECK_ARG(mdesc && dP && d_mdesc && d_bin, "match_head_backward: NULL argument");
    T2P_TRY(check_sizes("match_head_backward", batch, M, N, D));
    T2P_CHECK_ARG(sinkhorn_iters >= 0, "match_head_backward: sinkhorn_iters < 0");
    const size_t need = head_bwd_ws_bytes(batch, M, N, sinkhorn_iters);
    if (need > 0 && (workspace == nullptr || workspace_bytes < need)) {
        set_error("match_head_backward: workspace %zu < %zu bytes", workspace_bytes, need);
        return T2P_E_WORKSPACE;
    }
    if (batch == 0) return 0;
    // Z0 and its gradient, u_t, v_t, v_{t-1}, gu, gv: <= 66.5 KiB at 63 + 63 tokens
    const size_t lds = head_lds_bytes(M, N, false) + ((size_t)(M + 1) * (N + 1) + (M + 1) + (size_t)2 * (N + 1)) * sizeof(double);
    if (lds > 64 * 1024) T2P_TRY(reserve_lds((const void*)k_head_sets_bwd, 80 * 1024, "match_head_backward"));
    ProfScope ps_("match_train_head_bwd", st);
    hipLaunchKernelGGL(k_head_sets_bwd, dim3((unsigned)batch), dim3(64), lds, st, mdesc, dP, batch, M, N, D, bin_score, sinkhorn_iters,
                       d_mdesc, d_bin, (double*)workspace);
    T2P_CHECK_LAUNCH("match_train_head_bwd");
    return 0;
}

int t2p_matching_loss_backward(const float* P, int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* idx,
                               const int32_t* entry_ptr, int64_t n_entries, const float* g, float* dP, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(P && idx && entry_ptr && g && dP, "matching_loss_backward: NULL argument");
    T2P_CHECK_ARG(batch >= 1 && batch <= 0x7fffffff && n_obj >= 1 && n_hints >= 1,
                  "matching_loss_backward: need batch, n_obj, n_hints >= 1 (got %lld, %d, %d)", (long long)batch, n_obj, n_hints);
    T2P_CHECK_ARG((int64_t)(n_obj + 1) * (n_hints + 1) <= 0x3fffffff, "matching_loss_backward: n_obj, n_hints too large (got %d, %d)",
                  n_obj, n_hints);
    T2P_CHECK_ARG(n_entries >= 1 && n_entries <= 0x3fffffff, "matching_loss_backward: need 1 <= n_entries < 2^30 (got %lld)",
                  (long long)n_entries);
    ProfScope ps_("matching_loss_bwd", st);
    hipLaunchKernelGGL(k_matching_loss_bwd, dim3((unsigned)batch), dim3(kLossThreads), 0, st, P, batch, n_obj + 1, n_hints + 1, idx,
                       entry_ptr, n_entries, g, dP);
    T2P_CHECK_LAUNCH("matching_loss_bwd");
    return 0;
}

int t2p_mse_loss_backward(const float* a, const float* b, int64_t n, const float* g, float* da, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(a && b && g && da, "mse_loss_backward: NULL argument");
    T2P_CHECK_ARG(n >= 1, "mse_loss_backward: no elements");
    const int64_t blocks = (n + kLossThreads - 1) / kLossThreads;
    ProfScope ps_("mse_loss_bwd", st);
    hipLaunchKernelGGL(k_mse_loss_bwd, dim3((unsigned)(blocks < 1024 ? blocks : 1024)), dim3(kLossThreads), 0, st, a, b, n, g, da);
    T2P_CHECK_LAUNCH("mse_loss_bwd");
    return 0;
}

int t2p_colsum(const float* x, int64_t rows, int32_t cols, float* out, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(x && out, "colsum: NULL argument");
    T2P_CHECK_ARG(rows >= 1 && cols >= 1, "colsum: need rows, cols >= 1 (got %lld, %d)", (long long)rows, cols);
    ProfScope ps_("colsum_f64", st);
    hipLaunchKernelGGL(k_colsum, dim3((unsigned)((cols + 63) / 64)), dim3(kLossThreads), 0, st, x, rows, cols, out);
    T2P_CHECK_LAUNCH("colsum_f64");
    return 0;
}

}  // extern "C"
