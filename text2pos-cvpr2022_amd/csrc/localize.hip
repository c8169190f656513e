// The serving path of the fine stage: matching against a database of encoded cells, and the pose estimates of a call on the device.
//
// Replaces (reference): the per-sample torch.stack of object and hint encodings in SuperGlueMatch.forward
// (models/superglue_matcher.py:94-103) for samples whose encodings already exist - a database cell's object tokens, a query's hint
// tokens - and get_pos_in_cell (models/superglue_matcher.py:139-161) with the world-coordinate step of calc_sample_accuracies
// (evaluation/utils.py:31-54: bbox_w + pos_in_cell * cell_size) and the confidence pick of evaluation/pipeline.py:196, :256
// (np.argmax over the candidates' matched-object counts), which the reference runs on host copies, per query.
//
// t2p_match_indexed: ONE gather kernel copies the token rows of the B samples out of the two tables into dense desc0 [B][M][D] /
// desc1 [B][N][D] at the head of the workspace (16-byte loads and stores: D is 64, 128 or 256, a row a whole number of them), then
// t2p_match runs on the copies with the rest of the workspace - the same kernels, so the same bits as t2p_match on gathered inputs.
// The pass moves 2 B (M + N) D 4 bytes, microseconds against the matcher's milliseconds.  A sample whose obj_row or hint_row lies
// outside its table is never read through: all its tokens are NaN (every row GEMM keeps rows apart, so its neighbours are untouched).
//
// t2p_localize_poses: a latency kernel like k_fine_step_stats (fine_stats.hip).  One workgroup per query; its wavefronts take the
// query's K candidates in turn, lane i slot i of the sample (M, N <= 63).  Counts and the float64 sums are reduced over the wavefront
// with a fixed xor butterfly; lane 0 writes the sample's outputs and its count to LDS (K <= 1,024: 4 KiB).  Behind one barrier the
// first wavefront picks the candidate with the most matched objects, first on ties.  No atomics: the same bits from call to call.
// Every output element is written on every path.  A sample with cell_row outside the table, a matches0 value outside [-1, N) or a
// NaN among its N offsets gets NaN rows and matched = -1; nothing is read through such an index (the loads behind it are predicated
// off), and `best` passes such samples over (-1 when the query has no other).
#include "t2p_common.h"

#include "../../include/t2p.h"

namespace t2p {
namespace {

constexpr int kLocThreads = 256;         // 4 wavefronts: a query's top-10 candidates in three turns, K = 1,024 in 256
constexpr int kLocMaxTopK = 1024;        // the LDS counts of the pick: 1024 x int32 = 4 KiB (T2P_LOCALIZE_MAX_TOP_K)
constexpr int kLocMaxTokens = 63;        // t2p_match's limit: a wavefront's lanes cover a set

__global__ __launch_bounds__(256) void k_gather_tokens(const f32x4* __restrict__ obj_table, const f32x4* __restrict__ hint_table,
                                                       const int32_t* __restrict__ obj_row, const int32_t* __restrict__ hint_row,
                                                       int64_t B, int M, int N, int D4, int64_t n_cells, int64_t n_queries,
                                                       f32x4* __restrict__ desc0, f32x4* __restrict__ desc1) {
    const int64_t v0 = (int64_t)M * D4, v1 = (int64_t)N * D4, per = v0 + v1;     // float4s of a sample: objects, hints
    const int64_t total = B * per;
    const float qn = __builtin_nanf("");
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / per, r = i % per;
        const int64_t ro = obj_row[b], rh = hint_row[b];
        const bool ok = ro >= 0 && ro < n_cells && rh >= 0 && rh < n_queries;
        const bool obj = r < v0;
        f32x4 v = {qn, qn, qn, qn};
        if (ok) v = obj ? obj_table[ro * v0 + r] : hint_table[rh * v1 + (r - v0)];      // (nothing is loaded through a bad row)
        if (obj) {
            desc0[b * v0 + r] = v;
        } else {
            desc1[b * v1 + (r - v0)] = v;
        }
    }
}

__global__ __launch_bounds__(kLocThreads) void k_localize_poses(
    const int64_t* __restrict__ matches0, const float* __restrict__ offsets, const int32_t* __restrict__ cell_row, int K, int M, int N,
    const double* __restrict__ center_xy, const double* __restrict__ bbox_xy, const double* __restrict__ cell_size, int64_t n_cells,
    double* __restrict__ pos_mean, double* __restrict__ pos_offset, double* __restrict__ world_mean, double* __restrict__ world_offset,
    int32_t* __restrict__ matched, int32_t* __restrict__ best) {
    __shared__ int counts[kLocMaxTopK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = blockIdx.x;
    const double nan = __builtin_nan("");
    for (int c = wave; c < K; c += kLocThreads / 64) {
        const int64_t s = q * K + c;
        const int64_t row = cell_row[s];
        bool ok = row >= 0 && row < n_cells;
        int64_t m0 = -1;
        if (lane < M) {
            m0 = matches0[s * M + lane];
            if (m0 < -1 || m0 >= N) ok = false;
        }
        if (lane < N) {
            const float* o = offsets + (s * N + lane) * 2;
            if (o[0] != o[0] || o[1] != o[1]) ok = false;
        }
        ok = __all(ok);                                      // from here on every index of the sample is in range, or nothing is read
        int assigned = 0;
        double cx = 0.0, cy = 0.0, ox = 0.0, oy = 0.0;
        if (ok && lane < M && m0 >= 0) {
            assigned = 1;
            const double* ctr = center_xy + (row * M + lane) * 2;
            const float* o = offsets + (s * N + m0) * 2;
            cx = ctr[0];
            cy = ctr[1];
            ox = cx + (double)o[0];
            oy = cy + (double)o[1];
        }
        assigned = wave_sum(assigned);
        cx = wave_sum(cx);
        cy = wave_sum(cy);
        ox = wave_sum(ox);
        oy = wave_sum(oy);
        if (lane == 0) {
            double r[8];
            if (ok) {
                const double k = (double)assigned;
                const double bx = bbox_xy[2 * row], by = bbox_xy[2 * row + 1], size = cell_size[row];
                r[0] = assigned ? cx / k : 0.5;
                r[1] = assigned ? cy / k : 0.5;
                r[2] = assigned ? ox / k : 0.5;
                r[3] = assigned ? oy / k : 0.5;
                r[4] = bx + r[0] * size;
                r[5] = by + r[1] * size;
                r[6] = bx + r[2] * size;
                r[7] = by + r[3] * size;
            } else {
#pragma unroll
                for (int i = 0; i < 8; i++) r[i] = nan;
            }
            pos_mean[2 * s] = r[0];
            pos_mean[2 * s + 1] = r[1];
            pos_offset[2 * s] = r[2];
            pos_offset[2 * s + 1] = r[3];
            world_mean[2 * s] = r[4];
            world_mean[2 * s + 1] = r[5];
            world_offset[2 * s] = r[6];
            world_offset[2 * s + 1] = r[7];
            const int cnt = ok ? assigned : -1;
            matched[s] = cnt;
            counts[c] = cnt;
        }
    }
    __syncthreads();
    if (wave == 0) {
        int bc = -1, bi = -1;                                // lane's own candidates in ascending order: a later one must be larger
        for (int c = lane; c < K; c += 64) {
            const int v = counts[c];
            if (v > bc) {
                bc = v;
                bi = c;
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {                   // larger count wins, the lower index among equals: np.argmax's first maximum
            const int oc = __shfl_xor(bc, o, 64), oi = __shfl_xor(bi, o, 64);
            if (oc > bc || (oc == bc && oc >= 0 && oi < bi)) {
                bc = oc;
                bi = oi;
            }
        }
        if (lane == 0) best[q] = bc >= 0 ? bi : -1;
    }
}

struct IndexedWs {
    float *desc0, *desc1;
    char* rest;
    size_t rest_bytes;
};

size_t carve_indexed(char* base, size_t cap, int64_t B, int M, int N, int D, IndexedWs* ws) {
    const size_t b0 = align_up((size_t)B * M * D * sizeof(float), 256), b1 = align_up((size_t)B * N * D * sizeof(float), 256);
    const size_t inner = t2p_match_workspace_bytes(B, M, N, D);
    if (ws) {
        ws->desc0 = (float*)base;
        ws->desc1 = (float*)(base + b0);
        ws->rest = base + b0 + b1;
        ws->rest_bytes = cap >= b0 + b1 ? cap - (b0 + b1) : 0;
    }
    return b0 + b1 + inner;
}

}  // namespace
}  // namespace t2p

using namespace t2p;

extern "C" {

size_t t2p_match_indexed_workspace_bytes(int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim) {
    if (batch <= 0 || n_obj < 1 || n_hints < 1 || embed_dim < 1) return 256;
    return carve_indexed(nullptr, 0, batch, n_obj, n_hints, embed_dim, nullptr);
}

int t2p_match_indexed(const float* obj_table, int64_t n_cells, const float* hint_table, int64_t n_queries, const int32_t* obj_row,
                      const int32_t* hint_row, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                      const t2p_match_weights* w, int32_t sinkhorn_iters, float match_threshold, float* P, int64_t* matches0,
                      int64_t* matches1, float* mscores0, float* mscores1, float* offsets, void* workspace, size_t workspace_bytes,
                      t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    const int M = n_obj, N = n_hints, D = embed_dim;
    T2P_CHECK_ARG(obj_table && hint_table && obj_row && hint_row && w && P && matches0 && matches1 && mscores0 && mscores1 && offsets,
                  "match_indexed: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && M >= 1 && N >= 1 && M <= kLocMaxTokens && N <= kLocMaxTokens,
                  "match_indexed: need 1 <= n_obj, n_hints <= 63 (got %d, %d)", M, N);
    T2P_CHECK_ARG(n_cells >= 1 && n_cells <= 0x3fffffff && n_queries >= 1 && n_queries <= 0x3fffffff,
                  "match_indexed: need 1 <= n_cells, n_queries < 2^30 table rows (got %lld, %lld)", (long long)n_cells, (long long)n_queries);
    if (D != 64 && D != 128 && D != 256) {
        set_error("match_indexed: embed_dim=%d not built (64, 128, 256)", D);
        return T2P_E_UNSUPPORTED;
    }
    T2P_CHECK_ARG((((uintptr_t)obj_table | (uintptr_t)hint_table) & 15) == 0, "match_indexed: the token tables must be 16-byte aligned");
    T2P_CHECK_ARG(w->n_layers >= 0 && w->n_layers <= 64 && (w->n_layers == 0 || w->cross != nullptr), "match_indexed: bad layer list");
    T2P_CHECK_ARG(sinkhorn_iters >= 0, "match_indexed: sinkhorn_iters < 0");
    {   // t2p_match's own refusal, ahead of the gather: a sample's attention rows (4 heads) must fit the LDS a workgroup may use
        const size_t T = (size_t)M + N, lds_attn = (T * (3 * D + 4) + T * 4 * (M > N ? M : N)) * sizeof(float);
        if (w->n_layers > 0 && lds_attn > 160 * 1024) {
            set_error("match: %d tokens x D=%d need %zu B of LDS per sample (> 160 KiB)", (int)T, D, lds_attn);
            return T2P_E_UNSUPPORTED;
        }
    }
    if (batch == 0) return 0;
    IndexedWs ws;
    const size_t need = carve_indexed((char*)workspace, workspace_bytes, batch, M, N, D, &ws);
    if (workspace == nullptr || need > workspace_bytes || ((uintptr_t)workspace & 15) != 0) {
        set_error("match_indexed: workspace %zu B < %zu B (or not 16-byte aligned)", workspace_bytes, need);
        return T2P_E_WORKSPACE;
    }
    {
        ProfScope ps_("match_gather", st);
        const int D4 = D / 4;
        const int64_t total = batch * (int64_t)(M + N) * D4;
        const unsigned grid = (unsigned)((total + 255) / 256 < 65535 ? (total + 255) / 256 : 65535);
        hipLaunchKernelGGL(k_gather_tokens, dim3(grid), dim3(256), 0, st, (const f32x4*)obj_table, (const f32x4*)hint_table, obj_row,
                           hint_row, batch, M, N, D4, n_cells, n_queries, (f32x4*)ws.desc0, (f32x4*)ws.desc1);
        T2P_CHECK_LAUNCH("match_gather");
    }
    return t2p_match(ws.desc0, ws.desc1, batch, M, N, D, w, sinkhorn_iters, match_threshold, P, matches0, matches1, mscores0, mscores1,
                     offsets, ws.rest, ws.rest_bytes, stream);
}

int t2p_localize_poses(const int64_t* matches0, const float* offsets, const int32_t* cell_row, int64_t n_queries, int32_t top_k,
                       int32_t n_obj, int32_t n_hints, const double* center_xy, const double* bbox_xy, const double* cell_size,
                       int64_t n_cells, double* pos_mean, double* pos_offset, double* world_mean, double* world_offset,
                       int32_t* matched, int32_t* best, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(matches0 && offsets && cell_row && center_xy && bbox_xy && cell_size && pos_mean && pos_offset && world_mean &&
                      world_offset && matched && best,
                  "localize_poses: NULL argument");
    T2P_CHECK_ARG(n_queries >= 0 && n_queries <= 0x7fffffff, "localize_poses: need 0 <= n_queries < 2^31 (got %lld)", (long long)n_queries);
    T2P_CHECK_ARG(top_k >= 1 && top_k <= kLocMaxTopK, "localize_poses: top_k %d outside [1, %d], the candidates the pick holds in LDS", top_k,
                  kLocMaxTopK);
    T2P_CHECK_ARG(n_obj >= 1 && n_hints >= 1 && n_obj <= kLocMaxTokens && n_hints <= kLocMaxTokens,
                  "localize_poses: need 1 <= n_obj, n_hints <= 63, the token limit of the matcher (got %d, %d)", n_obj, n_hints);
    T2P_CHECK_ARG(n_cells >= 1 && n_cells <= 0x3fffffff, "localize_poses: need 1 <= n_cells < 2^30 table rows (got %lld)", (long long)n_cells);
    if (n_queries == 0) return 0;
    ProfScope ps_("localize_poses", st);
    hipLaunchKernelGGL(k_localize_poses, dim3((unsigned)n_queries), dim3(kLocThreads), 0, st, matches0, offsets, cell_row, (int)top_k,
                       (int)n_obj, (int)n_hints, center_xy, bbox_xy, cell_size, n_cells, pos_mean, pos_offset, world_mean, world_offset,
                       matched, best);
    T2P_CHECK_LAUNCH("localize_poses");
    return 0;
}

}  // extern "C"
