// All-pairs cosine scores in float64 + ordered top-k; small calls at k <= 16 keep the scores on the chip.
//
// Replaces the host loop of training/coarse.py:134-140 (per query: `scores = cell_encodings[:] @ text_encodings[q]`
// on float64 arrays, `np.argsort(-scores)[0:max(top_k)]`).  The reference ranks in float64 (np.zeros arrays,
// training/coarse.py:100,103), so the GEMM runs on v_mfma_f64_16x16x4_f64: the fp32 embeddings are widened on the
// fly and every score is an fp64 fma chain -- ranking ties are then only exact duplicates, which are ordered by
// ascending cell index (the pinned stable order, oracle/model.py::retrieve_topk_f64).
//
// Two paths.  Which one runs is a function of the problem size for every k in 1..KREG, never of k within that range:
//     k <= KREG and nq * nc <  kTileMinPairs  -> register lists  (k_sim_partial + k_topk_merge)
//     k <= KREG and nq * nc >= kTileMinPairs  -> score tile      (k_sim_scores + k_topk_select, with the caller's k)
//     k >  KREG                               -> score tile
// (a database so large that one query's scores exceed the tile, nc > 33,554,400, stays on the lists at k <= KREG).  The insertion
// network of the lists sits inside the MFMA loop and halves its fp64 rate, and the merge walks 4 x splits x 16 candidates with one
// wave per query: writing the scores once and selecting from the Infinity Cache was faster at every swept shape (64..1,250 queries
// x 1,000..100,000 cells), 1.1 to 7 times, except k = 1 at 10^8 pairs and more, +2 % and +12 % (profiles/topk_sweep.py --shapes
// route; profiles/t04_topk_route_sweep.md).  kTileMinPairs is the smallest swept product above the 130 x 1,000 call that the tests
// pin to the lists.  Both paths give a pair the same score bits and order by better(): the result does not depend on the route.
//
// Register lists:
// Pass 1  (grid = query blocks x cell splits): a workgroup keeps 128 queries as MFMA B operands in registers
//         (fp32, widened at use), streams its cell range through LDS in 32-row blocks (register-prefetched) and
//         every lane maintains a private sorted top-KCAP list per query in registers.
// Pass 2  (one wave per query): k-round ordered selection over the 4 x splits partial lists.
//
// Score tile (any k up to KMAX; k > KREG cannot keep a list per lane).  The same product loop (sim_product_loop: the score bits of a pair do
// not depend on k) then writes a chunk of queries' float64 scores to the workspace (k_sim_scores), and one workgroup per
// query selects exactly (k_topk_select): MSB-first radix passes over order-preserving 64-bit keys find the k-th key and
// the number of keys above it, an ascending-index sweep with a scan collects everything above and the lowest-index ties,
// and a bitonic sort in LDS puts the k candidates into better() order.  Queries go through in chunks whose score tile
// stays within 256 MiB (the Infinity Cache: the select passes re-read what the score kernel just wrote).
//
// Restricted rankings.  The two product kernels (k_sim_partial, k_sim_scores) come in three compile-time families, MASK; a family's
// epilogue selects -inf for a pair its mask does not allow - a select on the finished score, so an allowed pair has the bits of
// the unrestricted call.  Merge and select order -inf entries after every finite score, lowest cell index first, and are shared.
//     MASK_NONE   t2p_sim_topk: every pair is allowed; reads the embeddings only.
//     MASK_GROUP  t2p_sim_topk_grouped (the street oracle, evaluation/pipeline.py:93-108: `scores[cell_street != pose_street] = -inf`
//                 before the argsort): allowed when the group ids are equal, whatever their sign; reads query_group [nq], cell_group [nc].
//     MASK_PRIOR  t2p_sim_topk_prior (include/t2p_serve.h: the serving path's prior): allowed when the query's prior point lies within
//                 its radius of the cell's closed square (float64, from comparisons so that a NaN anywhere masks the pair) and when the
//                 query's group is negative or equals the cell's.  Reads PriorArgs and the two group arrays; either half may be
//                 absent (a NULL pointer set, uniform over the launch).
// One type, QueryMask<MASK>, holds a lane's query side of the test and answers allowed(); sim_product_loop stages the cell side (group
// ids, boxes) next to the block's rows.  What a family does not read sits behind `if constexpr` and is not compiled into it.
#include <type_traits>

#include "t2p_common.h"

namespace t2p {
namespace {

constexpr int KREG = 16;     // per-lane list capacity == largest k of the register-list path
constexpr int KCAP = KREG;
constexpr int KMAX = 1024;   // largest supported k (the select kernel's LDS candidate array)
#ifndef T2P_SIM_TILE_MIN_PAIRS   // (an A/B build of the sweep forces one path: profiles/topk_sweep.py)
#define T2P_SIM_TILE_MIN_PAIRS 256000
#endif
constexpr int64_t kTileMinPairs = T2P_SIM_TILE_MIN_PAIRS;   // k <= KREG: nq * nc from which the score-tile path runs
constexpr int QB = 128;      // queries per workgroup (4 waves x 2 tiles x 16)
constexpr int CB = 32;       // cells staged per iteration
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));
constexpr int MASK_NONE = 0, MASK_GROUP = 1, MASK_PRIOR = 2;   // the families of the product kernels

// What a MASK_PRIOR kernel reads besides the embeddings: xy [nq][2], radius [nq], box [nc][4] = x0 y0 x1 y1 (all three or none; box
// 16-byte aligned).  The group arrays travel as in MASK_GROUP (both or none).
struct PriorArgs {
    const double* xy;
    const double* radius;
    const double* box;
};

// A query's side of the geometric test in registers: px, py and r * r (-1 for a negative or NaN radius: no distance passes).
struct PriorQuery {
    double px, py, r2;
};
__device__ __forceinline__ PriorQuery prior_query(const PriorArgs& pr, int64_t q, bool in_range) {
    PriorQuery o = {0.0, 0.0, -1.0};
    if (pr.box != nullptr && in_range) {
        const double r = pr.radius[q];
        o.px = pr.xy[2 * q];
        o.py = pr.xy[2 * q + 1];
        o.r2 = r >= 0.0 ? r * r : -1.0;
    }
    return o;
}
// max(lo - p, p - hi, 0) built from comparisons: a NaN in any of the three operands comes out as NaN (fmax would drop it)
__device__ __forceinline__ double prior_gap(double lo, double hi, double p) {
    const double a = lo - p, b = p - hi;
    double m = a > b ? a : b;   // a NaN in b stays; one in a alone is put back below
    m = a != a ? a : m;
    return m < 0.0 ? 0.0 : m;
}
// distance^2 from the prior point to the closed box [x0, x1] x [y0, y1] <= r^2; false on any NaN.  Two products and one sum, not
// contracted: the boundary pairs of integer-valued geometry are exact equalities.
__device__ __forceinline__ bool prior_reaches(const PriorQuery& pq, const f64x2& lo, const f64x2& hi) {
#pragma clang fp contract(off)
    const double dx = prior_gap(lo[0], hi[0], pq.px), dy = prior_gap(lo[1], hi[1], pq.py);
    const double xx = dx * dx, yy = dy * dy;
    return (xx + yy) <= pq.r2;
}

// A lane's query side of the mask: the group ids and prior points of its two queries q0 + 16 t + (lane & 15), t = 0, 1, and which
// halves of the test the launch has (uniform).  What is not read - a query >= nq, an absent half, another family's members - keeps
// its initial value; a prior call without groups thus asks for "any group" (-1), and allowed() needs no has_grp.
template <int MASK>
struct QueryMask {
    int qgrp[2] = {MASK == MASK_PRIOR ? -1 : 0, MASK == MASK_PRIOR ? -1 : 0};
    PriorQuery pq[2] = {};
    bool has_grp, has_geo;

    __device__ __forceinline__ QueryMask(const int32_t* __restrict__ query_group, const int32_t* __restrict__ cell_group,
                                         const PriorArgs& prior, int64_t q0, int64_t nq)
        : has_grp(MASK == MASK_GROUP || (MASK == MASK_PRIOR && cell_group != nullptr)),
          has_geo(MASK == MASK_PRIOR && prior.box != nullptr) {
        if constexpr (MASK != MASK_NONE) {
#pragma unroll
            for (int t = 0; t < 2; t++) {
                const int64_t q = q0 + t * 16 + (threadIdx.x & 15);
                if (has_grp && q < nq) qgrp[t] = query_group[q];
                if constexpr (MASK == MASK_PRIOR) pq[t] = prior_query(prior, q, q < nq);
            }
        }
    }
    // the pair (query t of this lane, a cell of group cgrp); box: the cell's four doubles in LDS (read only with has_geo)
    __device__ __forceinline__ bool allowed(int t, int cgrp, const double* box) const {
        if constexpr (MASK == MASK_GROUP) return cgrp == qgrp[t];
        if constexpr (MASK == MASK_PRIOR) {
            bool ok = qgrp[t] < 0 || cgrp == qgrp[t];
            if (has_geo) ok = ok && prior_reaches(pq[t], *(const f64x2*)box, *(const f64x2*)(box + 2));
            return ok;
        }
        return true;
    }
};

struct Cand {
    double s;
    int i;
};
__device__ __forceinline__ bool better(double s, int i, double s2, int i2) { return s > s2 || (s == s2 && i < i2); }

// D layout of v_mfma_f64_16x16x4_f64: column (query) = lane & 15, row (cell) = (lane >> 4) + 4 * reg
__device__ __forceinline__ int d_row(int lane, int reg) { return (lane >> 4) + 4 * reg; }

// A lane of the product loop owns cells cell0 + (lane >> 4) + 4 r of a 16-cell tile; where its four values are kept side by
// side, cell c sits at tile_pos(c) = (c & ~15) | (c & 3) << 2 | (c >> 2) & 3 (the two 2-bit fields swapped; its own inverse).
__device__ __forceinline__ int tile_pos(int c) { return (c & ~15) | ((c & 3) << 2) | ((c >> 2) & 3); }

// The LDS of a product kernel: c = the block's CB cell rows (pitch DIM + 4), g = its group ids at tile_pos (MASK != MASK_NONE),
// b = its boxes, 4 doubles per cell (MASK_PRIOR).
struct ProductLds {
    float* c;
    int* g;
    double* b;
    // the box of the cell in row d_row(lane, r) of the tile that starts at cell0 (blocks start at c_begin + a multiple of CB)
    __device__ __forceinline__ const double* box(int64_t cell0, int64_t c_begin, int lane, int r) const {
        return b + 4 * (((int)(cell0 - c_begin) & (CB - 1)) + d_row(lane, r));
    }
};
template <int DIM, int MASK>
__device__ __forceinline__ ProductLds product_lds() {
    __shared__ __attribute__((aligned(16))) float c_buf[CB * (DIM + 4)];
    ProductLds lds = {c_buf, nullptr, nullptr};
    if constexpr (MASK != MASK_NONE) {
        __shared__ __attribute__((aligned(16))) int g_buf[CB];
        lds.g = g_buf;
    }
    if constexpr (MASK == MASK_PRIOR) {
        __shared__ __attribute__((aligned(16))) double b_buf[CB * 4];
        lds.b = b_buf;
    }
    return lds;
}

// The product loop of both paths: a workgroup of 4 waves keeps queries [q0_wg, q0_wg + QB) as MFMA B operands in registers
// (wave w: two 16-query tiles from q0_wg + 32 w), streams cells [c_begin, c_end) through c_lds in CB-row blocks
// (register-prefetched) and hands every finished 16 x 16 tile to epi(t, cell0, acc): lane `lane` holds, for query
// q0_wg + 32 w + 16 t + (lane & 15), the scores of cells cell0 + d_row(lane, r) in acc[r], r = 0..3 (cells >= c_end are
// products with zero rows; the epilogue drops them).  One fp64 fma chain over dim per pair, the same whatever the epilogue.
// With groups (mask.has_grp: MASK_GROUP, or MASK_PRIOR with the group arrays) the block's CB group ids travel with its rows - one
// register of the first CB threads, prefetched under the same cell < c_end guard (nothing is read past cell_group[c_end - 1]),
// stored to lds.g at tile_pos so that a lane's four cells sit side by side - and epi receives them as cg[r] (ids of cells >= c_end
// are 0 and unused).  Without groups cell_group / lds.g are not touched and cg is a constant the epilogues ignore.
// With geometry (mask.has_geo: MASK_PRIOR with the boxes) the block's CB boxes travel the same way - one 16-byte half box in a
// register pair of the first 2 CB threads, prefetched under the same guard (nothing is read past cell_box[c_end - 1]), stored to
// lds.b as [cell of the block][x0 y0 x1 y1]; the epilogue reads its four cells' boxes at lds.box().
template <int DIM, int MASK, class Epi>
__device__ __forceinline__ void sim_product_loop(const float* __restrict__ Q, const float* __restrict__ Cm, int64_t nq,
                                                 int64_t q0_wg, int64_t c_begin, int64_t c_end, const ProductLds& lds,
                                                 const QueryMask<MASK>& mask, const int32_t* __restrict__ cell_group,
                                                 const double* __restrict__ cell_box, Epi&& epi) {
    float* const c_lds = lds.c;
    constexpr int LDC = DIM + 4;
    constexpr int KQ = DIM / 4;   // k per lane group (lane>>4 owns k in [g*KQ, (g+1)*KQ))
    constexpr int F4 = CB * DIM / 4 / 256;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    const int64_t q0 = q0_wg + wave * 32;

    // B operands: this wave's 2 query tiles, fp32 in registers
    float qreg[2][KQ];
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int64_t q = q0 + t * 16 + l15;
#pragma unroll
        for (int s4 = 0; s4 < KQ / 4; s4++) {
            f32x4 v = {0.f, 0.f, 0.f, 0.f};
            if (q < nq) v = *(const f32x4*)(Q + q * DIM + g4 * KQ + s4 * 4);
#pragma unroll
            for (int e = 0; e < 4; e++) qreg[t][s4 * 4 + e] = v[e];
        }
    }

    f32x4 stage[F4];
    int gstage = 0;
    f64x2 bstage = {0.0, 0.0};
    auto load_block = [&](int64_t cb) {
        if constexpr (MASK != MASK_NONE) {
            if (mask.has_grp && tid < CB) gstage = (cb + tid) < c_end ? cell_group[cb + tid] : 0;
        }
        if constexpr (MASK == MASK_PRIOR) {
            if (mask.has_geo && tid < 2 * CB)
                bstage = (cb + (tid >> 1)) < c_end ? *(const f64x2*)(cell_box + (cb + (tid >> 1)) * 4 + (tid & 1) * 2) : f64x2{0.0, 0.0};
        }
#pragma unroll
        for (int it = 0; it < F4; it++) {
            const int qd = it * 256 + tid;
            const int r = qd / (DIM / 4), c4 = qd % (DIM / 4);
            const int64_t cell = cb + r;
            stage[it] = cell < c_end ? *(const f32x4*)(Cm + cell * DIM + c4 * 4) : f32x4{0.f, 0.f, 0.f, 0.f};
        }
    };
    auto store_block = [&]() {
        if constexpr (MASK != MASK_NONE) {
            if (mask.has_grp && tid < CB) lds.g[tile_pos(tid)] = gstage;
        }
        if constexpr (MASK == MASK_PRIOR) {
            if (mask.has_geo && tid < 2 * CB) *(f64x2*)(lds.b + 2 * tid) = bstage;
        }
#pragma unroll
        for (int it = 0; it < F4; it++) {
            const int qd = it * 256 + tid;
            const int r = qd / (DIM / 4), c4 = qd % (DIM / 4);
            *(f32x4*)(c_lds + r * LDC + c4 * 4) = stage[it];
        }
    };

    if (c_begin < c_end) load_block(c_begin);
    for (int64_t cb = c_begin; cb < c_end; cb += CB) {
        store_block();
        __syncthreads();
        if (cb + CB < c_end) load_block(cb + CB);
#pragma unroll
        for (int ct = 0; ct < CB / 16; ct++) {
            f64x4 acc[2];
#pragma unroll
            for (int t = 0; t < 2; t++) acc[t] = f64x4{0.0, 0.0, 0.0, 0.0};
            if constexpr (MASK == MASK_PRIOR && DIM >= 256) {
                // The compiler widens the loop-invariant queries once, ahead of the loop: 2 * DIM / 4 more registers, which beside
                // the prior's no longer fit (the lists at 256, both kernels at 384) and would go to scratch.  An empty asm that
                // "rewrites" each fp32 query per tile, in an accumulation register, keeps them in the AGPR half of the file and
                // the widening (one read, one convert) at its use, in the shadow of the MFMA it feeds.
#pragma unroll
                for (int t = 0; t < 2; t++)
#pragma unroll
                    for (int j = 0; j < KQ; j++) asm volatile("" : "+a"(qreg[t][j]));
            }
            const float* arow = c_lds + (ct * 16 + l15) * LDC + g4 * KQ;
#pragma unroll
            for (int s4 = 0; s4 < KQ / 4; s4++) {
                const f32x4 a = *(const f32x4*)(arow + s4 * 4);
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const double ad = (double)a[e];
#pragma unroll
                    for (int t = 0; t < 2; t++)
                        acc[t] = __builtin_amdgcn_mfma_f64_16x16x4f64(ad, (double)qreg[t][s4 * 4 + e], acc[t], 0, 0, 0);
                }
            }
            i32x4 cg = {0, 0, 0, 0};
            if constexpr (MASK != MASK_NONE) {
                if (mask.has_grp) cg = *(const i32x4*)(lds.g + ct * 16 + g4 * 4);   // == tile_pos(ct * 16 + d_row(lane, r)), r = 0..3
            }
#pragma unroll
            for (int t = 0; t < 2; t++) epi(t, cb + ct * 16, acc[t], cg);
        }
        __syncthreads();
    }
}

// A pair the mask does not allow enters the lists as (-inf, cell) - a select on the finished score, so the allowed pairs' bits
// are those of the MASK_NONE kernel; the lists start at (-inf, 0x7fffffff), so masked cells fill what the mask leaves.
template <int DIM, int MASK>
__global__ __launch_bounds__(256, 1) void k_sim_partial(const float* __restrict__ Q, const float* __restrict__ Cm,
                                                         const int32_t* __restrict__ query_group,
                                                         const int32_t* __restrict__ cell_group,
                                                         int64_t nq, int64_t nc, int cells_per_split,
                                                         double* __restrict__ ps, int* __restrict__ pi, int n_split, PriorArgs prior) {
    const ProductLds lds = product_lds<DIM, MASK>();
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, g4 = lane >> 4, l15 = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.x * QB + wave * 32;
    const int split = blockIdx.y;
    const int64_t c_begin = (int64_t)split * cells_per_split;
    const int64_t c_end = (c_begin + cells_per_split) < nc ? (c_begin + cells_per_split) : nc;

    double ls[2][KCAP];
    int li[2][KCAP];
#pragma unroll
    for (int t = 0; t < 2; t++)
#pragma unroll
        for (int j = 0; j < KCAP; j++) { ls[t][j] = -INFINITY; li[t][j] = 0x7fffffff; }
    const QueryMask<MASK> mask(query_group, cell_group, prior, q0, nq);

    sim_product_loop<DIM, MASK>(Q, Cm, nq, (int64_t)blockIdx.x * QB, c_begin, c_end, lds, mask, cell_group, prior.box,
                                [&](int t, int64_t cell0, const f64x4& acc, const i32x4& cg) {
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const int64_t cell = cell0 + d_row(lane, r);
            const double s = mask.allowed(t, cg[r], lds.box(cell0, c_begin, lane, r)) ? acc[r] : -INFINITY;
            const int ci = (int)cell;
            if (cell < c_end && better(s, ci, ls[t][KCAP - 1], li[t][KCAP - 1])) {
                ls[t][KCAP - 1] = s;
                li[t][KCAP - 1] = ci;
#pragma unroll
                for (int j = KCAP - 1; j > 0; j--) {
                    const bool sw = better(ls[t][j], li[t][j], ls[t][j - 1], li[t][j - 1]);
                    const double ts = ls[t][j];
                    const int ti = li[t][j];
                    ls[t][j] = sw ? ls[t][j - 1] : ts;
                    li[t][j] = sw ? li[t][j - 1] : ti;
                    ls[t][j - 1] = sw ? ts : ls[t][j - 1];
                    li[t][j - 1] = sw ? ti : li[t][j - 1];
                }
            }
        }
    });
    // partial lists: [q][split][g4][KCAP]
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int64_t q = q0 + t * 16 + l15;
        if (q < nq) {
            const int64_t base = ((q * n_split + split) * 4 + g4) * KCAP;
#pragma unroll
            for (int j = 0; j < KCAP; j++) { ps[base + j] = ls[t][j]; pi[base + j] = li[t][j]; }
        }
    }
}

// one wave per query: k ordered selection rounds over n_cand candidates
__global__ __launch_bounds__(256) void k_topk_merge(const double* __restrict__ ps, const int* __restrict__ pi,
                                                    int64_t nq, int n_cand, int k, int64_t index_offset,
                                                    int64_t* __restrict__ out_idx, double* __restrict__ out_score) {
    const int lane = threadIdx.x & 63;
    const int64_t q = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (q >= nq) return;
    const double* s = ps + q * n_cand;
    const int* id = pi + q * n_cand;
    double last_s = INFINITY;
    int last_i = -1;
    for (int r = 0; r < k; r++) {
        double bs = -INFINITY;
        int bi = 0x7fffffff;
        for (int c = lane; c < n_cand; c += 64) {
            const double cs = s[c];
            const int ci = id[c];
            if (ci == 0x7fffffff) continue;
            const bool after = better(last_s, last_i, cs, ci);  // strictly after the previous pick
            if (after && better(cs, ci, bs, bi)) { bs = cs; bi = ci; }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
            const double os = __shfl_xor(bs, off, 64);
            const int oi = __shfl_xor(bi, off, 64);
            if (better(os, oi, bs, bi)) { bs = os; bi = oi; }
        }
        if (lane == 0) {
            const bool ok = bi != 0x7fffffff;
            out_idx[q * k + r] = ok ? (int64_t)bi + index_offset : -1;
            out_score[q * k + r] = ok ? bs : -INFINITY;
        }
        if (bi == 0x7fffffff) { last_s = -INFINITY; last_i = 0x7fffffff; }
        else { last_s = bs; last_i = bi; }
    }
}

// ---- k in (KREG, KMAX]: score tile + exact selection ---------------------------------------------------------------------
// Score tile of a query chunk: row q holds ld_s (a multiple of 16) doubles.  A lane stores its four scores side by side, so
// cell c of a row sits at tile_pos(c) and the four lane groups of a query fill one 128-byte line.

// A pair the mask does not allow is written as -inf (score_key(-inf) > 0: k_topk_select retrieves it after every finite score,
// lowest index first).
template <int DIM, int MASK>
__global__ __launch_bounds__(256, 1) void k_sim_scores(const float* __restrict__ Q, const float* __restrict__ Cm,
                                                        const int32_t* __restrict__ query_group,
                                                        const int32_t* __restrict__ cell_group,
                                                        int64_t nq, int64_t nc, int cells_per_split,
                                                        double* __restrict__ S, int64_t ld_s, PriorArgs prior) {
    const ProductLds lds = product_lds<DIM, MASK>();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g4 = lane >> 4, l15 = lane & 15;
    const int64_t q0 = (int64_t)blockIdx.x * QB + wave * 32;
    const int64_t c_begin = (int64_t)blockIdx.y * cells_per_split;
    const int64_t c_end = (c_begin + cells_per_split) < nc ? (c_begin + cells_per_split) : nc;
    const QueryMask<MASK> mask(query_group, cell_group, prior, q0, nq);
    sim_product_loop<DIM, MASK>(Q, Cm, nq, (int64_t)blockIdx.x * QB, c_begin, c_end, lds, mask, cell_group, prior.box,
                                [&](int t, int64_t cell0, const f64x4& acc, const i32x4& cg) {
        const int64_t q = q0 + t * 16 + l15;
        // whole 16-cell tiles: cell0 < c_end <= nc keeps cell0 + 15 < ld_s; the cells past nc in the last one are never read
        if (q < nq && cell0 < c_end) {
            double s[4];
#pragma unroll
            for (int r = 0; r < 4; r++) s[r] = mask.allowed(t, cg[r], lds.box(cell0, c_begin, lane, r)) ? acc[r] : -INFINITY;
            double* dst = S + q * ld_s + cell0 + g4 * 4;   // == tile_pos(cell0 + d_row(lane, r)) for r = 0..3
            *(f64x2*)dst = f64x2{s[0], s[1]};
            *(f64x2*)(dst + 2) = f64x2{s[2], s[3]};
        }
    });
}

// Order-preserving key of a score: a > b as doubles <=> key(a) > key(b); -0.0 and +0.0 share a key; every NaN maps to 0,
// below -inf (whose key is 0x000f'ffff'ffff'ffff), so "key > 0" is "may be retrieved".
__device__ __forceinline__ uint64_t score_key(double s) {
    uint64_t u = (uint64_t)__double_as_longlong(s);
    if (s != s) return 0;
    if (s == 0.0) u = 0;
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}

constexpr int SEL_T = 1024;       // threads of the select workgroup: a pass is a chain of dependent L2 / Infinity Cache reads per
constexpr int SEL_W = SEL_T / 64; // thread, and a chunk of a large database has only a few hundred queries (= workgroups) to hide them
constexpr int SEL_U = 4;          // loads in flight per thread in the passes over the scores
constexpr int RBITS = 11;         // radix bits per pass: 2048 bins = 8 KB of LDS, 2 bins per thread in the suffix scan
constexpr int RBINS = 1 << RBITS;

// exclusive prefix sum over the workgroup's threads; wsum: SEL_W ints of LDS.  Every thread must call it.
__device__ __forceinline__ int block_excl_scan(int v, int* wsum) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();   // (wsum may still be read from the previous call)
    if (lane == 63) wsum[wave] = inc;
    __syncthreads();
    int base = 0;
    for (int w = 0; w < wave; w++) base += wsum[w];
    return base + inc - v;
}

// One workgroup per query of the chunk.  kk = min(k, cells whose score is not NaN) entries are real, the rest -1 / -inf.
__global__ __launch_bounds__(SEL_T) void k_topk_select(const double* __restrict__ S, int64_t ld_s, int nc, int k,
                                                       int64_t index_offset, int64_t* __restrict__ out_idx,
                                                       double* __restrict__ out_score) {
    __shared__ int hist[RBINS];
    __shared__ double cand_s[KMAX];
    __shared__ int cand_i[KMAX];
    __shared__ int wsum[SEL_W];
    __shared__ int seg_gt[SEL_W], seg_eq[SEL_W];
    __shared__ int sh_nan, sh_bin, sh_above, sh_count;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double* row = S + (int64_t)blockIdx.x * ld_s;
    out_idx += (int64_t)blockIdx.x * k;
    out_score += (int64_t)blockIdx.x * k;

    // ---- radix descent: T = the kk-th largest key, n_gt = keys above it ----------------------------------------------------
    uint64_t prefix = 0;   // the bits of T found so far (the top 64 - shift bits)
    int shift = 64;
    int need = 0, kk = 0;  // need: rank of T among the keys that share its prefix
    bool take_all = false; // early stop: every key with this prefix is wanted, T = the smallest such key - 1
    if (tid == 0) sh_nan = 0;
    for (int pass = 0; shift > 0; pass++) {
        const int width = shift >= RBITS ? RBITS : shift;
        const int hi_shift = shift;   // keys taking part: key >> hi_shift == prefix (pass 0: all)
        shift -= width;
        for (int b = tid; b < RBINS; b += SEL_T) hist[b] = 0;
        __syncthreads();
        int n_nan = 0;
        for (int c0 = 0; c0 < nc; c0 += SEL_T * SEL_U) {
            double sv[SEL_U];
#pragma unroll
            for (int u = 0; u < SEL_U; u++) {
                const int c = c0 + u * SEL_T + tid;
                sv[u] = c < nc ? row[tile_pos(c)] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < SEL_U; u++) {
                const int c = c0 + u * SEL_T + tid;
                bool act = false;
                int bin = 0;
                if (c < nc) {
                    const uint64_t key = score_key(sv[u]);
                    if (pass == 0) { act = true; n_nan += key == 0; }
                    else act = (key >> hi_shift) == prefix;
                    bin = (int)((key >> shift) & (uint64_t)((1 << width) - 1));
                }
                // cosine scores share their leading bits: the first passes send most of a wave to a few bins.  Up to 4 of a wave's
                // bins are counted with one atomic each; what is left (spread bins) goes one atomic per lane.
                for (int it = 0; it < 4; it++) {
                    const uint64_t m = __ballot(act);
                    if (m == 0) break;
                    const int leader = __ffsll((unsigned long long)m) - 1;
                    const int b = __shfl(bin, leader, 64);
                    const bool same = act && bin == b;
                    const uint64_t ms = __ballot(same);
                    if (lane == leader) atomicAdd(&hist[b], __popcll(ms));
                    act = act && !same;
                }
                if (act) atomicAdd(&hist[bin], 1);
            }
        }
        if (pass == 0 && n_nan) atomicAdd(&sh_nan, n_nan);
        __syncthreads();
        if (pass == 0) {
            const int valid = nc - sh_nan;
            kk = k < valid ? k : valid;
            need = kk;
            if (kk == 0) break;   // (uniform)
        }
        // thread t owns RBINS / SEL_T bins from RBINS - 1 - t * (RBINS / SEL_T) downwards: `above` = keys in the bins above its own
        int own = 0;
        int cnt[RBINS / SEL_T];
#pragma unroll
        for (int j = 0; j < RBINS / SEL_T; j++) { cnt[j] = hist[RBINS - 1 - (tid * (RBINS / SEL_T) + j)]; own += cnt[j]; }
        int above = block_excl_scan(own, wsum);
        if (above < need && need <= above + own) {   // exactly one thread: the bins' total is >= need
#pragma unroll
            for (int j = 0; j < RBINS / SEL_T; j++) {
                if (above < need && need <= above + cnt[j]) {
                    sh_bin = RBINS - 1 - (tid * (RBINS / SEL_T) + j);
                    sh_above = above;
                    sh_count = cnt[j];
                }
                above += cnt[j];
            }
        }
        __syncthreads();
        prefix = (prefix << width) | (uint64_t)sh_bin;
        need -= sh_above;
        const int in_bin = sh_count;
        __syncthreads();   // (sh_* and hist are rewritten by the next pass)
        if (shift > 0 && in_bin == need && prefix != 0) { take_all = true; break; }
    }

    if (kk > 0) {
        // keys above T are taken, and of the keys equal to T the `n_eq` of lowest cell index
        const uint64_t T = take_all ? (prefix << shift) - 1 : prefix;
        const int n_eq = take_all ? 0 : need;
        const int n_gt = kk - n_eq;
        // ---- ascending-index sweep: wave w owns cells [w * seg, (w + 1) * seg), 64 at a time; counts first, then positions ----
        // (the places come from ballots and running counts in index order, never from the order atomics arrive in)
        const int seg = ((nc + SEL_W * 64 - 1) / (SEL_W * 64)) * 64;
        const int c_lo = wave * seg, c_hi = (c_lo + seg) < nc ? (c_lo + seg) : nc;
        int my_gt = 0, my_eq = 0;
        for (int c0 = c_lo + lane; c0 < c_hi; c0 += 64 * SEL_U) {
            double sv[SEL_U];
#pragma unroll
            for (int u = 0; u < SEL_U; u++) sv[u] = (c0 + 64 * u) < c_hi ? row[tile_pos(c0 + 64 * u)] : 0.0;
#pragma unroll
            for (int u = 0; u < SEL_U; u++) {
                const uint64_t key = score_key(sv[u]);
                my_gt += (c0 + 64 * u) < c_hi && key > T;
                my_eq += (c0 + 64 * u) < c_hi && key == T;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) { my_gt += __shfl_xor(my_gt, o, 64); my_eq += __shfl_xor(my_eq, o, 64); }
        if (lane == 0) { seg_gt[wave] = my_gt; seg_eq[wave] = my_eq; }
        __syncthreads();
        int run_gt = 0, run_eq = 0;   // entries of each kind at lower cell indices than this wave's next 64
        for (int w = 0; w < wave; w++) { run_gt += seg_gt[w]; run_eq += seg_eq[w]; }
        const uint64_t below = (1ull << lane) - 1;
        for (int cu = c_lo; cu < c_hi; cu += 64 * SEL_U) {
            double sv[SEL_U];
#pragma unroll
            for (int u = 0; u < SEL_U; u++) sv[u] = (cu + 64 * u + lane) < c_hi ? row[tile_pos(cu + 64 * u + lane)] : 0.0;
#pragma unroll
            for (int u = 0; u < SEL_U; u++) {
                const int c = cu + 64 * u + lane;
                const double s = sv[u];
                const uint64_t key = score_key(s);
                const bool gt = c < c_hi && key > T, eq = c < c_hi && key == T;
                const uint64_t m_gt = __ballot(gt), m_eq = __ballot(eq);
                int slot = -1;
                if (gt) slot = run_gt + __popcll(m_gt & below);
                else if (eq) {
                    const int e = run_eq + __popcll(m_eq & below);
                    if (e < n_eq) slot = n_gt + e;
                }
                if (slot >= 0 && slot < KMAX) { cand_s[slot] = s; cand_i[slot] = c; }
                run_gt += __popcll(m_gt);
                run_eq += __popcll(m_eq);
            }
        }
    }
    // ---- bitonic sort of the candidates on better(), padded to a power of two with entries that sort last ------------------
    int n2 = 1;
    while (n2 < kk) n2 <<= 1;
    for (int j = kk + tid; j < n2; j += SEL_T) { cand_s[j] = -INFINITY; cand_i[j] = 0x7fffffff; }
    __syncthreads();
    for (int size = 2; size <= n2; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int p = tid; p < (n2 >> 1); p += SEL_T) {
                const int i = ((p & ~(stride - 1)) << 1) | (p & (stride - 1));   // lower element of the pair
                const int j = i | stride;
                const bool first_wins = (i & size) == 0;   // this run ends up best-first (the last stage: all of them)
                const double si = cand_s[i], sj = cand_s[j];
                const int ii = cand_i[i], ij = cand_i[j];
                if (better(sj, ij, si, ii) == first_wins) {
                    cand_s[i] = sj; cand_i[i] = ij;
                    cand_s[j] = si; cand_i[j] = ii;
                }
            }
            __syncthreads();
        }
    }
    for (int j = tid; j < k; j += SEL_T) {
        const bool ok = j < kk;
        out_idx[j] = ok ? (int64_t)cand_i[j] + index_offset : -1;
        out_score[j] = ok ? cand_s[j] : -INFINITY;
    }
}

int pick_splits(int64_t nq, int64_t nc) {
    const int64_t qblocks = nq > 0 ? (nq + QB - 1) / QB : 1;   // (the size query of an empty call)
    int64_t want = (2LL * num_cus() + qblocks - 1) / qblocks;  // ~2 workgroups per CU in flight
    int64_t max_split = (nc + 4 * CB - 1) / (4 * CB);          // keep >= 128 cells per split
    if (want > max_split) want = max_split;
    if (want < 1) want = 1;
    if (want > 1024) want = 1024;
    return (int)want;
}

// k > KREG: queries per chunk and the row stride of the score tile (include/t2p.h states the formula); chunk 0 = one
// query's scores alone exceed the tile bound
constexpr size_t kScoreTileBytes = (size_t)256 << 20;   // the Infinity Cache
int64_t score_ld(int64_t nc) { return (nc + 15) / 16 * 16; }
int64_t score_chunk(int64_t nq, int64_t nc) {
    const size_t row = (size_t)score_ld(nc) * sizeof(double);
    int64_t cap = row == 0 ? nq : (int64_t)((kScoreTileBytes - 256) / row);
    if (cap >= QB) cap = cap / QB * QB;   // whole query blocks of the score kernel
    return nq < cap ? nq : cap;
}

// The run-time (dim, mask) as compile-time constants: f(D, M) with decltype(D)::value = DIM, decltype(M)::value = MASK.
// dim is one of the three instantiated widths (sim_topk_impl refuses any other).
template <class F>
void with_dim_mask(int dim, int mask, F&& f) {
    auto with_mask = [&](auto d) {
        if (mask == MASK_PRIOR) f(d, std::integral_constant<int, MASK_PRIOR>{});
        else if (mask == MASK_GROUP) f(d, std::integral_constant<int, MASK_GROUP>{});
        else f(d, std::integral_constant<int, MASK_NONE>{});
    };
    if (dim == 256) with_mask(std::integral_constant<int, 256>{});
    else if (dim == 384) with_mask(std::integral_constant<int, 384>{});
    else with_mask(std::integral_constant<int, 128>{});
}

// The route (the rule at the top of the file): a function of (nq, nc) alone for every k <= KREG
bool use_score_tile(int64_t nq, int64_t nc, int k) {
    if (k > KREG) return true;
    const bool large = nq > 0 && nc > 0 && (nq >= kTileMinPairs || nc >= (kTileMinPairs + nq - 1) / nq);   // nq * nc >= kTileMinPairs
    return large && score_chunk(1, nc) > 0;
}

// What every entry point refuses first, under its own name.  An empty side has no storage to point to (nq == 0 launches nothing;
// k < 1 is refused by its range, in sim_topk_impl).
int check_sizes_and_pointers(const char* name, const float* Q, const float* Cm, int64_t nq, int64_t nc, int k, const int64_t* out_idx,
                             const double* out_score) {
    T2P_CHECK_ARG(nq >= 0 && nc >= 0, "%s: negative size", name);
    T2P_CHECK_ARG((Q != nullptr || nq == 0) && (Cm != nullptr || nc == 0) && ((out_idx != nullptr && out_score != nullptr) || nq == 0 || k < 1),
                  "%s: NULL argument", name);
    return 0;
}

// every entry point: the family `mask` with what it reads (qg / cg are nullptr for MASK_NONE, pr's members for all but MASK_PRIOR)
int sim_topk_impl(int mask, const float* Q, const float* Cm, const int32_t* qg, const int32_t* cg, const PriorArgs& pr, int64_t nq,
                  int64_t nc, int dim, int k, int64_t c_index_offset, int64_t* out_idx, double* out_score, void* ws, size_t ws_bytes,
                  hipStream_t st) {
    T2P_CHECK_ARG(k >= 1 && k <= KMAX, "sim_topk: k=%d outside [1,%d]", k, KMAX);
    T2P_CHECK_ARG(dim == 256 || dim == 128 || dim == 384, "sim_topk: dim=%d not instantiated (128, 256, 384)", dim);
    T2P_CHECK_ARG(nc < 0x7fffffff, "sim_topk: nc too large");
    T2P_CHECK_ARG((((uintptr_t)Q) & 15) == 0 && (((uintptr_t)Cm) & 15) == 0, "sim_topk: Q and C must be 16-byte aligned");
    T2P_CHECK_ARG(k <= KREG || score_chunk(1, nc) > 0,
                  "sim_topk: k=%d > %d keeps one query's float64 scores (8 B x nc=%lld) in a workspace tile of at most %zu B: nc too large",
                  k, KREG, (long long)nc, kScoreTileBytes);
    if (nq == 0) return 0;
    const size_t need = sim_topk_workspace_bytes(nq, nc, k);
    if (ws_bytes < need || ws == nullptr) {
        set_error("sim_topk: workspace %zu B < required %zu B", ws_bytes, need);
        return T2P_E_WORKSPACE;
    }
    if (use_score_tile(nq, nc, k)) {
        T2P_CHECK_ARG((((uintptr_t)ws) & 15) == 0, "sim_topk: workspace must be 16-byte aligned");
        const int64_t chunk = score_chunk(nq, nc), ld_s = score_ld(nc);
        double* S = (double*)ws;
        for (int64_t qa = 0; qa < nq; qa += chunk) {   // chunks run back to back on `st`: the tile is reused in stream order
            const int64_t n = (nq - qa) < chunk ? (nq - qa) : chunk;
            if (nc > 0) {
                const int sp = pick_splits(n, nc);
                int cps = (int)((nc + sp - 1) / sp);
                cps = ((cps + CB - 1) / CB) * CB;
                const dim3 grid((unsigned)((n + QB - 1) / QB), (unsigned)sp);
                ProfScope ps_("sim_scores", st);
                const int32_t* qga = qg ? qg + qa : nullptr;   // the chunk's queries: the per-query arrays move with qa
                const PriorArgs pra = pr.box ? PriorArgs{pr.xy + 2 * qa, pr.radius + qa, pr.box} : pr;
                with_dim_mask(dim, mask, [&](auto D, auto M) {
                    hipLaunchKernelGGL((k_sim_scores<decltype(D)::value, decltype(M)::value>), grid, dim3(256), 0, st, Q + qa * dim, Cm,
                                       qga, cg, n, nc, cps, S, ld_s, pra);
                });
            }
            T2P_CHECK_LAUNCH("sim_scores");
            ProfScope ps2_("topk_select", st);
            hipLaunchKernelGGL(k_topk_select, dim3((unsigned)n), dim3(SEL_T), 0, st, (const double*)S, ld_s, (int)nc, k,
                               c_index_offset, out_idx + qa * k, out_score + qa * k);
            T2P_CHECK_LAUNCH("topk_select");
        }
        return 0;
    }
    const int sp = pick_splits(nq, nc);
    const int64_t n_lists = nq * sp * 4 * KCAP;
    double* ps = (double*)ws;
    int* pi = (int*)(ps + n_lists);
    int cps = (int)((nc + sp - 1) / sp);
    cps = ((cps + CB - 1) / CB) * CB;
    dim3 grid((unsigned)((nq + QB - 1) / QB), (unsigned)sp);
    {
    ProfScope ps_("sim_partial", st);
    with_dim_mask(dim, mask, [&](auto D, auto M) {
        hipLaunchKernelGGL((k_sim_partial<decltype(D)::value, decltype(M)::value>), grid, dim3(256), 0, st, Q, Cm, qg, cg, nq, nc, cps,
                           ps, pi, sp, pr);
    });
    }
    T2P_CHECK_LAUNCH("sim_partial");
    ProfScope ps2_("topk_merge", st);
    hipLaunchKernelGGL(k_topk_merge, dim3((unsigned)((nq + 3) / 4)), dim3(256), 0, st, ps, pi, nq, sp * 4 * KCAP, k,
                       c_index_offset, out_idx, out_score);
    T2P_CHECK_LAUNCH("topk_merge");
    return 0;
}
constexpr PriorArgs kNoPrior = {nullptr, nullptr, nullptr};

}  // namespace

size_t sim_topk_workspace_bytes(int64_t nq, int64_t nc, int k) {
    if (use_score_tile(nq, nc, k)) return (size_t)score_chunk(nq, nc) * score_ld(nc) * sizeof(double) + 256;
    const int sp = pick_splits(nq, nc);
    return (size_t)nq * sp * 4 * KCAP * (sizeof(double) + sizeof(int)) + 256;
}

int launch_sim_topk(const float* Q, const float* Cm, int64_t nq, int64_t nc, int dim, int k, int64_t c_index_offset,
                    int64_t* out_idx, double* out_score, void* ws, size_t ws_bytes, hipStream_t st) {
    T2P_TRY(check_sizes_and_pointers("sim_topk", Q, Cm, nq, nc, k, out_idx, out_score));
    return sim_topk_impl(MASK_NONE, Q, Cm, nullptr, nullptr, kNoPrior, nq, nc, dim, k, c_index_offset, out_idx, out_score, ws, ws_bytes, st);
}

int launch_sim_topk_grouped(const float* Q, const float* Cm, const int32_t* query_group, const int32_t* cell_group, int64_t nq,
                            int64_t nc, int dim, int k, int64_t c_index_offset, int64_t* out_idx, double* out_score, void* ws,
                            size_t ws_bytes, hipStream_t st) {
    T2P_TRY(check_sizes_and_pointers("sim_topk_grouped", Q, Cm, nq, nc, k, out_idx, out_score));
    T2P_CHECK_ARG((query_group != nullptr || nq == 0) && (cell_group != nullptr || nc == 0), "sim_topk_grouped: NULL group array");
    // (query_group is NULL only with nq == 0, which launches nothing; with nc == 0 no kernel reads cell_group)
    return sim_topk_impl(MASK_GROUP, Q, Cm, query_group, cell_group, kNoPrior, nq, nc, dim, k, c_index_offset, out_idx, out_score, ws,
                         ws_bytes, st);
}

int launch_sim_topk_prior(const float* Q, const float* Cm, const double* query_xy, const double* query_radius, const double* cell_box,
                          const int32_t* query_group, const int32_t* cell_group, int64_t nq, int64_t nc, int dim, int k,
                          int64_t c_index_offset, int64_t* out_idx, double* out_score, void* ws, size_t ws_bytes, hipStream_t st) {
    T2P_TRY(check_sizes_and_pointers("sim_topk_prior", Q, Cm, nq, nc, k, out_idx, out_score));
    const int n_geo = (query_xy != nullptr) + (query_radius != nullptr) + (cell_box != nullptr);
    const int n_grp = (query_group != nullptr) + (cell_group != nullptr);
    T2P_CHECK_ARG(n_geo == 0 || n_geo == 3, "sim_topk_prior: query_xy, query_radius and cell_box go together (%d of 3 given)", n_geo);
    T2P_CHECK_ARG(n_grp == 0 || n_grp == 2, "sim_topk_prior: query_group and cell_group go together (1 of 2 given)");
    T2P_CHECK_ARG(n_geo + n_grp > 0, "sim_topk_prior: neither geometry nor groups given: call t2p_sim_topk");
    T2P_CHECK_ARG((((uintptr_t)cell_box) & 15) == 0, "sim_topk_prior: cell_box must be 16-byte aligned");
    return sim_topk_impl(MASK_PRIOR, Q, Cm, query_group, cell_group, PriorArgs{query_xy, query_radius, cell_box}, nq, nc, dim, k,
                         c_index_offset, out_idx, out_score, ws, ws_bytes, st);
}

}  // namespace t2p
