// Distinct candidates of the serving path: greedy non-overlap selection over a query's ranked cells (include/t2p_select.h).
//
// The reference has no such step: its evaluation takes the top_k best-scoring cells as they come (evaluation/pipeline.py:93-108).
// On 30 m cells with a 10 m stride these are a few places seen many times, so the serving path ranks a POOL of cells
// (t2p_sim_topk*, exactly ordered) and keeps the k best no two of which overlap.
//
// t2p_topk_distinct: a latency kernel.  One wavefront per query - the walk is sequential per query, parallel over queries.
//   pass 1  every pool entry above -inf has its index checked; one outside the table marks the query (n_valid = -1, every column
//           -1 / -inf) and nothing of it is looked up.
//   pass 2  the pool 64 entries at a time, one per lane, up to the first entry at -inf.  A lane tests its entry against the
//           accepted list of the earlier chunks (x, y, group in LDS: 20 B an entry, 20 KiB at k = 1,024; every lane reads the
//           same address, a broadcast).  The chunk is then resolved in lane order with ballots: the lowest surviving lane is
//           accepted - it appends itself to the list and writes its output column - and knocks out the later lanes it conflicts
//           with; repeat until no lane survives or k are accepted.
//   fill    the columns behind the accepted ones get the first pool entry's index and -inf.
// float64 comparisons of one subtraction each, a fixed order, no atomics; every output element is written exactly once.
#include "t2p_common.h"

#include <math.h>

#include "../../include/t2p_select.h"

namespace t2p {
namespace {

constexpr int kDistinctMaxPool = T2P_SIM_TOPK_MAX_K;     // the longest ordered list t2p_sim_topk returns

__global__ __launch_bounds__(64) void k_topk_distinct(const int64_t* __restrict__ pool_idx, const double* __restrict__ pool_score, int pool,
                                                      int64_t n_cells, int64_t index_offset, const double* __restrict__ cell_xy,
                                                      const int32_t* __restrict__ cell_group, double sep, int k,
                                                      int64_t* __restrict__ out_idx, double* __restrict__ out_score,
                                                      int32_t* __restrict__ n_valid, int32_t* __restrict__ exhausted) {
    extern __shared__ double lds_distinct[];             // ax [k] | ay [k] | ag [k] (int32)
    double* ax = lds_distinct;
    double* ay = ax + k;
    int* ag = (int*)(ay + k);
    const int lane = threadIdx.x;
    const int64_t q = blockIdx.x;
    const int64_t* pi = pool_idx + q * pool;
    const double* ps = pool_score + q * pool;
    int64_t* oi = out_idx + q * k;
    double* os = out_score + q * k;
    const double ninf = -__builtin_inf();

    bool bad = false;
    for (int e = lane; e < pool; e += 64) {
        const int64_t row = pi[e] - index_offset;
        if (ps[e] != ninf && (row < 0 || row >= n_cells)) bad = true;
    }
    if (__any(bad)) {                                    // the marked state: nothing was read through the pool's indices
        for (int c = lane; c < k; c += 64) {
            oi[c] = -1;
            os[c] = ninf;
        }
        if (lane == 0) {
            n_valid[q] = -1;
            exhausted[q] = 0;
        }
        return;
    }

    int acc = 0;
    bool saw_inf = false;
    for (int base = 0; base < pool && acc < k && !saw_inf; base += 64) {
        const int e = base + lane;
        int64_t idx = 0;
        double sc = ninf;
        if (e < pool) {
            idx = pi[e];
            sc = ps[e];
        }
        const unsigned long long m_inf = __ballot(e < pool && sc == ninf);
        bool alive = e < pool;
        if (m_inf) {                                     // the walk ends at the first -inf entry
            saw_inf = true;
            alive = alive && lane < (int)__builtin_ctzll(m_inf);
        }
        double x = 0.0, y = 0.0;
        int g = 0;
        if (alive) {                                     // (in range: pass 1 saw every entry above -inf)
            const int64_t row = idx - index_offset;
            x = cell_xy[2 * row];
            y = cell_xy[2 * row + 1];
            if (cell_group) g = cell_group[row];
        }
        for (int j = 0; j < acc; j++) {                  // against the cells accepted in earlier chunks
            if (fabs(x - ax[j]) < sep && fabs(y - ay[j]) < sep && g == ag[j]) alive = false;
        }
        unsigned long long m = __ballot(alive);
        while (m && acc < k) {
            const int l = (int)__builtin_ctzll(m);
            const double lx = __shfl(x, l, 64), ly = __shfl(y, l, 64);
            const int lg = __shfl(g, l, 64);
            if (lane == l) {
                ax[acc] = x;
                ay[acc] = y;
                ag[acc] = g;
                oi[acc] = idx;
                os[acc] = sc;
            }
            acc++;
            if (lane <= l || (fabs(x - lx) < sep && fabs(y - ly) < sep && g == lg)) alive = false;
            m = __ballot(alive);
        }
        __syncthreads();                                 // one wavefront: orders the list's writes before the next chunk's reads
    }

    const int64_t first = pi[0];
    for (int c = acc + lane; c < k; c += 64) {
        oi[c] = first;
        os[c] = ninf;
    }
    if (lane == 0) {
        n_valid[q] = acc;
        exhausted[q] = (acc < k && !saw_inf && (int64_t)pool < n_cells) ? 1 : 0;
    }
}

}  // namespace
}  // namespace t2p

using namespace t2p;

extern "C" {

int t2p_topk_distinct(const int64_t* pool_idx, const double* pool_score, int64_t nq, int32_t pool, int64_t n_cells,
                      int64_t index_offset, const double* cell_xy, const int32_t* cell_group, double sep, int32_t k,
                      int64_t* out_idx, double* out_score, int32_t* n_valid, int32_t* exhausted, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(pool_idx && pool_score, "topk_distinct: NULL pool_idx or pool_score");
    T2P_CHECK_ARG(cell_xy != nullptr, "topk_distinct: NULL cell_xy");
    T2P_CHECK_ARG(out_idx && out_score, "topk_distinct: NULL out_idx or out_score");
    T2P_CHECK_ARG(n_valid && exhausted, "topk_distinct: NULL n_valid or exhausted");
    T2P_CHECK_ARG(nq >= 0 && nq <= 0x7fffffff, "topk_distinct: need 0 <= nq < 2^31 (got %lld)", (long long)nq);
    T2P_CHECK_ARG(n_cells >= 1, "topk_distinct: need n_cells >= 1 (got %lld)", (long long)n_cells);
    T2P_CHECK_ARG(k >= 1, "topk_distinct: k=%d must be at least 1", k);
    T2P_CHECK_ARG(pool <= kDistinctMaxPool, "topk_distinct: pool=%d exceeds T2P_SIM_TOPK_MAX_K=%d, the longest ranked list", pool,
                  kDistinctMaxPool);
    T2P_CHECK_ARG(k <= pool, "topk_distinct: k=%d exceeds pool=%d", k, pool);
    T2P_CHECK_ARG(sep >= 0.0, "topk_distinct: sep=%g must be a number >= 0 (inf: one cell per group)", sep);   // (NaN fails the comparison)
    if (nq == 0) return 0;
    ProfScope ps_("topk_distinct", st);
    const size_t lds = (size_t)k * (2 * sizeof(double) + sizeof(int));
    hipLaunchKernelGGL(k_topk_distinct, dim3((unsigned)nq), dim3(64), lds, st, pool_idx, pool_score, (int)pool, n_cells, index_offset,
                       cell_xy, cell_group, sep, (int)k, out_idx, out_score, n_valid, exhausted);
    T2P_CHECK_LAUNCH("topk_distinct");
    return 0;
}

}  // extern "C"
