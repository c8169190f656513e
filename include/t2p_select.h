/*
 * t2p_select.h -- extension of the C ABI of libt2p_hip.so for the serving path (text2pos_amd.localize): the selection of
 * spatially distinct candidates from a ranked list of cells.
 *
 * Like include/t2p_serve.h an addition in a header of its own, with a version and a record of its own (T2P_SELECT_ABI_VERSION,
 * tests/golden/abi_select.json): t2p.h, t2p_serve.h, their versions and every binding made from them stay as they are.  Same
 * dialect of C (the parser of text2pos-cvpr2022_amd/_lib.py reads all three), same conventions: device pointers, caller-owned
 * buffers, work enqueued on `stream`, no allocation and no synchronisation inside, 0 / hipError_t / T2P_E_* return values with
 * the message in t2p_last_error().  The .hip file that defines an export below includes this header, so the C++ compiler
 * refuses a definition that differs from it.
 * Change a signature: bump T2P_SELECT_ABI_VERSION and regenerate tests/golden/abi_select.json.
 */
#ifndef T2P_SELECT_H
#define T2P_SELECT_H
#include "t2p.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2P_SELECT_ABI_VERSION 1

int t2p_select_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Distinct candidates: greedy non-overlap selection over the ordered list t2p_sim_topk / _grouped / _prior return.
 * On a map of overlapping cells (30 m cells on a 10 m stride: up to 24 neighbours share most of a cell's objects) the k
 * best-scoring cells of a query are a few places seen many times; this picks the k best cells no two of which overlap.
 *     pool_idx [nq][pool], pool_score [nq][pool]   a query's cells in the order of t2p_sim_topk (score descending, ties to the
 *                                                  lower index, masked cells at exactly -inf last), as index_offset + row
 *     cell_xy [n_cells][2] float64                 the position a cell is compared by (its centre)
 *     cell_group [n_cells] int32 or NULL           cells of different groups (scenes) never suppress each other
 * Two cells a, b CONFLICT iff fabs(xa - xb) < sep && fabs(ya - yb) < sep (float64, one subtraction each, comparisons only: a
 * NaN never conflicts) and, with cell_group, group[a] == group[b].  Per query: walk the pool from the front up to its first
 * entry at -inf; accept an entry iff it conflicts with no entry accepted so far; stop at k accepted.
 *     out_idx, out_score [nq][k]   the accepted entries in pool order, index and score bits as the pool holds them; the columns
 *                                  behind them hold the index of the query's first pool entry and -inf
 *     n_valid [nq]                 the number accepted
 *     exhausted [nq]               1 iff n_valid < k, the pool held no -inf entry and pool < n_cells: the walk was cut short by
 *                                  the pool, not by the database; wherever it is 0 the result is that of the walk over all
 *                                  n_cells ranked cells
 *   sep = 0: nothing conflicts, the first k pool entries bit for bit.  sep = +inf: one cell per group.
 *   A pool entry above -inf whose index lies outside [index_offset, index_offset + n_cells) is never read through: the query
 *   gets n_valid = -1, exhausted = 0 and every column -1 / -inf.  An entry at -inf is not looked up at all.
 *   One wavefront per query, float64, fixed order, no atomics: every output element is written once, the same bits every call.
 *   Profile name: topk_distinct.
 *   T2P_E_ARG, nothing launched: a NULL buffer (cell_group excepted); nq < 0 or >= 2^31; n_cells < 1; k < 1; k > pool;
 *   pool > T2P_SIM_TOPK_MAX_K; sep NaN or negative.  The message names the argument.
 * ---------------------------------------------------------------------------------------------------------- */
int t2p_topk_distinct(const int64_t* pool_idx, const double* pool_score, int64_t nq, int32_t pool, int64_t n_cells,
                      int64_t index_offset, const double* cell_xy, const int32_t* cell_group, double sep, int32_t k,
                      int64_t* out_idx, double* out_score, int32_t* n_valid, int32_t* exhausted, t2p_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2P_SELECT_H */
