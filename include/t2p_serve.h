/*
 * t2p_serve.h -- extension of the C ABI of libt2p_hip.so for the serving path (text2pos_amd.localize): retrieval restricted
 * to a prior position and / or to named groups of cells.
 *
 * include/t2p.h and its record tests/golden/abi.json state the ABI every earlier caller was built against; an addition goes into
 * a header of its own, with a version and a record of its own (this one: T2P_SERVE_ABI_VERSION, tests/golden/abi_serve.json),
 * so that t2p.h, T2P_ABI_VERSION and every binding made from them stay as they are.  Same dialect of C as t2p.h (the parser of
 * text2pos-cvpr2022_amd/_lib.py reads both), same conventions: device pointers, caller-owned buffers and workspace, work enqueued
 * on `stream`, 0 / hipError_t / T2P_E_* return values.  The .hip file that defines an export below includes this header, so the
 * C++ compiler refuses a definition that differs from it.
 * Change a signature: bump T2P_SERVE_ABI_VERSION and regenerate tests/golden/abi_serve.json.
 */
#ifndef T2P_SERVE_H
#define T2P_SERVE_H
#include "t2p.h"

#ifdef __cplusplus
extern "C" {
#endif

#define T2P_SERVE_ABI_VERSION 1

int t2p_serve_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Prior-restricted retrieval: t2p_sim_topk over the cells a query's prior allows.  A deployed localiser knows roughly where
 * it is (a last fix, a GPS reading, the drive it is on); applied after an unrestricted top-k such a prior returns nothing
 * whenever the k best cells of the whole database lie elsewhere, so the restriction sits in the ranking kernel.
 * The arguments of t2p_sim_topk plus
 *     query_xy [nq][2], query_radius [nq], cell_box [nc][4] = x0 y0 x1 y1      float64, all three or none (NULL)
 *     query_group [nq], cell_group [nc]                                        int32, both or none (NULL)
 * With s the score t2p_sim_topk gives the pair (q, c), bit for bit:
 *     geo(q, c) = no geometry given, or
 *                 dx = max(x0[c] - px[q], px[q] - x1[c], 0), dy likewise with y0, y1, py:
 *                 dx * dx + dy * dy <= r[q] * r[q]       float64, two products, one sum, in this order, never contracted
 *     grp(q, c) = no groups given, or query_group[q] < 0 (any group), or cell_group[c] == query_group[q]
 *     s'(q, c)  = geo && grp ? s : -inf                  a select on the finished score, never arithmetic
 *   The geometric test is the distance from the prior point to the cell's CLOSED square, not to its centre: r = 0 keeps the
 *   cells that contain the point (borders included), r = +inf keeps every cell.  A NaN in px, py, r or any of the four box
 *   members masks the pair (the maxima keep NaN and the final comparison fails on it), and so does a negative r.
 *   The result is the first k entries of the order on s' - score descending, ties and +-0.0 to the lower cell index: when fewer
 *   than k pairs of a query are allowed, its allowed cells come first, then masked cells at exactly -inf in ascending index.
 *   An allowed cell whose score is NaN is never retrieved; nc < k fills the tail with -1 / -inf.  index_offset shifts only the
 *   indices written out.  Nothing is read past cell_box[nc - 1] or cell_group[nc - 1].
 *   Same k range, widths, alignment rules, two selection paths (chosen by the same rule), workspace
 *   (t2p_sim_topk_workspace_bytes(nq, nc, k)) and profile names (sim_partial, topk_merge / sim_scores, topk_select) as
 *   t2p_sim_topk and t2p_sim_topk_grouped.
 *   T2P_E_ARG, nothing launched: a partial set of the three geometry pointers or of the two group pointers; both sets NULL
 *   (call t2p_sim_topk); cell_box not 16-byte aligned; and every refusal of t2p_sim_topk (k, dim, nc, workspace).
 * ---------------------------------------------------------------------------------------------------------- */
int t2p_sim_topk_prior(const float* queries, const float* cells, const double* query_xy, const double* query_radius,
                       const double* cell_box, const int32_t* query_group, const int32_t* cell_group, int64_t nq, int64_t nc,
                       int32_t dim, int32_t k, int64_t index_offset, int64_t* out_idx, double* out_score, void* workspace,
                       size_t workspace_bytes, t2p_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2P_SERVE_H */
