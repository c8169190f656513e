/*
 * t2p.h -- C ABI of libt2p_hip.so: the MI355X (gfx950) implementation of the Text2Pos coarse
 * cell-retrieval forward path.
 *
 * The reference (mako443/Text2Pos-CVPR2022) is pure Python and has no FFI/plugin interface; its boundary for
 * this path is the Python class models/cell_retrieval.py::CellRetrievalNetwork plus the retrieval loop of
 * training/coarse.py::eval_epoch.  The entry points below are what a ctypes binding of that class calls
 * (INTEGRATION.md shows the stub); each one names the reference interface it replaces.
 *
 * This file is the ONE statement of the ABI.  The C++ compiler holds every definition to it (each .hip that defines an export
 * includes it) and the Python binding is generated from it at import (text2pos-cvpr2022_amd/_lib.py parses the prototypes, the
 * typedef structs and the integer #define T2P_* below; tests/test_abi_host.py checks the result against the host C compiler).
 * So it stays within the C that parser reads: scalar types int, int32_t, int64_t, uint32_t, size_t, float; pointers to those, to
 * void, char, double, uint8_t, uint16_t, uint64_t and to the structs; members `T name`, `T name[n]`, `T a, b` and `T *a, *b`; no
 * function pointers, bit-fields, nested structs or array parameters.  Anything else fails the import, naming the declaration.
 * Change a signature or a struct: bump T2P_ABI_VERSION and regenerate tests/golden/abi.json.
 * Additions live in extension headers with a version and a record of their own: include/t2p_serve.h (the serving path's
 * prior-restricted retrieval).
 *
 * Conventions
 *   - Every pointer is a DEVICE pointer (HBM) unless its name ends in _host.  Buffers are owned by the caller;
 *     the library never allocates or frees device memory and keeps no global mutable state besides the
 *     thread-local error string.  Scratch space is a caller-provided workspace, sized by the *_workspace_bytes
 *     functions.
 *   - Every call enqueues work on `stream` (a hipStream_t; NULL = the default stream) and returns without
 *     synchronising.  Re-entrant; one process per GPU for multi-GPU use.
 *   - Return value: 0 = success; > 0 = hipError_t of a failed launch; < 0 = T2P_E_* argument / workspace /
 *     unsupported-configuration error.  t2p_last_error() returns the message of the calling thread's last failure.
 *   - All floating-point tensors are fp32 row-major; weights are "k-major" ([in_features][out_features], i.e. the
 *     transpose of torch.nn.Linear.weight) with eval-mode BatchNorm folded in by the host
 *     (models/modules.py:21-29: Linear -> BatchNorm1d -> ReLU).
 */
#ifndef T2P_H
#define T2P_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2P_ABI_VERSION 33
#define T2P_DEFAULT_CHUNK_OBJECTS 65000 /* t2p_cell_config.chunk_objects == 0 */
#define T2P_MAX_CHUNK_OBJECTS 65535     /* 32-bit table offsets / 16-bit local indices: chunk_objects and the largest single
                                           cell may not exceed it (T2P_E_ARG otherwise).  The caller-provided workspace holds
                                           one chunk: ~0.6 MB per object, i.e. ~38 GB at the default chunk for a batch that
                                           fills it (t2p_encode_cells_workspace_bytes gives the exact figure; a second
                                           stream's call needs its own workspace) */
#define T2P_TUNING_MASK 0xD              /* t2p_cell_config.tuning: the bits that select a built plan */
#define T2P_E_ARG (-1)
#define T2P_E_WORKSPACE (-2)
#define T2P_E_UNSUPPORTED (-3)

typedef void* t2p_stream_t; /* hipStream_t */

int t2p_abi_version(void);
const char* t2p_last_error(void);

/* ------------------------------------------------------------------------------------------------------------
 * Cell branch: CellRetrievalNetwork.encode_objects  (models/cell_retrieval.py:77-107), i.e.
 * ObjectEncoder.forward (models/object_encoder.py:61-142) -> PointNet2.forward
 * (models/pointcloud/pointnet2.py:80-100) -> DynamicEdgeConv + global_max_pool + lin + F.normalize.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct t2p_cell_weights {
    /* PointNet2.sa{1,2,3}.point_conv.local_nn (models/pointcloud/pointnet2.py:57-59).  Layer 1 is applied to
     * [x_j | pos_j - pos_i]; sa_w1[l] is [Kpad_l][H_l] with rows = [x features (3,64,128) | pos (3) | zero pad]
     * (Kpad = 6, 96, 160; H = 32, 128, 256); sa_w2[l] is [H_l][C_l] (C = 64, 128, 256). */
    const float* sa_w1[3];
    const float* sa_b1[3];
    const float* sa_w2[3];
    const float* sa_b2[3];
    /* PointNet2.ga.mlp (pointnet2.py:60): [288][512] (rows = [x 256 | pos 3 | pad 29]) and [512][1024] */
    const float* ga_w1;
    const float* ga_b1;
    const float* ga_w2;
    const float* ga_b2;
    /* PointNet2.lin1 / lin2 (pointnet2.py:62-63,89-90): [1024][512], [512][256] */
    const float* lin1_w;
    const float* lin1_b;
    const float* lin2_w;
    const float* lin2_b;
    /* ObjectEncoder.mlp_pointnet (object_encoder.py:53-58,98): [dim_f][D], dim_f = 1024/512/256 */
    const float* pn_w;
    const float* pn_b;
    /* ObjectEncoder.color_encoder / pos_encoder (object_encoder.py:40-41): [3][64], [64][D] */
    const float* col_w1;
    const float* col_b1;
    const float* col_w2;
    const float* col_b2;
    const float* pos_w1;
    const float* pos_b1;
    const float* pos_w2;
    const float* pos_b2;
    /* ObjectEncoder.mlp_merge (object_encoder.py:59,137-138): [n_features*D][D]; unused when n_features == 1 */
    const float* merge_w;
    const float* merge_b;
    /* CellRetrievalNetwork.graph1.nn (cell_retrieval.py:46-48).  Layer 1 on [x_i | x_j - x_i] is split as
     * P_i + Q_j: g_wp = (W1a - W1b)^T [D][D] with bias g_bp, g_wq = W1b^T [D][D]; layer 2 g_w2 [D][D], g_b2. */
    const float* g_wp;
    const float* g_bp;
    const float* g_wq;
    const float* g_w2;
    const float* g_b2;
    /* CellRetrievalNetwork.lin (cell_retrieval.py:49): [D][D] x 2 */
    const float* lin_w1;
    const float* lin_b1;
    const float* lin_w2;
    const float* lin_b2;
    /* Optional "f16x3" split-precision images of the MFMA-heavy layer-2 weights (used when cfg->precision == 1):
     * every weight is split w = hi + lo/2048 with hi, lo in fp16, stored in MFMA B-operand register order
     * uint16 [2 planes hi,lo][N/32 column tiles][K/16 steps][2 lane halves][32 lanes][8]  holding
     * w[k = half*K/2 + 8*step + e][n = 32*tile + lane]  (packing.py::pack_f16x3). */
    const void* sa_w2_x3[3];
    const void* ga_w2_x3;
    /* The SA layer-2 images (sa_w2_x3) use the scaled single-accumulator form instead: w' = s w with s = sa_w2_scale[l]
     * a power of two (so that |w'| uses fp16's range), hi = fp16(w'), lo = fp16(w' - hi) (no 2048 factor: MFMA honours
     * fp16 denormals), the three products hi.hi + hi.lo + lo.hi share ONE fp32 accumulator.  The kernels of the 256-point
     * level shapes (k_sa_points, k_sa_rows, k_sa3) start it at 0, take the maximum over a centroid's rows and add
     * sa_b2_x3[l] = s b2 once, at the drain: relu(max + s b2) / s; k_sa_stream (every other size) starts it at s b2 and
     * drains relu(max) / s.  Both divide by s (a power of two: exact) when they drain an object
     * (packing.py::pack_f16x3_scaled; tests/trunk_ref.py derives one bound for both). */
    const float* sa_b2_x3[3];
    float sa_w2_scale[3];
    /* Scaled split images of the dense layers behind the trunk, for the LDS-tiled f16x3 GEMM
     * (packing.py::pack_gemm_x3): uint16 [2 planes hi,lo][N][K rounded up to 32] holding s w[k][n], lo = s w - hi. */
    const void* lin1_x3;
    const void* lin2_x3;
    const void* merge_x3;
    const void* pn_x3;   /* mlp_pointnet */
    const void* g_wp_x3; /* DynamicEdgeConv layer-1 tables P, Q */
    const void* g_wq_x3;
    float lin1_scale, lin2_scale, merge_scale, pn_scale, g_wp_scale, g_wq_scale;
    /* pack_f16x3 images of the layer-1 matrices that read SA output rows: of their first C + 16 rows only
     * (K = 80 / 144 for sa_w1[1], sa_w1[2]; 272 for ga_w1: [features C | xyz | zero rows]; the fp32 matrices keep C + 32
     * rows).  Levels 1 and 2 only (level 0 has K = 6 and runs on the VALU); [0] is ignored */
    const void* sa_w1_x3[3];
    const void* ga_w1_x3;
    /* ObjectEncoder.class_embedding / color_embedding (object_encoder.py:31-38), used by the --class_embed /
     * --color_embed ablations only: [n_classes + 1][D], [8][D] */
    const float* class_embedding;
    const float* color_embedding;
    /* fp16-range guard (cfg->overflow_flag): bound of GA layer 1's output from its input's magnitude,
     * |gh| <= ga_w1_l1 * max(|F_3|, 1) + ga_b1_absmax with ga_w1_l1 = max over output columns of sum_k |ga_w1[k][col]|
     * and ga_b1_absmax = max |ga_b1| (the high side; the kernel's exact maximum of what it stores also serves the low side). */
    float ga_w1_l1;
    float ga_b1_absmax;
    /* the same kind of bound for the layer-1 tables that depend on the inputs only: sa_wp_l1[l] = max over columns of
     * |W1p_l[0][c]| + |W1p_l[1][c]| + |W1p_l[2][c]| (position rows of SA level l's first layer: |B_l| <= sa_wp_l1[l] max|xyz|),
     * sa_a1_l1 = max over columns of sum_k |sa_w1[0][k][c]| and sa_b1_absmax = max |sa_b1[0]| (|A_1| <= sa_a1_l1 max|input|
     * + sa_b1_absmax). */
    float sa_wp_l1[3];
    float sa_a1_l1;
    float sa_b1_absmax;
    /* optional f16x3 image (packing.py::pack_f16x3 layout, as ga_w2_x3) of g_w2, DynamicEdgeConv's second layer */
    const void* g_w2_x3;
} t2p_cell_weights;

typedef struct t2p_cell_config {
    int32_t n_pts;             /* points per object after T.FixedPoints (args.pointnet_numpoints, training/args.py:53): 8 to 256
                                  (default 256); outside that range T2P_E_UNSUPPORTED */
    int32_t embed_dim;         /* D; 256 */
    int32_t pointnet_features; /* 0 | 1 | 2 (training/args.py:58) */
    int32_t use_class;         /* "class" / "color" / "position" in args.use_features (training/args.py:21) */
    int32_t use_color;
    int32_t use_position;
    int32_t self_loops;        /* 1 = PyG PointConv(add_self_loops=True) semantics (upstream default), 0 = none */
    int32_t knn_k;             /* DynamicEdgeConv k (cell_retrieval.py:47); 8 */
    int32_t variation;         /* args.variation (cell_retrieval.py:45-54): 0 = max, 1 = mean aggregation + mean pool */
    float radius[3];           /* SA ball radii (pointnet2.py:57-59); 0.2, 0.3, 0.4 */
    int32_t chunk_objects;     /* objects processed per internal chunk (whole cells); 0 = T2P_DEFAULT_CHUNK_OBJECTS */
    int32_t precision;         /* 0 = fp32 MFMA (exact fp32 fma chains); 1 = f16x3 split-precision MFMA with fp32
                                  accumulation (hi.hi + hi.lo + lo.hi), same 1e-4 parity bar (for every cell whose DynamicEdgeConv
                                  kNN graph has no near-tie: DESIGN.md section 2), 5.3x the MFMA rate */
    /* ground-truth embedding ablations (training/args.py:60-61, object_encoder.py:74-84,103-120): when class_embed
     * is set the PointNet++ is skipped and the "class" feature is F.normalize(class_embedding[class_idx]); when
     * color_embed is set the "color" feature is F.normalize(color_embedding[color_idx]).  Index arrays are DEVICE
     * int32 [n_obj] (NULL when the flag is 0). */
    int32_t class_embed;
    int32_t color_embed;
    const int32_t* class_idx;
    const int32_t* color_idx;
    /* 1 = stop after ObjectEncoder.forward (models/object_encoder.py:61-142): no cell head; `out` is ignored (may be
     * NULL), the [n_obj][D] result is returned through trace->obj_emb (required).  This is the entry the fine stage
     * uses (SuperGlueMatch.forward, models/superglue_matcher.py:101-103); embed_dim may then be any multiple of 64
     * up to 512 (the fine stage trains with 128, README.md:62). */
    int32_t objects_only;
    /* fp16-range guard of the f16x3 path (precision == 1): the split-precision kernels convert fp32 activations to fp16
     * (round to nearest: a magnitude past 65504 would become inf).  When non-NULL, this DEVICE word receives a
     * sticky OR of a non-zero code whenever a conversion site of the call may have left fp16's range (bits 0-2: SA level
     * 1-3 edge inputs, judged by max|A_l| + max|B_l|; bit 3: SA output rows split by the dense table kernels; bit 4: GA
     * hidden planes, judged by a norm bound and by their exact maximum; bit 5: rows of the LDS-tiled GEMMs and the kNN edge
     * rows; bit 6: a NaN among the input points / colours - the float-max aggregation of the f16x3 kernels would drop it where
     * the reference's scatter-max propagates it - or a NaN / infinity in an object's embedding row as the cell head receives it:
     * every kNN distance to that object is NaN, so it gets no neighbour and no edge row, and in BOTH precisions the output row
     * of its cell is NaN (never a finite row computed from the cell's other objects);
     * bit 7: LOW side - the largest hidden activation or the largest output of an
     * SA level, the largest GA hidden activation, PointNet2 feature (features0 / 1 / 2, each on its own) or kNN edge row is
     * below 2^-7, where the fp16 pieces keep an absolute 2^-25 instead of a relative 2^-22 and a later BatchNorm that rescales
     * would expose the loss).  The tests are conservative: they may
     * fire for a checkpoint that would just have fitted, never the other way round.  The caller clears it, reads it after the stream has drained, and must
     * not trust the call's output when it is set (the Python host raises or re-runs with precision = 0).  NULL: no check. */
    int32_t* overflow_flag;
    /* A/B switch between equivalent execution plans (0 = the default plan):
     *   bit 0: keep the edge rows of repeated points in SA level 1's row lists (default: t2p_dedup_rows drops them; every
     *          output bit is the same either way)
     *   bit 2: keep the FULL row lists of SA levels 2 and 3: the edge rows of repeated centroids at SA level 2 (default: the
     *          centroids FPS repeats once an object's distinct positions are used up share one copy of their rows, see
     *          t2p_group_rows_shared) and, at both levels, the rows whose source is a repeated dense point (default with
     *          self_loops = 0 in the plan of bit 3 clear: they leave the lists, see t2p_group_rows_pruned); every output bit
     *          is the same either way
     *   bit 3: SA level 1's rows listed by the scan kernel and pruned in place by t2p_dedup_rows, as before (default, at 256
     *          points per object and with bit 0 clear: the scan publishes each centroid's hit mask and one builder kernel
     *          writes the pruned list once, see t2p_group_rows_built; the list is the same bit for bit)
     * Bits outside T2P_TUNING_MASK are refused (T2P_E_ARG).  (Rounds 1-3 kept alternative SA kernels behind further bits; the
     * measured record is docs/notebook.md, the code is in the git history.) */
    int32_t tuning;
} t2p_cell_config;

/* Optional stage outputs for parity tests (any member may be NULL).  Layouts:
 *   fps_idx[l] uint8 [n_obj][n_cent_l]      local FPS indices into level l's dense ordering
 *   nbr[l]     uint8 [n_obj][n_cent_l][32]  ball-query neighbours (first cnt valid), cnt[l] uint8 [n_obj][n_cent_l]
 *   sa_out[l]  fp32  [n_obj*n_cent_l][C_l+32] rows = [features C_l | centroid xyz | 0 | 28 columns the call leaves untouched]
 *   features0  fp32  [n_obj][1024]; features1 [n_obj][512]; features2 [n_obj][256]; obj_emb [n_obj][D] (ObjectEncoder output)
 *   knn_idx    int32 [n_obj][knn_k] global object rows (-1 = none)
 * The cell head's stages (D = cfg->embed_dim, the padded width the kernels run at; not written by objects_only calls):
 *   head_in    fp32  [n_obj][D]   F.normalize(obj_emb), the rows the P / Q products and the kNN read
 *   head_edge  fp32  [n_obj][D]   DynamicEdgeConv's output rows (max or mean over each object's neighbours)
 *   head_pool  fp32  [n_cells][D] global max / mean pool over each cell's rows
 *   head_l1    fp32  [n_cells][D] first layer of CellRetrievalNetwork.lin; head_l2: the second, which the final F.normalize reads */
typedef struct t2p_cell_trace {
    uint8_t* fps_idx[3];
    uint8_t* nbr[3];
    uint8_t* cnt[3];
    float* sa_out[3];
    float* features0;
    float* features2;
    float* obj_emb;
    int32_t* knn_idx;
    float* features1;
    float* head_in;
    float* head_edge;
    float* head_pool;
    float* head_l1;
    float* head_l2;
} t2p_cell_trace;

size_t t2p_encode_cells_workspace_bytes(int64_t n_obj, int64_t n_cells, const t2p_cell_config* cfg);

/* xyz, rgb [n_obj][n_pts][3] (PyG batch .pos / .x of dataloading/kitti360pose/utils.py:99-109, objects of all
 * cells concatenated); center, mean_rgb [n_obj][3] (Object3d.get_center / get_color_rgb,
 * datapreparation/kitti360pose/imports.py:28-41); cell_ptr [n_cells+1] int32 CSR over objects, given both in host
 * memory (chunk planning) and in device memory.  out [n_cells][D], L2-normalised rows. */
int t2p_encode_cells(const float* xyz, const float* rgb, const float* center, const float* mean_rgb,
                     const int32_t* cell_ptr_host, const int32_t* cell_ptr, int64_t n_obj, int64_t n_cells,
                     const t2p_cell_weights* w, const t2p_cell_config* cfg, float* out, const t2p_cell_trace* trace,
                     void* workspace, size_t workspace_bytes, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * PointNet++ as a classifier of its own: PointNet2.forward (models/pointcloud/pointnet2.py:80-100) in eval mode, the model
 * the reference pre-trains in training/pointcloud/pointnet2.py before the coarse stage loads it (models/object_encoder.py:46).
 * The trunk is the cell encoder's (same kernels, same folded weights: the sa_*, ga_*, lin1_*, lin2_* members of
 * t2p_cell_weights and their *_x3 images and guard norms; every other member is ignored), stopped behind lin2.  The reference
 * hands a DataLoader batch to the model as ONE PyG batch, so the whole call is one cell of n_obj objects: PointConv's self-loop
 * rewrite aliases dense row i of the BATCH onto centroid row i of the batch.  n_obj <= T2P_MAX_CHUNK_OBJECTS (T2P_E_ARG).
 * Of cfg only n_pts, self_loops, radius, precision, overflow_flag and tuning are read (the guard word covers the stages that
 * run: bits 0-4, 6, 7 and bit 5 for features0 / features1 as lin1 / lin2 split them).
 * head_w [256][n_classes + n_colors] k-major (class_classifier.weight^T | color_classifier.weight^T side by side), head_b
 * [n_classes + n_colors]; n_classes, n_colors in [1, 64] (T2P_E_UNSUPPORTED otherwise).  head_w == NULL: trunk only.
 * Outputs (each may be NULL): features0 [n_obj][1024], features1 [n_obj][512], features2 [n_obj][256],
 * class_pred [n_obj][n_classes], color_pred [n_obj][n_colors] (pointnet2.py:91-92; fp32, bias + 256 fma in ascending k).
 * ---------------------------------------------------------------------------------------------------------- */
size_t t2p_pointnet2_workspace_bytes(int64_t n_obj, const t2p_cell_config* cfg);
int t2p_pointnet2_forward(const float* xyz, const float* rgb, int64_t n_obj, const t2p_cell_weights* w, const t2p_cell_config* cfg,
                          const float* head_w, const float* head_b, int32_t n_classes, int32_t n_colors, float* features0,
                          float* features1, float* features2, float* class_pred, float* color_pred, void* workspace,
                          size_t workspace_bytes, t2p_stream_t stream);
/* The two heads alone (csrc/classify.hip): features2 [n][256] -> class_pred [n][n_classes], color_pred [n][n_colors]. */
int t2p_classifier_heads(const float* features2, const float* head_w, const float* head_b, int64_t n, int32_t n_classes,
                         int32_t n_colors, float* class_pred, float* color_pred, t2p_stream_t stream);
/* nn.CrossEntropyLoss()(class_pred, batch.y) with its gradient and the accuracy count of the pre-training loop
 * (training/pointcloud/pointnet2.py:37, :42, :134) in one launch.  logits [n][n_classes] with row pitch ld_logits (floats),
 * labels int32 [n].  row_loss [n] = logsumexp(row) - row[label] (loss = sum(row_loss) / n, summed by the caller in a fixed
 * order); d_logits [n][n_classes] (row pitch ld_d) = (softmax(row) - onehot(label)) / n; correct int32 [n] =
 * (argmax(row) == label), ties to the lower index as torch.argmax.  The row maximum is subtracted before exp; reductions are
 * cross-lane butterflies, no atomics: deterministic.  A label outside [0, n_classes) gives NaN in row_loss and in the row of
 * d_logits and correct = 0; nothing is read or written through it. */
int t2p_softmax_xent(const float* logits, int32_t ld_logits, const int32_t* labels, int64_t n, int32_t n_classes, float* row_loss,
                     float* d_logits, int32_t ld_d, int32_t* correct, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Input packing on the device: replaces the per-object host work of
 * dataloading/kitti360pose/utils.py:89-110 (Data -> T.FixedPoints -> T.NormalizeScale -> Batch) and the per-object
 * NumPy means of models/object_encoder.py:121-131 (Object3d.get_color_rgb / get_center).
 * raw_xyz, raw_rgb [n_points_total][3] fp32: the raw points of all objects back to back; obj_ptr [n_obj+1] int32 CSR;
 * sample_idx [n_obj][n_pts] int32: per-object LOCAL indices drawn with replacement by the host's seeded generator
 * (T.FixedPoints is random even at evaluation time, evaluation/pipeline.py:290-293 -- the draw stays on the host so that
 * runs are reproducible).  rot_cos_sin: NULL, or [n_obj][2] fp32 (cos, sin) of one angle per object = the training
 * transform's T.RandomRotate(120, axis=2) between FixedPoints and NormalizeScale (training/coarse.py:192-198):
 * pos <- pos @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] (PyG 1.7 - 2.0 LinearTransformation; later releases multiply by the
 * transpose, i.e. the opposite angle -- the same distribution for a symmetric range); the angle is drawn on the host.
 * Outputs are exactly the inputs of t2p_encode_cells.
 * ---------------------------------------------------------------------------------------------------------- */
int t2p_pack_objects(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* sample_idx,
                     const float* rot_cos_sin, int64_t n_obj, int32_t n_pts, float* xyz, float* rgb, float* center, float* mean_rgb,
                     t2p_stream_t stream);

/* The dataloader of a scene that is RESIDENT in HBM - what evaluation/pipeline.py:282-342 builds per batch on the host
 * (Kitti360CoarseDatasetMulti / Kitti360TopKDataset -> batch_object_points, dataloading/kitti360pose/utils.py:89-110,
 * dataloading/kitti360pose/eval.py:117-189) for every cell of the database and again for every (query, candidate cell)
 * pair of the fine stage.  The raw points of all objects of the scene are uploaded once (raw_xyz, raw_rgb [n_points][3]
 * fp32, obj_ptr [n_scene_obj + 1] int32 CSR) together with the per-object means scene_center / scene_color
 * [n_scene_obj][3] fp32 (Object3d.get_center() / get_color_rgb(): the reference's float64 NumPy means, cast); a call then
 * packs any list of them: output slot s takes scene object obj_id[s] (int32 [n_out]; the same object may fill many slots:
 * a cell retrieved for several queries, the padding object of dataloading/kitti360pose/eval.py:147-149).
 * T.FixedPoints(n_pts) is counter-based: point p of slot s is raw point
 *       ((mix64(key[s] ^ p * 0xD6E8FEB86659FD93) >> 32) * m) >> 32      of the object's m points, with
 *       mix64(x): x += 0x9E3779B97F4A7C15; x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB;
 *                 x ^ x >> 31   (64-bit wrap-around),
 * key [n_out] uint64 chosen by the host (pipeline.PerCellTransform: a hash of (seed, global cell index, slot in the cell),
 * so a cell's sample does not depend on the rank, batch or stream that packs it).  T.NormalizeScale follows, bit for bit
 * as ATen computes it on the host (csrc/small_kernels.hip).  n_pts <= 1024.
 * Outputs: xyz, rgb [n_out][n_pts][3], center, mean_rgb [n_out][3] = the inputs of t2p_encode_cells; rgb, center, mean_rgb
 * and sample_idx_out (int32 [n_out][n_pts]: the draws, for checking) may each be NULL (not written). */
int t2p_pack_scene_objects(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* obj_id,
                           const uint64_t* key, const float* scene_center, const float* scene_color, int64_t n_out, int32_t n_pts,
                           float* xyz, float* rgb, float* center, float* mean_rgb, int32_t* sample_idx_out, t2p_stream_t stream);

/* The same for TRAINING batches: the augmentation of Kitti360CoarseDataset.__getitem__ (dataloading/kitti360pose/cells.py:79-91)
 * on the resident scene - the horizontal / vertical flip of the cell (flip_pose_in_cell, dataloading/kitti360pose/utils.py:13-86)
 * and the T.RandomRotate(120, axis=2) of the training transform (training/coarse.py:192-198) - in the reference's order:
 *   flip (on the RAW object) -> T.FixedPoints -> rotation -> T.NormalizeScale.
 * flip: NULL, or uint8 [n_out]: bit 0 = the slot's object is mirrored in x, bit 1 = in y (only the two low bits are read).  The
 *   reference mirrors the raw float64 points, `obj.xyz[:, a] = 1 - obj.xyz[:, a]`, and casts to fp32 afterwards; 1.f - x32 is not that
 *   value, so the scene carries a second image of the two columns, raw_mirror_xy [n_points][2] = float32(1.0 - xyz64[:, 0:2]), and
 *   scene_center_mirror_xy [n_scene_obj][2] = float32 of NumPy's float64 mean over the mirrored column (get_center() of the flipped
 *   object).  A slot with bit a set reads coordinate a of its points from raw_mirror_xy and coordinate a of its centre from
 *   scene_center_mirror_xy; z, the colours and mean_rgb are the plain call's.  The kernel selects pointers and computes nothing
 *   here: exact.  A flip does not change an object's point count, so a slot draws the same indices flipped or not.
 * rot_cos_sin: NULL, or [n_out][2] fp32 (cos, sin) per slot, applied as in t2p_pack_objects between the gather and
 *   NormalizeScale: xr = x*c + y*(-s), yr = x*s + y*c.
 * flip = NULL and rot_cos_sin = NULL give t2p_pack_scene_objects' outputs bit for bit.  Refused (T2P_E_ARG): flip without
 * raw_mirror_xy; flip with center wanted and no scene_center_mirror_xy; n_pts > 1024; NULL required arguments.  Outputs and their
 * NULL rules are the plain call's. */
int t2p_pack_scene_objects_aug(const float* raw_xyz, const float* raw_rgb, const float* raw_mirror_xy, const int32_t* obj_ptr,
                               const int32_t* obj_id, const uint64_t* key, const uint8_t* flip, const float* rot_cos_sin,
                               const float* scene_center, const float* scene_center_mirror_xy, const float* scene_color,
                               int64_t n_out, int32_t n_pts, float* xyz, float* rgb, float* center, float* mean_rgb,
                               int32_t* sample_idx_out, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fine stage: hint <-> object matching + offset regression.
 * Replaces SuperGlue.forward models/superglue.py:239-330 (GNN of ["self","cross"] x num_layers AttentionalPropagation
 * layers, final_proj, scores / sqrt(D), log-space optimal transport with dustbin, mutual nearest neighbours + 0.2
 * threshold) and mlp_offsets (models/superglue_matcher.py:116).  Inputs are the L2-normalised object / hint encodings
 * of SuperGlueMatch.forward (:94-103), tokens-major: desc0 [B][n_obj][D], desc1 [B][n_hints][D] fp32.
 * All matrices k-major [in][out], BatchNorm (eval) folded into mlp.0: per GNN layer l
 *   wqkv [D][3D] = attn.proj.{0,1,2} side by side (q | k | v), bqkv [3D];  wm [D][D], bm [D] = attn.merge;
 *   w1 [2D][2D], b1 [2D] = mlp.0 + mlp.1 (BN);  w2 [2D][D], b2 [D] = mlp.3;   cross[l] (HOST array) 0 = self, 1 = cross.
 * Outputs: P [B][n_obj+1][n_hints+1] fp32; matches0 [B][n_obj], matches1 [B][n_hints] int64 (-1 = no match);
 * matching_scores0/1 fp32; offsets [B][n_hints][2] fp32.  The optimal-transport part (scores, the log-Sinkhorn iterations, the
 * log couplings the matches are read from) is float64 inside and rounds P and the scores once, as t2p_match_head does.
 * With GNN layers a sample's (n_obj + n_hints)(3 D + 4) + 4 (n_obj + n_hints) max(n_obj, n_hints) floats must fit 160 KiB of
 * LDS (T2P_E_UNSUPPORTED otherwise, before any launch); without a layer every 1 <= n_obj, n_hints <= 63 runs.
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct t2p_match_weights {
    int32_t n_layers;
    const int32_t* cross;
    const float *wqkv, *bqkv, *wm, *bm, *w1, *b1, *w2, *b2; /* [n_layers][...] device */
    const float *wf, *bf;                                   /* final_proj [D][D], [D] */
    float bin_score;
    const float *wo1, *bo1, *wo2, *bo2;                     /* mlp_offsets: [D][D/2], [D/2], [D/2][2], [2] */
    /* Optional scaled split images (packing.py::pack_gemm_x3, one [2][N][Kp] image per layer, layers back to back) of
     * the GNN / final_proj matrices for the f16x3 GEMM; NULL = fp32 MFMA.  One power-of-two scale per matrix family. */
    const void *wqkv_x3, *wm_x3, *w1_x3, *w2_x3, *wf_x3;
    float scale_qkv, scale_m, scale_1, scale_2, scale_f;
} t2p_match_weights;

size_t t2p_match_workspace_bytes(int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim);

int t2p_match(const float* desc0, const float* desc1, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
              const t2p_match_weights* w, int32_t sinkhorn_iters, float match_threshold, float* P, int64_t* matches0,
              int64_t* matches1, float* mscores0, float* mscores1, float* offsets, void* workspace,
              size_t workspace_bytes, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Fine stage in train() mode (csrc/match_train.hip): what SuperGlueMatch.forward needs besides row GEMMs and batch-statistics
 * BatchNorm, and the two loss values of training/fine.py:56-59.  BatchNorm takes its statistics over all object tokens of the
 * batch, then over all hint tokens (models/superglue.py:119-129 called twice per layer, :139-146), so the token rows are
 * SET-major here: rows [0, B n_obj) the object tokens (row b n_obj + i), rows [B n_obj, B (n_obj + n_hints)) the hint tokens
 * (row B n_obj + b n_hints + j).  1 <= n_obj, n_hints <= 63 (T2P_E_ARG otherwise), embed_dim in {64, 128, 256}
 * (T2P_E_UNSUPPORTED otherwise); refused before any launch.  fp32 in and out; deterministic (no atomics).
 * ---------------------------------------------------------------------------------------------------------- */
/* MultiHeadedAttention of one GNN layer without its projections (models/superglue.py:90-116: attention, the head split of
 * :107-109 - channel c belongs to head c % 4 - and the merge of the heads' outputs into one row; the Conv1d projections and
 * `merge` are row GEMMs of the caller).  qkv [B (n_obj + n_hints)][3 D]: q | k | v of every token; cross = 0: a token attends to
 * its own set, 1: to the other set of its sample (models/superglue.py:139-143).  msg [B (n_obj + n_hints)][D]. */
int t2p_match_attention(const float* qkv, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim, int32_t cross,
                        float* msg, t2p_stream_t stream);
/* The optimal-transport head of SuperGlue.forward (models/superglue.py:283-322 with log_optimal_transport :149-177) on
 * mdesc [B (n_obj + n_hints)][D] = final_proj of the token rows: scores m0 m1^T / sqrt(D), dustbin row and column bin_score,
 * sinkhorn_iters log-space iterations (carried in float64), P = exp(Z) [B][n_obj + 1][n_hints + 1], mutual nearest neighbours
 * of the inner block with match_threshold: matches0 [B][n_obj], matches1 [B][n_hints] int64 (-1 = none), matching scores fp32.
 * The offset MLP (models/superglue_matcher.py:116) is two row GEMMs of the caller. */
int t2p_match_head(const float* mdesc, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim, float bin_score,
                   int32_t sinkhorn_iters, float match_threshold, float* P, int64_t* matches0, int64_t* matches1, float* mscores0,
                   float* mscores1, t2p_stream_t stream);
/* MatchingLoss.forward (training/losses.py:20-30) in one launch.  P [B][n_obj + 1][n_hints + 1]; idx int32 [n_entries][2]: the
 * (object, hint) pairs of all samples back to back, entry_ptr int32 [B + 1] their CSR over the samples.
 * sample_loss [B] = mean over the sample's entries of -log P[b, i, j]; loss [1] = mean of sample_loss; terms accumulated in
 * float64 in a fixed order.  An entry outside [0, n_obj] x [0, n_hints], an empty sample or a row pointer outside
 * [0, n_entries] gives NaN in that sample's loss (and so in loss); nothing is read through it. */
int t2p_matching_loss(const float* P, int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* idx, const int32_t* entry_ptr,
                      int64_t n_entries, float* sample_loss, float* loss, t2p_stream_t stream);
/* nn.MSELoss() (mean reduction; training/fine.py:36, :57-59) of a, b [n] fp32 -> loss [1]; float64 accumulation in a fixed order. */
int t2p_mse_loss(const float* a, const float* b, int64_t n, float* loss, t2p_stream_t stream);

/* Backward of the four entry points above, for training the fine stage (training/fine.py:53-70).  Each recomputes what it needs
 * from its forward's INPUTS, writes every element of its gradient exactly once (no zero fill, no atomics: the same bits from call
 * to call) and refuses the sizes its forward refuses, with the same codes, before any launch.  An upstream gradient g is a device
 * pointer to one float: nothing is read back to the host. */
/* d_msg [B (n_obj + n_hints)][D] -> d_qkv [B (n_obj + n_hints)][3 D].  With S = scale q k^T, P = softmax(S), scale = 1 / sqrt(D / 4):
 * dV[m] = sum_t P[t, m] dO[t], dP = dO V^T, dS = P o (dP - rowsum(P o dP)), dq[t] = scale sum_m dS[t, m] k[m],
 * dk[m] = scale sum_t dS[t, m] q[t]; dq to the q columns of the target rows, dk | dv to the k | v columns of the source rows. */
int t2p_match_attention_backward(const float* qkv, const float* d_msg, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                                 int32_t cross, float* d_qkv, t2p_stream_t stream);
/* dP [B][n_obj + 1][n_hints + 1] -> d_mdesc [B (n_obj + n_hints)][D] fp32 and d_bin [B] float64, the per-sample gradient of bin_score
 * (its gradient is their sum).  float64 throughout: the forward's iterations are run again with every iterate u_t, v_t kept in
 * `workspace` (sinkhorn_iters (n_obj + n_hints + 2) doubles per sample; T2P_E_WORKSPACE when it is too small), G = dP exp(Z) is
 * formed from the float64 log couplings, and the unrolled iterations are walked backwards.  sinkhorn_iters = 0 is legal. */
size_t t2p_match_head_backward_workspace_bytes(int64_t batch, int32_t n_obj, int32_t n_hints, int32_t sinkhorn_iters);
int t2p_match_head_backward(const float* mdesc, const float* dP, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                            float bin_score, int32_t sinkhorn_iters, float* d_mdesc, double* d_bin, void* workspace,
                            size_t workspace_bytes, t2p_stream_t stream);
/* The whole dP [B][n_obj + 1][n_hints + 1]: -g / (B M_b P[b, i, j]) per listed entry of sample b (M_b entries; a pair listed twice
 * counts twice), 0 elsewhere.  A listed coupling that is 0 gives what the formula gives. */
int t2p_matching_loss_backward(const float* P, int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* idx,
                               const int32_t* entry_ptr, int64_t n_entries, const float* g, float* dP, t2p_stream_t stream);
/* da [n] = 2 g (a - b) / n. */
int t2p_mse_loss_backward(const float* a, const float* b, int64_t n, const float* g, float* da, t2p_stream_t stream);
/* out [cols] = column sums of x [rows][cols], accumulated in float64 in a fixed order and rounded once: the bias gradients of the
 * matcher's Conv1d layers.  Three of its four bias families per layer stand in front of a softmax or a BatchNorm and have a gradient
 * that is exactly zero: what is left of it is the rounding of the summands, and an fp32 sum would add its own on top. */
int t2p_colsum(const float* x, int64_t rows, int32_t cols, float* out, t2p_stream_t stream);

/* The statistics training/fine.py:77-112 takes from one step - calc_recall_precision (training/losses.py:33-62) and three calls of
 * calc_pose_error (training/losses.py:81-123) with get_pos_in_cell (models/superglue_matcher.py:139-161) - in ONE launch on the
 * model's outputs where they are: matches0 int64 [B][n_obj], matches1 int64 [B][n_hints], offsets fp32 [B][n_hints][2].  The ground
 * truth comes from three device tables with n_rows rows (one per pose of the feed, training.SceneFineFeed), row pose_idx[b] for
 * sample b: gt_hint int32 [n_rows][n_obj] (the hint matched to a slot, or -1), pose_xy float64 [n_rows][2], slot_center_xy float64
 * [n_rows][n_obj][2] (the float64 object centres).  loss / loss_offsets: one fp32 value each on the device, or NULL.
 * sample_stats float64 [B][5] = recall, precision, pose_mid, pose_mean, pose_offsets of every sample:
 *   recall     (slots i with j = gt_hint[i] >= 0 and matches0[i] == j or matches1[j] == i) / (slots with gt_hint[i] >= 0); 0 without any
 *   precision  (slots with matches0[i] >= 0 and gt_hint[i] == matches0[i]) / (slots with matches0[i] >= 0); 0 without any
 *   pose_*     distance from pose_xy to the estimate: (0.5, 0.5) for pose_mid and when no slot is matched, else the mean over the
 *              matched slots of slot_center_xy[i] (pose_mean) or of slot_center_xy[i] + double(offsets[matches0[i]]) (pose_offsets)
 * step_row float64 [7] = double(loss), double(loss_offsets) (NaN for NULL), then the means over the samples of the five columns,
 * summed in ascending sample order.  float64 throughout, wavefront reductions with a fixed tree, no atomics: the same bits from call
 * to call; every output element is written.
 * Refused before any launch (T2P_E_ARG): NULL pointers (the two losses excepted); batch, n_obj or n_hints < 1; n_obj or n_hints > 63
 * (the token limit of t2p_match_attention); batch > T2P_FINE_STATS_MAX_BATCH (the per-sample rows of the batch reduction sit in
 * LDS: 1024 x 5 doubles = 40 KiB); n_rows outside [1, 2^30).
 * In the kernel a pose_idx outside [0, n_rows), a matches0 value outside [-1, n_hints), a matches1 value outside [-1, n_obj) or a
 * gt_hint entry outside [-1, n_hints) turns the sample's row (and so the five means) into NaN; nothing is read through it -
 * t2p_matching_loss's rule. */
#define T2P_FINE_STATS_MAX_BATCH 1024
int t2p_fine_step_stats(const int64_t* matches0, const int64_t* matches1, const float* offsets, const int32_t* pose_idx,
                        int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* gt_hint, const double* pose_xy,
                        const double* slot_center_xy, int64_t n_rows, const float* loss, const float* loss_offsets,
                        double* sample_stats, double* step_row, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Serving path (csrc/localize.hip): text queries against a database of cells that were encoded once.
 * ---------------------------------------------------------------------------------------------------------- */
/* t2p_match with its inputs addressed through tables: sample b matches the object tokens of database cell obj_row[b] against
 * the hint tokens of query hint_row[b].  obj_table fp32 [n_cells][n_obj][D] and hint_table fp32 [n_queries][n_hints][D] (both
 * 16-byte aligned), obj_row / hint_row int32 [batch] on the device.  Replaces the torch.stack of per-sample encodings of
 * models/superglue_matcher.py:94-103 for encodings that already exist: the reference re-encodes a cell's objects for every
 * (query, candidate) sample (dataloading/kitti360pose/eval.py:117-189, evaluation/pipeline.py:189-191).  One gather kernel
 * copies the samples' token rows into dense desc0 / desc1 at the head of `workspace`; t2p_match then runs on the copies with
 * the rest of it, so every output has the bits t2p_match gives on the gathered inputs.  Same limits and codes as t2p_match;
 * n_cells, n_queries in [1, 2^30).  A sample whose obj_row or hint_row lies outside its table is never read through: its tokens
 * are NaN, so its P is NaN and its matches are -1 (its offsets are not NaN: the offset MLP's ReLU maps NaN to 0 - a caller tells
 * such a sample by its P, or hands the same row to t2p_localize_poses, which marks it); the other samples are unaffected. */
size_t t2p_match_indexed_workspace_bytes(int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim);
int t2p_match_indexed(const float* obj_table, int64_t n_cells, const float* hint_table, int64_t n_queries, const int32_t* obj_row,
                      const int32_t* hint_row, int64_t batch, int32_t n_obj, int32_t n_hints, int32_t embed_dim,
                      const t2p_match_weights* w, int32_t sinkhorn_iters, float match_threshold, float* P, int64_t* matches0,
                      int64_t* matches1, float* mscores0, float* mscores1, float* offsets, void* workspace, size_t workspace_bytes,
                      t2p_stream_t stream);
/* The pose estimates of n_queries x top_k samples (query-major: sample q top_k + c) in one launch: get_pos_in_cell
 * (models/superglue_matcher.py:139-161), the world-coordinate step of calc_sample_accuracies (evaluation/utils.py:31-54,
 * bbox_w + pos_in_cell * cell_size) and the confidence pick of evaluation/pipeline.py:196, :256, which the reference computes on
 * host copies per query.  matches0 int64 [Q K][n_obj], offsets fp32 [Q K][n_hints][2] (the matcher's outputs, where they are),
 * cell_row int32 [Q K]: the sample's row of the float64 tables center_xy [n_cells][n_obj][2] (object centres of the cell's padded
 * slots), bbox_xy [n_cells][2], cell_size [n_cells].  Per sample: pos_mean [2] / pos_offset [2] float64 in cell units - the mean
 * over the slots with matches0[i] >= 0 of center_xy[i] resp. center_xy[i] + double(offsets[matches0[i]]), (0.5, 0.5) when
 * nothing matched - world_mean / world_offset [2] = bbox_xy + pos * cell_size, and matched int32 = the number of such slots.
 * Per query: best int32 = the candidate with the largest `matched`, the first among equals.  float64 throughout, wavefront
 * reductions with a fixed tree, no atomics: the same bits from call to call; every output element is written.
 * Refused before any launch (T2P_E_ARG): NULL pointers; top_k outside [1, T2P_LOCALIZE_MAX_TOP_K] (the candidates' counts sit in
 * LDS); n_obj or n_hints outside [1, 63]; n_cells outside [1, 2^30); n_queries < 0 (0 launches nothing).
 * In the kernel a cell_row outside [0, n_cells), a matches0 value outside [-1, n_hints) or a NaN among the sample's offsets
 * turns the sample's four rows into NaN and its `matched` into -1; nothing is read through it (t2p_fine_step_stats's rule).
 * `best` passes such samples over and is -1 when the query has no other. */
#define T2P_LOCALIZE_MAX_TOP_K 1024
int t2p_localize_poses(const int64_t* matches0, const float* offsets, const int32_t* cell_row, int64_t n_queries, int32_t top_k,
                       int32_t n_obj, int32_t n_hints, const double* center_xy, const double* bbox_xy, const double* cell_size,
                       int64_t n_cells, double* pos_mean, double* pos_offset, double* world_mean, double* world_offset,
                       int32_t* matched, int32_t* best, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Text branch: CellRetrievalNetwork.encode_text (models/cell_retrieval.py:69-75) on token ids produced by the
 * host tokeniser of LanguageEncoder.forward (models/modules.py:60-72).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct t2p_text_weights {
    const float* embedding; /* word_embedding.weight [V][D] (row 0 = padding/<unk>) */
    const float* w_ih;      /* [2][D][4D] k-major: lstm.weight_ih_l0^T, lstm.weight_ih_l0_reverse^T */
    const float* w_hh;      /* [2][D][4D] k-major: lstm.weight_hh_l0^T, ..._reverse^T */
    const float* bias;      /* [2][4D] = bias_ih + bias_hh (gate order i, f, g, o) */
    /* NULL (exact fp32 MFMA recurrence), or the f16x3 images of w_hh: per direction one packing.py::pack_f16x3_scaled image
     * (as t2p_cell_weights.sa_w2_x3: uint16 [2 planes hi,lo][4D/32 tiles][D/16 steps][2 halves][32 lanes][8] of
     * w' = w_hh_scale * w, w_hh_scale a power of two) - the recurrent product then runs as 3 f16 MFMAs per 16 k with fp32
     * accumulation: fp32-class error, a time step 5x shorter (a call's latency is max_len time steps whatever the batch) */
    const void* w_hh_x3;
    float w_hh_scale;
} t2p_text_weights;

size_t t2p_encode_text_workspace_bytes(int64_t batch, int32_t vocab, int32_t embed_dim);

/* tokens [batch][max_len] int32 right-padded with 0, lengths [batch] int32.  out_raw (nullable) receives the
 * LanguageEncoder output (mean of the two final hidden states), out the L2-normalised rows; both [batch][D]. */
int t2p_encode_text(const int32_t* tokens, const int32_t* lengths, int64_t batch, int32_t max_len, int32_t vocab,
                    int32_t embed_dim, const t2p_text_weights* w, float* out_raw, float* out, void* workspace,
                    size_t workspace_bytes, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Retrieval: replaces the per-query NumPy loop of training/coarse.py:134-140
 * (float64 `cell_encodings @ text_encodings[q]`, `argsort(-scores)[:k]`).
 * queries [nq][dim], cells [nc][dim] fp32; out_idx [nq][k] int64 (= cell row + index_offset, ties -> lower index,
 * -1 when nc < k), out_score [nq][k] float64.
 *
 * 1 <= k <= T2P_SIM_TOPK_MAX_K (T2P_E_ARG otherwise, nothing launched); dim 128, 256 or 384.  The float64 score of a
 * (query, cell) pair, and the order (score descending, ties and -0.0 / +0.0 to the lower cell index), do not depend on k:
 * the first j columns of a k-result are the j-result, bit for bit.  A NaN score is never retrieved; when fewer than k
 * cells qualify the tail is -1 / -inf.
 * Two selection paths.  Which one runs depends on the problem size for every k <= T2P_SIM_TOPK_REG_K, never on k within 1..16
 * (so the workspace of a shape is one number for all of them):
 *     register lists:  k <= T2P_SIM_TOPK_REG_K and nq * nc <  T2P_SIM_TOPK_TILE_MIN_PAIRS
 *     score tile:      k >  T2P_SIM_TOPK_REG_K, or nq * nc >= T2P_SIM_TOPK_TILE_MIN_PAIRS
 * (k <= T2P_SIM_TOPK_REG_K with nc > 33,554,400, one query's scores beyond the tile, stays on the lists whatever nq * nc).
 *   Register lists: per-lane candidate lists in registers, scores never leave the chip.  Workspace:
 *     nq * splits * 4 * 16 * 12 + 256 bytes, splits = the cell ranges the launch divides the database into (it depends on
 *     nq, nc and the device's CU count, not on k).
 *   Score tile: the call walks the queries in chunks; per chunk one kernel writes the chunk's float64 scores
 *     into the workspace and one workgroup per query selects its k exactly (radix selection on order-preserving keys,
 *     lowest-index ties by an ascending sweep, sort in LDS).  Workspace = one chunk's score tile, never more than
 *     T2P_SIM_TOPK_TILE_BYTES whatever nq, nc and k:
 *         ld    = ceil(nc / 16) * 16                       doubles per query row
 *         cap   = floor((T2P_SIM_TOPK_TILE_BYTES - 256) / (8 * ld)), rounded down to a multiple of 128 when >= 128
 *         chunk = min(nq, cap)                             queries per chunk
 *         bytes = chunk * 8 * ld + 256
 *     cap == 0, i.e. one query's scores (8 * nc bytes, nc > 33,554,400) exceed the tile: T2P_E_ARG with a message that
 *     says so (k <= T2P_SIM_TOPK_REG_K has no such limit besides nc < 2^31: the lists).  The workspace must be 16-byte aligned.
 * ---------------------------------------------------------------------------------------------------------- */
#define T2P_SIM_TOPK_MAX_K 1024
#define T2P_SIM_TOPK_REG_K 16
#define T2P_SIM_TOPK_TILE_MIN_PAIRS 256000 /* k <= T2P_SIM_TOPK_REG_K: nq * nc from which the score-tile path runs (profiles/t04_topk_route_sweep.md) */
#define T2P_SIM_TOPK_TILE_BYTES ((size_t)256 << 20) /* the MI355X's Infinity Cache: the selection re-reads the tile from it */
size_t t2p_sim_topk_workspace_bytes(int64_t nq, int64_t nc, int32_t k);
int t2p_sim_topk(const float* queries, const float* cells, int64_t nq, int64_t nc, int32_t dim, int32_t k,
                 int64_t index_offset, int64_t* out_idx, double* out_score, void* workspace, size_t workspace_bytes,
                 t2p_stream_t stream);
/* Group-restricted retrieval: the street oracle of the reference's evaluation (evaluation/pipeline.py:93-108: float64
 * scores of a query against the whole database, `scores[cell_street_indices != pose_street_idx] = -np.inf`, then
 * `argsort(-scores)[:k]`).  The arguments of t2p_sim_topk plus query_group [nq] and cell_group [nc] (int32, any values:
 * only equality matters; cell_group is indexed like `cells`, index_offset shifts only the indices written out; nothing is
 * read past cell_group[nc - 1]).  Workspace: t2p_sim_topk_workspace_bytes(nq, nc, k), the same as the unrestricted call.
 *   effective score  s'(q, c) = cell_group[c] == query_group[q] ? s(q, c) : -inf, s = t2p_sim_topk's score bit for bit.
 *   The mask is a select, not arithmetic: a masked pair is -inf whatever its product was, NaN included.
 *   The result is the first k entries of the same order on s' (score descending, ties to the lower cell index): a query
 *   whose group holds fewer than k cells gets its group's cells first, then masked cells with score -inf in ascending
 *   index - what argsort on the masked array gives under the pinned tie rule.  An allowed cell whose score is NaN is never
 *   retrieved; nc < k fills the tail with -1 / -inf.  Same k range, widths, alignment rules and two selection paths as
 *   t2p_sim_topk; a NULL group pointer (with nq > 0 / nc > 0) is T2P_E_ARG, nothing launched. */
int t2p_sim_topk_grouped(const float* queries, const float* cells, const int32_t* query_group, const int32_t* cell_group,
                         int64_t nq, int64_t nc, int32_t dim, int32_t k, int64_t index_offset, int64_t* out_idx,
                         double* out_score, void* workspace, size_t workspace_bytes, t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Opt-in kernel timing for bench.py: when enabled, every kernel launch of the calls above is bracketed by hipEvents
 * recorded on the launch stream (the only process-global state of the library; not thread-safe, off by default).
 * t2p_profile_report waits for the recorded launches and writes "<kernel> <launches> <total_ms>\n" lines into buf.
 * ---------------------------------------------------------------------------------------------------------- */
void t2p_profile_enable(int on);
int t2p_profile_report(char* buf, size_t buf_bytes);
/* Measurement hook for the per-kernel energy table (profiles/energy_table.py): from now on every launch the report above
 * lists under `scope` (the ten largest kernels of the cell branch have the hook) is issued `reps` times back to back with
 * the same arguments - each of them rewrites its outputs from its inputs, so results do not change - which holds ONE kernel
 * on the chip long enough for a power sampler.  reps <= 1 or scope == NULL: off (the default). */
void t2p_profile_repeat(const char* scope, int32_t reps);

/* ------------------------------------------------------------------------------------------------------------
 * Training-mode text branch (first part): one step of the LSTM recurrence of
 * LanguageEncoder.forward (models/modules.py:77-90: nn.LSTM on a PackedSequence, gates i, f, g, o) with its activations
 * kept, and the matching backward step.  The host loop (text2pos-cvpr2022_amd/modules.py::_LstmTrainFn) alternates them with
 * t2p_gemm for the recurrent products; the caller is training/coarse.py:44 (anchor = model.encode_text(...); loss.backward()).
 *   forward:  pre [B][4D] = h_{s-1} W_hh (k-major product from t2p_gemm); gate_table [V][4D] = E W_ih + b_ih + b_hh;
 *             sequences with step >= length carry (c, h) over and store zero gates; reverse != 0 reads token len-1-step.
 *   backward: dh = dh_gemm (d_pre of step+1 times W_hh^T, NULL for the last step) + dh_carry_in; d_pre [B][4D] is the
 *             gradient of the step's gate pre-activations (zero for finished sequences, whose dh / dc pass through
 *             dh_carry_out / dc_out).
 * ---------------------------------------------------------------------------------------------------------- */
/* The whole recurrence of ONE direction with the time loop inside the library (one call instead of 2 T: the per-step kernels are
 * tiny and the Python loop around them was bound by the host's launch rate).  Layouts as modules._LstmTrainFn keeps them:
 * gates [T][B][4D], cs / hs [T+1][B][D] with slice 0 = the initial state (zeros), w_hh_k [D][4D] = W_hh^T, pre_ws [B][4D] scratch.
 * backward: dh_last [B][D] = the gradient of the final hidden state, w_hh_t [4D][D] = W_hh, d_pre [T][B][4D] (out),
 * ws [5][B][D] scratch.  embed_dim must be a multiple of 4 (else T2P_E_UNSUPPORTED with nothing written: the host falls back to the
 * per-step calls, its products zero-padded to t2p_gemm's granules).
 * The recurrent products run on a few-rows kernel (tg_gemm.hip::k_gemm_skinny): fp32 sums in another order than t2p_gemm's. */
int t2p_lstm_train_forward(const float* gate_table, const float* w_hh_k, const int32_t* tokens, const int32_t* lengths,
                           int64_t batch, int32_t max_len, int32_t embed_dim, int32_t reverse, float* gates, float* cs, float* hs,
                           float* pre_ws, t2p_stream_t stream);
int t2p_lstm_train_backward(const float* dh_last, const float* w_hh_t, const float* gates, const float* cs, const int32_t* lengths,
                            int64_t batch, int32_t max_len, int32_t embed_dim, float* d_pre, float* ws, t2p_stream_t stream);
int t2p_lstm_cell_forward(const float* pre, const float* gate_table, const int32_t* tokens, const int32_t* lengths,
                          int64_t batch, int32_t max_len, int32_t embed_dim, int32_t step, int32_t reverse, const float* c_prev,
                          const float* h_prev, float* gates, float* c, float* h, t2p_stream_t stream);
int t2p_lstm_cell_backward(const float* dh_gemm, const float* dh_carry_in, const float* dc_in, const float* gates,
                           const float* c_prev, const float* c, const int32_t* lengths, int64_t batch, int32_t embed_dim,
                           int32_t step, float* d_pre, float* dc_out, float* dh_carry_out, t2p_stream_t stream);

/* Training-mode building blocks of the cell branch (second part; csrc/train_ops.hip).
 * BatchNorm1d in training mode + optional ReLU over row SEGMENTS (models/modules.py:21-29 in model.train(); the reference
 * runs its PointNet++ once per cell, models/object_encoder.py:92-95, so those layers take their statistics per cell):
 * x, y [M][C] fp32; seg_ptr [n_seg+1] int32 (device) tiles the rows; mean / invstd / var_unbiased [n_seg][C] (biased
 * variance normalises, the unbiased one feeds the running estimate; float64 accumulation in a fixed order: row chunks of a
 * segment are reduced by separate workgroups into `workspace` - t2p_bn_train_workspace_bytes - and combined in order).
 * backward: dx [M][C]; dgamma_seg / dbeta_seg [n_seg + 1][C]: per segment, and in row n_seg their sum over the segments (the
 * layer's weight / bias gradient, added in float64 in segment order); it takes x
 * and the layer's beta [C], not y: the ReLU mask (y > 0) is recomputed from x exactly as the forward formed y.
 * Segment max (PointConv aggr="max", gnn.global_max_pool, DynamicEdgeConv aggr="max" over rows sorted by destination):
 * out [n_seg][C], arg [n_seg][C] = winning row (first one on ties, -1 and out = 0 for an empty segment); the backward
 * routes dout to the winning rows.
 * Non-finite input, forward: both follow torch.  The ReLU keeps NaN (a NaN or inf among a segment's rows makes that segment's
 * column of y NaN - its statistics are NaN -, not 0); segment max: a NaN wins over every number (arg = the first NaN row), a column
 * that is all -inf gives -inf with arg = the segment's first row.  The backward passes on non-finite input are unspecified. */
size_t t2p_bn_train_workspace_bytes(int64_t rows, int32_t n_seg, int32_t channels);
int t2p_bn_relu_train_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int64_t rows, int32_t channels,
                              const float* gamma, const float* beta, float eps, int32_t relu, float* y, float* mean,
                              float* invstd, float* var_unbiased, void* workspace, size_t workspace_bytes,
                              t2p_stream_t stream);
int t2p_bn_relu_train_backward(const float* dy, const float* x, const float* beta, const int32_t* seg_ptr, int32_t n_seg,
                               int64_t rows, int32_t channels, const float* mean, const float* invstd, const float* gamma,
                               int32_t relu, float* dx, float* dgamma_seg, float* dbeta_seg, void* workspace,
                               size_t workspace_bytes, t2p_stream_t stream);
int t2p_segment_max_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* out, int32_t* arg,
                            t2p_stream_t stream);
int t2p_segment_max_backward(const float* dout, const int32_t* arg, const int32_t* seg_ptr, int32_t n_seg, int32_t channels,
                             float* dx, t2p_stream_t stream);
/* segment mean (variation 1: DynamicEdgeConv aggr="mean", gnn.global_mean_pool; models/cell_retrieval.py:50-54, :100-103) */
int t2p_segment_mean_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* out,
                             t2p_stream_t stream);
int t2p_segment_mean_backward(const float* dout, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* dx,
                              t2p_stream_t stream);

/* Message inputs of the two graph operators and F.normalize, with their backward (training mode):
 *   edge features  out [E][width] = [x[src] | pos[src] - pos_c[dst] | 0 ..]   (PointConv, models/pointcloud/pointnet2.py:31-35;
 *                  width >= C + 3 is the row pitch of out / d_out: a multiple of 8 spares the Linear behind it a padded copy);
 *                  backward: dx [rows of x][C] += d_out[:, :C] at src (dx zeroed by the caller; float atomics)
 *   pair features  out [E][2D] = [x[tgt] | x[src] - x[tgt]]          (DynamicEdgeConv, models/cell_retrieval.py:46-48)
 *   rownorm backward: gradient of t2p_rownorm (F.normalize, eps 1e-12) */
int t2p_edge_features_forward(const float* x, const float* pos, const float* pos_c, const int32_t* src, const int32_t* dst,
                              int64_t n_edges, int32_t channels, int32_t width, float* out, t2p_stream_t stream);
int t2p_edge_features_backward(const float* d_out, const int32_t* src, int64_t n_edges, int32_t channels, int32_t width, float* dx,
                               t2p_stream_t stream);
int t2p_pair_features_forward(const float* x, const int32_t* tgt, const int32_t* src, int64_t n_edges, int32_t dim, float* out,
                              t2p_stream_t stream);
int t2p_pair_features_backward(const float* d_out, const int32_t* tgt, const int32_t* src, int64_t n_edges, int32_t dim,
                               float* dx, t2p_stream_t stream);
int t2p_rownorm_backward(const float* x, const float* dy, int64_t n_rows, int32_t dim, float* dx, t2p_stream_t stream);

/* PairwiseRankingLoss (training/losses.py:126-164, margin training/args.py:46) on the score matrix of the L2-normalised
 * anchor / positive embeddings, scores [B][B] = im_n s_n^T:  row_loss [B] (loss = sum(row_loss) / B),
 * d_scores [B][B] = dLoss / dScores, row_count [B] scratch.  Deterministic (fixed-order reductions).
 * Hinge rule: a term max(0, x) counts, and has gradient 1, only where x > 0.  At an exact hinge x == 0 this implementation
 * yields gradient 0; the reference's element-wise torch.max(zeros, x) yields 1/2 there.  Off the diagonal d_scores is
 * (number of its two terms that are > 0) * fl(1 / B), on the diagonal -(number of terms > 0 that hold it) / B.
 * NaN rule: a NaN hinge stays NaN, as in torch.max(zeros, x): row_loss[i] is NaN if S[i][i], any S[i][j] or any S[j][j] is.
 * Every entry of d_scores is written; its values where a NaN took part are unspecified.  batch in [0, 32768]; 0 writes nothing. */
int t2p_pairwise_ranking(const float* scores, int32_t batch, float margin, float* row_loss, float* d_scores, float* row_count,
                         t2p_stream_t stream);

/* HardestRankingLoss (training/losses.py:167-201, --ranking_loss hardest) on the same score matrix: best [2B] = the largest
 * hinge of every row (first B) and column (last B), where [2B] = its position (-1 if none is positive),
 * d_scores [B][B] = dLoss / dScores; loss = (sum best[:B] + sum best[B:]) / B.
 * Hinge rule: only a hinge > 0 can win; a row or column whose largest hinge is <= 0 has best = 0, where = -1 and adds nothing
 * to d_scores (torch's relu has gradient 0 at an exact 0 as well; an element-wise torch.max(zeros, x) would yield 1/2).
 * Tie rule: among equal maxima the lowest index wins (torch.max on the CPU).  d_scores gets +fl(1 / B) at each winner and
 * -fl(1 / B) on the diagonal of its row (row maxima) or column (column maxima): every entry is a small integer times fl(1 / B).
 * NaN rule: a NaN hinge wins over every number, as relu and max keep it in torch: best = NaN, where = the first position that
 * holds one.  Every entry of d_scores is written; its values in the rows / columns of a NaN winner are unspecified.
 * batch in [0, 32768]; 0 writes nothing. */
int t2p_hardest_ranking(const float* scores, int32_t batch, float margin, float* best, int32_t* where, float* d_scores,
                        t2p_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Stage-level exports (used by the stage-wise parity tests).
 * ---------------------------------------------------------------------------------------------------------- */
/* Fused gnn.fps + gnn.radius of the three SA levels (pointnet2.py:26-30); outputs as in t2p_cell_trace.
 * n_cent_l = ceil(n_dense_l / 2), n_dense_0 = n_pts. */
int t2p_sample_group(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host /*[3]*/,
                     uint8_t* const* fps_idx /*[3]*/, uint8_t* const* nbr /*[3]*/, uint8_t* const* cnt /*[3]*/,
                     t2p_stream_t stream);
/* The same kernel with its compact edge-row lists as output (what the SA edge kernels of t2p_encode_cells consume):
 * rows[l] uint16 [n_obj][n_cent_l * 33], per object sorted by centroid: (centroid | 0x80 for the self-loop row) << 8 | source,
 * hits in ascending source order (<= 32), then - with self_loops - the centroid's self-loop row (source byte = centroid);
 * n_rows[l] uint16 [n_obj].  t2p_edge_counts / t2p_edge_expand turn a level's lists into the edge arrays of
 * gnn.PointConv(...)(x, (pos, pos[idx]), edge_index) with torch_geometric's self-loop rewrite (pointnet2.py:26-35) for the
 * training-mode path: counts [n_obj * n_cent] kept rows per centroid (a hit whose two CELL-local indices agree is dropped: the
 * appended loop (i, i) replaces it; first_obj [n_obj] = first object of the object's cell); with cent_ptr = exclusive prefix of
 * counts (n_obj * n_cent + 1 entries), src / dst [cent_ptr[last]] int32 = (dense row, centroid row) of every edge, sorted by dst. */
int t2p_group_rows(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host /*[3]*/, int32_t self_loops,
                   uint8_t* const* fps_idx /*[3]*/, uint16_t* const* rows /*[3]*/, uint16_t* const* n_rows /*[3]*/,
                   t2p_stream_t stream);
/* t2p_group_rows with the row list of SA level 2 in the SHARED form its f16x3 kernel consumes (share_mask bit 1; every other
 * bit must be clear: levels 1 and 3 have no shared form; n_pts = 256 unless share_mask = 0).  For inspection and tests.
 * T.FixedPoints draws with replacement, so an object with few base points has few distinct positions; FPS (start at point 0,
 * ties to the lowest index) takes each once and then picks point 0 for the rest of the level.  Those TAIL centroids - c > 0 with
 * fps_idx[c] == 0, a suffix of the centroid list - stand at centroid 0's position: their ball-query hits are centroid 0's and
 * each of their edge rows is centroid 0's row, bit for bit; only the self-loop row (dense row c of the cell's batch) is their
 * own.  In a shared list
 *   - a centroid that is not in the tail has its hits and its self-loop row, as in t2p_group_rows;
 *   - the FIRST tail centroid's hits appear once under the pseudo-centroid code X = 64 in the centroid byte (no self-loop
 *     flag), followed by its self-loop row ((c | 0x80) << 8 | c);
 *   - every later tail centroid has its self-loop row only (self_loops = 0: no row at all).
 * The consumer accumulates the X rows against centroid 0's B row in a slot of their own and takes max(acc[c], acc[X]) for every
 * tail centroid c - what the full list leaves in acc[c], since max is idempotent.  A shared list is not sorted by centroid;
 * n_rows, the 0xFFFF terminator and the alignment are those of t2p_group_rows.  t2p_edge_counts / t2p_edge_expand and
 * t2p_dedup_rows take full lists only. */
int t2p_group_rows_shared(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host /*[3]*/, int32_t self_loops,
                          int32_t share_mask, uint8_t* const* fps_idx /*[3]*/, uint16_t* const* rows /*[3]*/,
                          uint16_t* const* n_rows /*[3]*/, t2p_stream_t stream);
/* t2p_group_rows_shared followed by t2p_dedup_rows on level 1's list, as t2p_encode_cells runs them by default: the same
 * fps_idx, lists, counts and terminators, bit for bit.  Of level 1 the scan kernel writes only each centroid's 256-bit hit mask
 * (into rows[0], which is workspace until the call returns its list there) and stops at the first tail centroid; a builder
 * kernel then applies the 32-neighbour cap in point order, drops the rows of repeated points (the repeat test of
 * t2p_dedup_rows: rgb is compared too) and writes the list once.  Levels 2 and 3 run no FPS: they pick the prefix of level 1's
 * picks, and the builder runs their ball queries one lane per centroid.  n_pts must be 256; xyz, rgb and rows 16-byte aligned. */
int t2p_group_rows_built(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, const float* radius_host /*[3]*/,
                         int32_t self_loops, int32_t share_mask, uint8_t* const* fps_idx /*[3]*/, uint16_t* const* rows /*[3]*/,
                         uint16_t* const* n_rows /*[3]*/, t2p_stream_t stream);
/* t2p_group_rows_built with the lists of SA levels 2 and 3 as t2p_encode_cells consumes them when self_loops = 0: without the
 * rows whose SOURCE is a repeated dense point.  Let k1 be level 1's first tail centroid (128: none).  Levels 2 and 3 pick the prefix of
 * level 1's picks (fps_idx[l][c] = c below k1, 0 from there on), so dense point j >= k_prev - k_prev = k1 at level 2, min(k1, 64)
 * at level 3 - is a tail centroid of the level below: it stands at dense point 0's position and carries row 0's features bit for
 * bit.  Dense point 0 is in range whenever j is and is always inside the 32-neighbour cap, so the row of j repeats a row the
 * centroid already has and the max-aggregate does not change.  The repeats are a suffix of the index order: a centroid's list
 * holds its first 32 hits among the dense points below k_prev; the shared copy of level 2's tail rows is cut the same way.
 * Self-loop rows, row order, tags, n_rows and the terminator are those of t2p_group_rows_built.  The premise holds only for
 * a model WITHOUT self-loop rows: a self-loop row takes its source from another object's rows (row sbase + c of the cell's
 * flattened batch, torch_geometric's index aliasing), which makes every tail centroid's output row its own - so
 * t2p_encode_cells consumes these lists only when self_loops = 0; the export itself lists by geometry alone, whatever
 * self_loops says.  Same arguments; for inspection and tests (t2p_edge_counts / t2p_edge_expand take full lists only). */
int t2p_group_rows_pruned(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, const float* radius_host /*[3]*/,
                          int32_t self_loops, int32_t share_mask, uint8_t* const* fps_idx /*[3]*/, uint16_t* const* rows /*[3]*/,
                          uint16_t* const* n_rows /*[3]*/, t2p_stream_t stream);
/* The range balancing of the SA edge kernels on its own (the device code t2p_encode_cells runs between the row builder and SA1):
 *   prefix[i] = sum over g < i of ceil(n_rows[g] / tile_rows) for i in [0, n], so prefix[n] = total tiles;
 *   bounds[b] = the first m in [0, n] with prefix[m] >= floor(b * total / n_wg) (b * total in 64 bits) for b < n_wg, bounds[n_wg] = n:
 * workgroup b of n_wg owns the objects [bounds[b], bounds[b + 1]).  n_rows uint16 [n]; prefix int32 [n + 1]; bounds int32 [n_wg + 1];
 * n >= 0, tile_rows >= 1, n_wg >= 1.  Integers only: the result does not depend on the launch. */
int t2p_sa_balance(const uint16_t* n_rows, int32_t n, int32_t tile_rows, int32_t n_wg, int32_t* prefix /*[n+1]*/,
                   int32_t* bounds /*[n_wg+1]*/, t2p_stream_t stream);
int t2p_edge_counts(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, int64_t n_obj, int32_t n_dense,
                    int32_t n_cent, int32_t self_loops, int32_t* counts, t2p_stream_t stream);
int t2p_edge_expand(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, const int32_t* cent_ptr, int64_t n_obj,
                    int32_t n_dense, int32_t n_cent, int32_t self_loops, int32_t* src, int32_t* dst, t2p_stream_t stream);
/* Level-1 (SA1) row lists without the edges of repeated points.  rows uint16 [n_obj][(n_pts/2) * 33]: per object the compact
 * edge-row list of k_sample_group, sorted by centroid: (centroid | 0x80 for the self-loop row) << 8 | source point, terminated
 * by four 0xFFFF; n_rows uint16 [n_obj].  A row whose source point repeats an EARLIER point of the object bit for bit (xyz and
 * rgb; T.FixedPoints draws with replacement, dataloading/kitti360pose/utils.py:99-109) carries the same message as that
 * point's row for the same centroid, so under PointConv's max-aggregation (pointnet2.py:31-35) it can be dropped.  In place;
 * detection is conservative (a repeat may survive, a non-repeat is never dropped).  n_pts must be 256. */
int t2p_dedup_rows(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, uint16_t* rows, uint16_t* n_rows,
                   t2p_stream_t stream);
/* knn of DynamicEdgeConv (cell_retrieval.py:46-48): x [n][dim], seg_ptr [n_seg+1] int32, out [n][k] int32 */
int t2p_knn(const float* x, int32_t dim, const int32_t* seg_ptr, int32_t n_seg, int32_t max_seg_rows, int32_t k,
            int32_t* out_idx, t2p_stream_t stream);
/* C[M][ldc] (+c0) = act(A[M][lda] W[K][N] + bias[N]);  K % 4 == 0, N % 8 == 0, lda % 4 == 0; A and W 16-byte aligned.
 * Only columns [c0, c0 + N) of rows [0, M) of C are written.  bias may be NULL.  act is the identity (relu = 0) or ReLU as
 * torch.relu states it: v <= 0 ? 0 : v, so a NaN stays a NaN (a non-finite element of A reaches exactly its own row of C). */
int t2p_gemm(const float* a, int32_t lda, const float* w, const float* bias, float* c, int32_t ldc, int32_t c0,
             int64_t m, int32_t k, int32_t n, int32_t relu, t2p_stream_t stream);
/* t2p_gemm with a residual added behind the activation: C = act(A W + bias) + resid[M][ldr] (resid NULL: t2p_gemm).  resid may
 * alias C (ldr = ldc, resid = c + c0: each element is read and written by one thread).  -1 on NULL operands or pitches below
 * the widths (lda < k, ldc < c0 + n, ldr < n). */
int t2p_gemm_residual(const float* a, int32_t lda, const float* w, const float* bias, float* c, int32_t ldc, int32_t c0,
                      int64_t m, int32_t k, int32_t n, int32_t relu, const float* resid, int32_t ldr, t2p_stream_t stream);
/* The same contract on the f16x3 matrix path (csrc/tg_gemm_x3.hip), the default-precision GEMM of the heads and the matcher:
 * wx is the image of packing.py::pack_gemm_x3 for `scale` (a power of two), 16-byte aligned.  A is split into fp16 hi + lo on
 * the fly; hi.hi + hi.lo + lo.hi share one fp32 accumulator, the epilogue divides by scale.  amax_in (may be NULL) is the
 * fp16-range guard word of A: the kernel raises it (atomic max on the bit pattern) to max |A[m][k]| over [M][K] exactly.
 * A NaN in A reaches its own row of C and nothing else (an infinity is past the guard: its row becomes NaN).
 * -1 on NULL operands (a, wx, c with m > 0), sizes below 1, pitches below the widths (lda < k, ldc < c0 + n, ldr < n), and a
 * scale that is not a positive power of two. */
int t2p_gemm_x3(const float* a, int32_t lda, const void* wx, float scale, const float* bias, float* c, int32_t ldc, int32_t c0,
                int64_t m, int32_t k, int32_t n, int32_t relu, const float* resid, int32_t ldr, uint32_t* amax_in,
                t2p_stream_t stream);
/* C[M][ldc] = A[M][lda] W[K][N] for few rows and a long K (csrc/tg_gemm.hip::k_gemm_skinny, the per-step products of the
 * training-mode LSTM): no bias, no activation; K % 4 == 0 (K >= 4), lda % 4 == 0, A 16-byte aligned, any N.  fp32 MFMA, sums
 * in another order than t2p_gemm's (deterministic).  -1 on NULL operands (with m > 0), sizes below 1, lda < k or ldc < n, and a K or
 * lda that is no multiple of 4. */
int t2p_gemm_skinny(const float* a, int32_t lda, const float* w, float* c, int32_t ldc, int64_t m, int32_t k, int32_t n,
                    t2p_stream_t stream);
/* C[k1][n] (ldc) = A[m][k1]^T B[m][n]: a product whose reduction runs over the ROWS - the weight gradient dW = dY^T X of
 * every nn.Linear, the recurrent / input weight gradients of the LSTM and its gate-table gradient in the training-mode path
 * (training/coarse.py:31-62 through autograd).  The rows are split over the grid and the partial products added in a fixed
 * order (deterministic); fp32 MFMA.  workspace: t2p_gemm_tn_workspace_bytes. */
size_t t2p_gemm_tn_workspace_bytes(int64_t m, int32_t k1, int32_t n);
int t2p_gemm_tn(const float* a, int32_t lda, const float* b, int32_t ldb, float* c, int32_t ldc, int64_t m, int32_t k1, int32_t n,
                void* workspace, size_t workspace_bytes, t2p_stream_t stream);
/* Weight and bias gradient of an nn.Linear in the training-mode path (every `get_mlp` block under model.train(),
 * models/modules.py:11-36), exact fp32 MFMA (csrc/train_gemm.hip):
 *   dW[K1][N] = dY[M][K1]^T X[M][N] and colsum[K1] = column sums of dY (the bias gradient; may be null): every operand row is
 *   read once per row range, the row ranges' partial blocks are added in a fixed order (deterministic).
 *   lda, ldb multiples of 4, operands 16-byte aligned.  workspace: t2p_linear_wgrad_workspace_bytes. */
size_t t2p_linear_wgrad_workspace_bytes(int64_t m, int32_t k1, int32_t n);
int t2p_linear_wgrad_f32(const float* dy, int32_t lda, const float* x, int32_t ldb, float* dw, int32_t ldc, float* colsum, int64_t m,
                         int32_t k1, int32_t n, void* workspace, size_t workspace_bytes, t2p_stream_t stream);
/* F.normalize(x, dim=-1), eps 1e-12 */
int t2p_rownorm(const float* x, int64_t n_rows, int32_t dim, float* out, t2p_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* T2P_H */
