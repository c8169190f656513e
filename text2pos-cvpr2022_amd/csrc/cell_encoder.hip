// The cell encoder's host side: the per-chunk workspace, the stages one chunk runs through, and the exports built on them
// (t2p_encode_cells, t2p_pointnet2_forward, the row-list exports).  No kernel lives here; every stage is a list of launches.
//
//   trunk          group -> sa_levels -> global_abstraction -> trunk_heads (lin1, lin2): PointNet2.forward up to features2
//   object_encoder the concat slots (mlp_pointnet | colour | position, or the embedding ablations) and mlp_merge
//   cell_head      rownorm, P / Q, kNN, DynamicEdgeConv, pool, lin, rownorm
//   copy_traces    the stage outputs a caller asked for
//
// An entry point issues its own cell index first (it clears the chunk's guard words), then the stages it needs, then the guard
// check as the chunk's last kernel, then the trace copies.
#include "../../include/t2p.h"
#include "t2p_common.h"

namespace t2p {
namespace {

// Level geometry for n_pts points: dense/centroid counts, feature widths, hidden widths.
struct Geo {
    int nd[3], nc[3];
    int gp;   // GA max group: SA level 3 writes gp rows per object (the next power of two >= nc[2]; rows past nc[2] repeat the last)
    static constexpr int H[3] = {32, 128, 256};
    static constexpr int C[3] = {64, 128, 256};
    static constexpr int LD[3] = {96, 160, 288};  // SA output row = [C | xyz 0 | 28 pad columns: zero at level 3, never written at levels 1-2 (their readers mask them: k_live)]: K % 32 == 0 for the next GEMM
    explicit Geo(int n_pts) {
        nd[0] = n_pts;
        for (int l = 0; l < 3; l++) {
            nc[l] = (nd[l] + 1) / 2;
            if (l < 2) nd[l + 1] = nc[l];
        }
        gp = 1;
        while (gp < nc[2]) gp *= 2;
    }
    // f16x3: the specialised SA kernels (LDS centroid table) are built for the level shapes of 256 points per object
    bool specialised(int l) const {
        static constexpr int ND[3] = {256, 128, 64}, NC[3] = {128, 64, 32};
        return nd[l] == ND[l] && nc[l] == NC[l];
    }
};
constexpr int Geo::H[3];
constexpr int Geo::C[3];
constexpr int Geo::LD[3];

struct CellWs {
    GroupTables gt;
    float *A[3], *B[3], *F[3];
    float *gh, *f0, *f1, *f2, *cat, *emb, *embn, *P, *Q, *x1, *pool, *l1, *l2;
    int32_t *knn, *seg_ptr, *first, *prefix[3], *bounds[3];
    uint32_t* guard;  // [G_SLOTS] fp16-range guard words of the chunk (t2p_common.h)
};

// rows of GA layer 1's output: n objects x gp rows, rounded up to the 32-row tiles GA layer 2 reads
int64_t gh_rows(int64_t n, const Geo& g) { return (n * g.gp + 31) / 32 * 32; }

int n_features(const t2p_cell_config& cfg) { return (cfg.use_class ? 1 : 0) + (cfg.use_color ? 1 : 0) + (cfg.use_position ? 1 : 0); }

// Carve the per-chunk workspace (n objects, nb cells).  With base == nullptr this only measures.  D = 0 (the trunk entry) leaves
// the buffers of the object encoder and the cell head empty.
size_t carve(Bump& b, int64_t n, int64_t nb, const Geo& g, int D, int nfeat, int knn_k, CellWs* ws) {
    CellWs w{};
    for (int l = 0; l < 3; l++) {
        w.gt.n_dense[l] = g.nd[l];
        w.gt.n_cent[l] = g.nc[l];
        w.gt.fps_idx[l] = b.take<uint8_t>(n * g.nc[l]);
        w.gt.nbr[l] = b.take<uint8_t>(n * g.nc[l] * 32);   // only filled when a trace asks for it
        w.gt.cnt[l] = b.take<uint8_t>(n * g.nc[l]);
        w.gt.rows[l] = b.take<uint16_t>(n * g.nc[l] * 33);
        w.gt.n_rows[l] = b.take<uint16_t>(n);
        w.A[l] = b.take<float>(n * g.nd[l] * Geo::H[l]);
        w.B[l] = b.take<float>(n * g.nc[l] * Geo::H[l]);
        w.F[l] = b.take<float>(n * (l == 2 ? g.gp : g.nc[l]) * Geo::LD[l]);
    }
    w.gh = b.take<float>(gh_rows(n, g) * 512);
    w.f0 = b.take<float>(n * 1024);
    w.f1 = b.take<float>(n * 512);
    w.f2 = b.take<float>(n * 256);
    w.cat = b.take<float>(n * (size_t)(nfeat > 0 ? nfeat : 1) * D);
    w.emb = b.take<float>(n * D);
    w.embn = b.take<float>(n * D);
    w.P = b.take<float>(n * D);
    w.Q = b.take<float>(n * D);
    w.x1 = b.take<float>(n * D);
    w.knn = b.take<int32_t>(n * (size_t)knn_k);
    w.first = b.take<int32_t>(n);
    for (int l = 0; l < 3; l++) {
        w.prefix[l] = b.take<int32_t>(n + 1);
        w.bounds[l] = b.take<int32_t>(1024 + 1);
    }
    w.seg_ptr = b.take<int32_t>(nb + 1);
    w.guard = b.take<uint32_t>(G_SLOTS);
    w.pool = b.take<float>(nb * D);
    w.l1 = b.take<float>(nb * D);
    w.l2 = b.take<float>(nb * D);
    if (ws) *ws = w;
    return align_up(b.off, 256);
}
size_t carve_cells(Bump& b, int64_t n, int64_t nb, const t2p_cell_config& cfg, CellWs* ws) {
    return carve(b, n, nb, Geo(cfg.n_pts), cfg.embed_dim, n_features(cfg), cfg.knn_k, ws);
}
size_t carve_trunk(Bump& b, int64_t n, const t2p_cell_config& cfg, CellWs* ws) { return carve(b, n, 1, Geo(cfg.n_pts), 0, 0, 0, ws); }

// Default chunk: as many objects as the 32-bit table offsets of the SA kernels allow (< 65,536); measured 32,768 / 49,152 /
// 65,000 objects per chunk: 105.1 / 104.4 / 104.1 ms per 12k-cell step (fewer launches, fewer kernel tails), ~0.6 MB each
int default_chunk(const t2p_cell_config& cfg) { return cfg.chunk_objects > 0 ? cfg.chunk_objects : T2P_DEFAULT_CHUNK_OBJECTS; }

// The two groups of configuration checks the trunk entry shares with the cell entry (whose messages they carry)
int check_n_pts(const t2p_cell_config& cfg) {
    if (cfg.n_pts < 8 || cfg.n_pts > 256) {
        set_error("encode_cells: n_pts=%d not built (8 <= n_pts <= 256 points per object)", cfg.n_pts);
        return T2P_E_UNSUPPORTED;
    }
    return 0;
}
int check_plan(const t2p_cell_config& cfg) {
    T2P_CHECK_ARG(cfg.precision == 0 || cfg.precision == 1, "encode_cells: precision=%d (0 = fp32, 1 = f16x3)", cfg.precision);
    T2P_CHECK_ARG((cfg.tuning & ~T2P_TUNING_MASK) == 0, "encode_cells: tuning=%#x has bits outside %#x", cfg.tuning, T2P_TUNING_MASK);
    return 0;
}

int check_cfg(const t2p_cell_config* cfg) {
    T2P_CHECK_ARG(cfg != nullptr, "encode_cells: cfg is NULL");
    T2P_TRY(check_n_pts(*cfg));
    if (cfg->objects_only) {
        if (cfg->embed_dim < 64 || cfg->embed_dim > 512 || cfg->embed_dim % 64 != 0) {
            set_error("encode_cells: objects_only supports embed_dim in {64, 128, ..., 512}, got %d", cfg->embed_dim);
            return T2P_E_UNSUPPORTED;
        }
    } else if (cfg->embed_dim != 256 && cfg->embed_dim != 128 && cfg->embed_dim != 384) {
        set_error("encode_cells: embed_dim=%d not built for the cell head (128, 256, 384; the host pads e.g. 300 to 384)", cfg->embed_dim);
        return T2P_E_UNSUPPORTED;
    }
    T2P_CHECK_ARG(cfg->variation == 0 || cfg->variation == 1, "encode_cells: variation=%d (0 = max, 1 = mean)",
                  cfg->variation);
    if (cfg->variation == 1 && cfg->knn_k != 8) {
        set_error("encode_cells: variation=1 (mean aggregation) is built for knn_k = 8 only, got %d", cfg->knn_k);
        return T2P_E_UNSUPPORTED;
    }
    T2P_CHECK_ARG(cfg->pointnet_features >= 0 && cfg->pointnet_features <= 2, "encode_cells: pointnet_features=%d",
                  cfg->pointnet_features);
    T2P_CHECK_ARG(cfg->use_class || cfg->use_color || cfg->use_position, "encode_cells: use_features is empty");
    T2P_CHECK_ARG(cfg->knn_k >= 1 && cfg->knn_k <= 32, "encode_cells: knn_k=%d outside [1,32]", cfg->knn_k);
    T2P_TRY(check_plan(*cfg));
    // 32-bit byte offsets into the per-chunk tables (n_obj * 128 points * 128 floats * 4 B < 2^32) and 16-bit object-local
    // indices cap a chunk at 65,535 objects; checked here, not deep inside a kernel launcher
    T2P_CHECK_ARG(cfg->chunk_objects >= 0 && cfg->chunk_objects <= T2P_MAX_CHUNK_OBJECTS,
                  "encode_cells: chunk_objects=%d outside [0, %d] (0 = default %d); the workspace takes ~0.6 MB per object of a chunk",
                  cfg->chunk_objects, T2P_MAX_CHUNK_OBJECTS, T2P_DEFAULT_CHUNK_OBJECTS);
    T2P_CHECK_ARG(!cfg->class_embed || cfg->class_idx != nullptr, "encode_cells: class_embed needs class_idx");
    T2P_CHECK_ARG(!cfg->color_embed || cfg->color_idx != nullptr, "encode_cells: color_embed needs color_idx");
    return 0;
}

// What the trunk needs of the weights before anything is launched: the packed images on the f16x3 path, the norms for its guard
int check_x3_weights(const char* what, const t2p_cell_weights& w, const t2p_cell_config& cfg) {
    if (cfg.precision == 1)
        T2P_CHECK_ARG(w.sa_w2_x3[0] && w.sa_w2_x3[1] && w.sa_w2_x3[2] && w.sa_b2_x3[0] && w.sa_b2_x3[1] && w.sa_b2_x3[2] &&
                          w.sa_w2_scale[0] > 0.f && w.sa_w2_scale[1] > 0.f && w.sa_w2_scale[2] > 0.f && w.sa_w1_x3[1] &&
                          w.sa_w1_x3[2] && w.ga_w1_x3 && w.ga_w2_x3,
                      "%s: precision = f16x3 needs the packed *_x3 weight images", what);
    if (cfg.precision == 1 && cfg.overflow_flag != nullptr)
        T2P_CHECK_ARG(w.ga_w1_l1 > 0.f && w.ga_b1_absmax >= 0.f && w.sa_a1_l1 > 0.f && w.sa_wp_l1[0] >= 0.f,
                      "%s: the fp16-range guard needs the weight norms of t2p_cell_weights (packing.py)", what);
    return 0;
}

// One chunk on its way through the stages: n objects in nb cells.  The trunk stages read of cfg only what include/t2p.h
// names for t2p_pointnet2_forward (n_pts, self_loops, radius, precision, overflow_flag, tuning).
struct Chunk {
    hipStream_t st;
    int64_t n, nb;
    Geo g;
    const t2p_cell_config& cfg;
    const t2p_cell_weights& W;
    CellWs& ws;
    // fp16-range guard (f16x3 only): the chunk's words are cleared by the first kernel and judged by the last
    uint32_t* guard;
    GuardBounds gbounds;

    Chunk(hipStream_t st_, int64_t n_, int64_t nb_, const t2p_cell_config& cfg_, const t2p_cell_weights& W_, CellWs& ws_)
        : st(st_), n(n_), nb(nb_), g(cfg_.n_pts), cfg(cfg_), W(W_), ws(ws_),
          guard(cfg_.precision == 1 && cfg_.overflow_flag != nullptr ? ws_.guard : nullptr), gbounds{} {
        for (int l = 0; l < 3; l++) gbounds.wp_l1[l] = W.sa_wp_l1[l];
        gbounds.a1_l1 = W.sa_a1_l1;
        gbounds.a1_bmax = W.sa_b1_absmax;
        gbounds.ga1_l1 = W.ga_w1_l1;
        gbounds.ga1_bmax = W.ga_b1_absmax;
    }
    uint32_t* gslot(int i) const { return guard ? guard + i : nullptr; }
    bool f16x3() const { return cfg.precision == 1; }
    // f16x3: the SA kernels of the level shapes of 256 points build their centroid tables B_i = W1p pos_i in LDS (sa_points.hip,
    // sa_rows.hip, sa3.hip); the HBM tables B_l are then neither written nor read.  The stream kernel (ws_sa.hip: fp32, and f16x3 at
    // the other shapes) gathers its table from HBM.
    bool lds_btab(int l) const { return f16x3() && g.specialised(l); }
    // level 0 runs on sa_points.hip, which computes layer 1 per edge from the points themselves: no point table A_1 either
    bool sa1_points() const { return lds_btab(0); }
    int guard_check() const { return launch_guard_check(guard, cfg.overflow_flag, gbounds, st); }

    int trunk(const float* xyz, const float* rgb, bool want_nbr) const;   // = group, sa_levels, global_abstraction, trunk_heads
    int group(const float* xyz, const float* rgb, bool want_nbr) const;
    int sa_levels(const float* xyz, const float* rgb) const;
    int global_abstraction() const;
    int trunk_heads() const;
    int object_encoder(const float* center, const float* mean_rgb, int32_t o_lo, const float** emb_out) const;
    int cell_head(const float* emb, int max_cell, float* out) const;
    int copy_traces(const t2p_cell_trace& tr, int64_t obj0, int64_t cell0, bool trunk_ran, const float* emb) const;
};

// FPS + ball query of the three levels, the row lists the SA kernels consume and their balanced object ranges
int Chunk::group(const float* xyz, const float* rgb, bool want_nbr) const {
    ws.gt.self_loops = cfg.self_loops;
    GroupTables gt = ws.gt;
    if (!want_nbr)
        for (int l = 0; l < 3; l++) gt.nbr[l] = gt.cnt[l] = nullptr;
    // the layer-1 tables that depend on geometry only are written by the same kernel: B_l = W1p_l pos_i (+ the
    // [xyz | 0] tail of the F_l rows) for every level, and the K = 6 point table A_1 of level 0
    for (int l = 0; l < 3; l++) {
        const int cf = l == 0 ? 3 : Geo::C[l - 1];
        gt.B[l] = lds_btab(l) ? nullptr : ws.B[l];
        gt.wp[l] = W.sa_w1[l] + (size_t)cf * Geo::H[l];
        gt.H[l] = Geo::H[l];
        gt.tail[l] = ws.F[l];
        gt.ld_tail[l] = Geo::LD[l];
        gt.tail_col0[l] = Geo::C[l];
    }
    gt.tail_rows[2] = g.gp;
    gt.A1 = sa1_points() ? nullptr : ws.A[0];
    gt.w1 = W.sa_w1[0];
    gt.b1 = W.sa_b1[0];
    gt.rgb = rgb;
    gt.H1 = Geo::H[0];
    gt.guard = guard;

    // the launch shapes of the three SA levels (which kernel runs a level decides its row-list form and its balancing)
    SaParams bp[3] = {};
    for (int l = 0; l < 3; l++) {
        bp[l].n_rows = gt.n_rows[l];
        bp[l].n_obj = n;
        bp[l].prefix_ws = ws.prefix[l];
        bp[l].bounds_ws = ws.bounds[l];
        bp[l].W_x3 = f16x3() ? W.sa_w2_x3[l] : nullptr;
        bp[l].wp = lds_btab(l) ? W.sa_w1[l] : nullptr;   // (non-null = LDS centroid table: selects the launch shape)
        bp[l].n_dense = g.nd[l];
        bp[l].n_cent = g.nc[l];
    }
    bp[0].w1 = sa1_points() ? W.sa_w1[0] : nullptr;
    // level 2: the centroids FPS repeats once an object's distinct positions are used up share one copy of their edge rows
    // (GroupTables::share_tail; same bits, -13 % rows on the synthetic cells) where k_sa_rows consumes them
    for (int l = 0; l < 3; l++) gt.share_tail[l] = sa_shares_tail_rows(l, Geo::H[l], Geo::C[l], bp[l], cfg.n_pts, cfg.tuning) ? 1 : 0;

    // level 0: edges of repeated points leave the row list (same max-aggregate, -36 % SA1 rows on the synthetic cells).
    // Default: the scan publishes level 0's hit masks and k_build_rows writes the pruned list once; tuning bit 3: the scan
    // lists every hit and k_dedup_rows prunes the list in place, as before (the same list, bit for bit)
    const bool prune_l0 = !(cfg.tuning & 1) && cfg.n_pts == 256;
    gt.mask_l0 = prune_l0 && !(cfg.tuning & 8) && !want_nbr && gt.rows[0] && gt.rows[1] && gt.rows[2] ? 1 : 0;
    // levels 2 and 3 of that plan: the rows whose source is a repeated dense point (a tail centroid of the level below) leave the
    // lists too (GroupTables::prune_dup; -5.5 % / -6.6 % rows on the synthetic cells); tuning bit 2 keeps the full lists.
    // WITHOUT self-loop rows only: a self-loop row takes its source from another object's rows (row sbase + c of the cell's
    // flattened batch, PyG's index aliasing), so with them a tail centroid's output row is max(centroid 0's hits, a row of its
    // own) - not centroid 0's row - and the dense point it becomes one level up repeats nothing
    gt.prune_dup[1] = gt.prune_dup[2] = gt.mask_l0 && !(cfg.tuning & 4) && !cfg.self_loops ? 1 : 0;
    T2P_TRY(launch_sample_group(xyz, n, cfg.n_pts, cfg.radius, gt, st));
    if (gt.mask_l0)
        T2P_TRY(launch_build_rows(xyz, rgb, n, cfg.n_pts, cfg.radius, gt, st));
    else if (prune_l0)
        T2P_TRY(launch_dedup_rows(xyz, rgb, n, cfg.n_pts, gt.rows[0], gt.n_rows[0], g.nc[0], st));
    // the per-centroid row counts of all three levels exist now: cut every level's balanced object ranges at once
    return launch_sa_balance_levels(bp, Geo::H, Geo::C, st);
}

// The three set-abstraction levels
int Chunk::sa_levels(const float* xyz, const float* rgb) const {
    for (int l = 0; l < 3; l++) {
        const int H = Geo::H[l], C = Geo::C[l];
        const int cf = l == 0 ? 3 : Geo::C[l - 1];  // feature columns in front of the xyz columns
        // layer-1 point table A_j = W1 [x_j | pos_j] + b1
        if (l != 0) {  // (level 0: written by k_sample_group)
            WsParams p{};
            p.A = ws.F[l - 1];
            p.lda = Geo::LD[l - 1];
            p.k_live = Geo::C[l - 1] + 4;   // [features | xyz 0]; the pad columns behind are never written
            p.W = W.sa_w1[l];
            p.W_x3 = f16x3() ? W.sa_w1_x3[l] : nullptr;
            p.ldw = H;
            p.bias = W.sa_b1[l];
            p.out = ws.A[l];
            p.ldo = H;
            p.relu = 0;
            p.M = n * g.nd[l];
            p.amax_out = gslot(l == 1 ? G_A2 : G_A3);
            T2P_TRY(launch_ws(WS_DENSE_STORE, Geo::LD[l - 1] - (f16x3() ? 16 : 0), H, p, st));  // (f16x3: K stops at C + 16)
        }
        // per-edge ReLU(A_j - B_i) -> layer 2 -> max per centroid
        SaParams p{};
        p.A = ws.A[l];
        p.Bc = ws.B[l];
        p.wp = lds_btab(l) ? W.sa_w1[l] + (size_t)cf * Geo::H[l] : nullptr;
        p.W = W.sa_w2[l];
        p.W_x3 = f16x3() ? W.sa_w2_x3[l] : nullptr;
        p.bias = f16x3() ? W.sa_b2_x3[l] : W.sa_b2[l];
        p.out_scale = f16x3() ? 1.0f / W.sa_w2_scale[l] : 1.0f;
        p.out = ws.F[l];
        p.ldo = Geo::LD[l];
        p.rows = ws.gt.rows[l];
        p.n_rows = ws.gt.n_rows[l];
        p.first = ws.first;
        p.fps_idx = ws.gt.fps_idx[l];
        p.pos_src = l == 0 ? xyz : ws.F[l - 1];
        p.ld_pos = l == 0 ? 3 : Geo::LD[l - 1];
        p.pos_col0 = l == 0 ? 0 : Geo::C[l - 1];
        if (l == 0 && sa1_points()) {
            p.feat_src = rgb;
            p.w1 = W.sa_w1[0];
            p.b1 = W.sa_b1[0];
        }
        p.n_dense = g.nd[l];
        p.n_cent = g.nc[l];
        p.n_obj = n;
        p.prefix_ws = ws.prefix[l];
        p.bounds_ws = ws.bounds[l];
        p.balanced = 1;
        p.amax_out = gslot(G_F1 + l);
        if (l == 2) p.out_rows = g.gp;
        T2P_TRY(launch_ws_sa(H, C, p, st));
    }
    return 0;
}

// [x | pos] -> 512 -> 1024, max over the object's nc[2] points (gp rows, the padding repeats one)
int Chunk::global_abstraction() const {
    WsParams p{};
    p.A = ws.F[2];
    p.lda = Geo::LD[2];
    p.W = W.ga_w1;
    p.W_x3 = f16x3() ? W.ga_w1_x3 : nullptr;
    p.ldw = 512;
    p.bias = W.ga_b1;
    p.out = ws.gh;
    // f16x3: GA1 hands its ReLU output to GA2 already split into fp16 hi / lo planes (same bytes as fp32), so the
    // eight column-slice workgroups of GA2 stage it with plain 16-byte copies instead of re-splitting it 8 times
    _Float16* gh_hi = (_Float16*)ws.gh;
    _Float16* gh_lo = gh_hi + (size_t)gh_rows(n, g) * 512;
    if (f16x3()) {
        p.out_hi = gh_hi;
        p.out_lo = gh_lo;
        p.amax_out = gslot(G_GA_H);
    }
    p.ldo = 512;
    p.relu = 1;
    p.M = n * g.gp;
    T2P_TRY(launch_ws(WS_DENSE_STORE, Geo::LD[2] - (f16x3() ? 16 : 0), 512, p, st));
    WsParams q{};
    q.A = ws.gh;
    if (f16x3()) {
        q.A_hi = gh_hi;
        q.A_lo = gh_lo;
    }
    q.lda = 512;
    q.W = W.ga_w2;
    q.W_x3 = f16x3() ? W.ga_w2_x3 : nullptr;
    q.ldw = 1024;
    q.bias = W.ga_b2;
    q.out = ws.f0;
    q.ldo = 1024;
    q.relu = 1;
    q.M = n * g.gp;
    q.group_rows = g.gp;
    return launch_ws(WS_DENSE_GROUPMAX, 512, 1024, q, st);
}

// PointNet2.lin1 / lin2: features0 -> features1 -> features2
int Chunk::trunk_heads() const {
    const bool x3 = f16x3() && W.lin1_x3 && W.lin2_x3;   // both images or neither
    const DenseW lin1{W.lin1_w, x3 ? W.lin1_x3 : nullptr, W.lin1_scale}, lin2{W.lin2_w, x3 ? W.lin2_x3 : nullptr, W.lin2_scale};
    T2P_TRY(launch_dense(ws.f0, 1024, lin1, W.lin1_b, ws.f1, 512, 0, n, 1024, 512, 1, st, nullptr, 0, gslot(G_PN_F0)));
    return launch_dense(ws.f1, 512, lin2, W.lin2_b, ws.f2, 256, 0, n, 512, 256, 1, st, nullptr, 0, gslot(G_PN_F1));
}

// PointNet2.forward up to features2 (behind the entry's cell index: the SA kernels read ws.first)
int Chunk::trunk(const float* xyz, const float* rgb, bool want_nbr) const {
    T2P_TRY(group(xyz, rgb, want_nbr));
    T2P_TRY(sa_levels(xyz, rgb));
    T2P_TRY(global_abstraction());
    return trunk_heads();
}

// ObjectEncoder.forward behind the PointNet++: one concat slot per feature, then mlp_merge.  *emb_out: the [n][D] result.
int Chunk::object_encoder(const float* center, const float* mean_rgb, int32_t o_lo, const float** emb_out) const {
    const int D = cfg.embed_dim, nfeat = n_features(cfg), ldcat = nfeat * D;
    int slot = 0;
    if (cfg.use_class && cfg.class_embed) {
        T2P_TRY(launch_gather_rownorm(W.class_embedding, cfg.class_idx + o_lo, n, D, ws.cat, ldcat, slot * D, st));
        slot++;
    } else if (cfg.use_class) {
        const float* fin = cfg.pointnet_features == 0 ? ws.f0 : (cfg.pointnet_features == 1 ? ws.f1 : ws.f2);
        const int kin = cfg.pointnet_features == 0 ? 1024 : (cfg.pointnet_features == 1 ? 512 : 256);
        // mlp_pointnet into P (scratch), then F.normalize into the concat slot
        const DenseW pn{W.pn_w, f16x3() ? W.pn_x3 : nullptr, W.pn_scale};
        T2P_TRY(launch_dense(fin, kin, pn, W.pn_b, ws.P, D, 0, n, kin, D, 1, st, nullptr, 0, gslot(G_PN_F0 + cfg.pointnet_features)));
        T2P_TRY(launch_rownorm(ws.P, D, n, D, ws.cat, ldcat, slot * D, st));
        slot++;
    }
    if (cfg.use_color && cfg.color_embed) {
        T2P_TRY(launch_gather_rownorm(W.color_embedding, cfg.color_idx + o_lo, n, D, ws.cat, ldcat, slot * D, st));
        slot++;
    } else if (cfg.use_color) {
        T2P_TRY(launch_mlp3_norm(mean_rgb, n, W.col_w1, W.col_b1, W.col_w2, W.col_b2, D, ws.cat, ldcat, slot * D, st));
        slot++;
    }
    if (cfg.use_position) {
        T2P_TRY(launch_mlp3_norm(center, n, W.pos_w1, W.pos_b1, W.pos_w2, W.pos_b2, D, ws.cat, ldcat, slot * D, st));
        slot++;
    }
    *emb_out = ws.cat;  // single feature: embeddings[0] is returned un-merged (object_encoder.py:137-140)
    if (nfeat > 1) {
        const DenseW merge{W.merge_w, f16x3() ? W.merge_x3 : nullptr, W.merge_scale};
        T2P_TRY(launch_dense(ws.cat, ldcat, merge, W.merge_b, ws.emb, D, 0, n, ldcat, D, 1, st, nullptr, 0, gslot(G_GEMM_IN)));
        *emb_out = ws.emb;
    }
    return 0;
}

// Cell head: normalize, DynamicEdgeConv(k, max), global max pool, lin, normalize
int Chunk::cell_head(const float* emb, int max_cell, float* out) const {
    const int D = cfg.embed_dim;
    T2P_TRY(launch_rownorm(emb, D, n, D, ws.embn, D, 0, st));
    const bool x3 = f16x3() && W.g_wp_x3 && W.g_wq_x3;   // both images or neither
    const DenseW wp{W.g_wp, x3 ? W.g_wp_x3 : nullptr, W.g_wp_scale}, wq{W.g_wq, x3 ? W.g_wq_x3 : nullptr, W.g_wq_scale};
    T2P_TRY(launch_dense(ws.embn, D, wp, W.g_bp, ws.P, D, 0, n, D, D, 0, st, nullptr, 0, gslot(G_GEMM_IN)));
    T2P_TRY(launch_dense(ws.embn, D, wq, nullptr, ws.Q, D, 0, n, D, D, 0, st, nullptr, 0, gslot(G_GEMM_IN)));
    T2P_TRY(launch_knn(ws.embn, D, ws.seg_ptr, (int)nb, max_cell, cfg.knn_k, ws.knn, st));
    WsParams p{};
    p.A = ws.Q;
    p.lda = D;
    p.Bc = ws.P;
    p.W = W.g_w2;
    p.W_x3 = f16x3() ? W.g_w2_x3 : nullptr;   // f16x3 image of layer 2 (absent: fp32 MFMA)
    p.amax_out = gslot(G_EDGE);            // (here: the rows this kernel splits itself)
    p.ldw = D;
    p.bias = W.g_b2;
    p.out = ws.x1;
    p.ldo = D;
    p.relu = 1;
    // small calls (the reference's 64-cell batches: ~1,000 objects = 31 groups of 32 on 256 CUs): groups of 8 destinations
    p.knn_group = (n + 31) / 32 < num_cus() ? 8 : 32;
    p.n_groups = (n + p.knn_group - 1) / p.knn_group;
    p.knn_idx = ws.knn;
    p.knn_k = cfg.knn_k;
    p.n_dst = n;
    p.mean = cfg.variation == 1;  // cell_retrieval.py:50-54: DynamicEdgeConv(aggr="mean") + global_mean_pool
    T2P_TRY(launch_ws(WS_EDGE_KNN, D, D, p, st));
    T2P_TRY(launch_segmax(ws.x1, D, ws.seg_ptr, (int)nb, ws.pool, cfg.variation == 1, st, ws.knn, cfg.knn_k, gslot(G_INPUT)));
    T2P_TRY(launch_gemm(ws.pool, D, W.lin_w1, W.lin_b1, ws.l1, D, 0, nb, D, D, 1, st));
    T2P_TRY(launch_gemm(ws.l1, D, W.lin_w2, W.lin_b2, ws.l2, D, 0, nb, D, D, 1, st));
    return launch_rownorm(ws.l2, D, nb, D, out, D, 0, st);
}

template <typename T>
int copy_trace(T* dst, int64_t row0, size_t width, const T* src, int64_t n, hipStream_t st) {
    if (dst == nullptr || n == 0 || width == 0) return 0;
    hipError_t e = hipMemcpyAsync(dst + row0 * width, src, (size_t)n * width * sizeof(T), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        set_error("encode_cells: trace copy failed: %s", hipGetErrorString(e));
        return (int)e;
    }
    return 0;
}

// The stage outputs tr names, into its object rows obj0 .. obj0 + n and its cell rows cell0 .. cell0 + nb.  trunk_ran: the
// PointNet++ stages hold this chunk's values; emb: the object encoder's result (nullptr: not run), with which tr->knn_idx and
// the cell head's stages go (not for objects_only calls: the head did not run).
int Chunk::copy_traces(const t2p_cell_trace& tr, int64_t obj0, int64_t cell0, bool trunk_ran, const float* emb) const {
    for (int l = 0; trunk_ran && l < 3; l++) {
        T2P_TRY(copy_trace(tr.fps_idx[l], obj0, g.nc[l], ws.gt.fps_idx[l], n, st));
        T2P_TRY(copy_trace(tr.nbr[l], obj0, (size_t)g.nc[l] * 32, ws.gt.nbr[l], n, st));
        T2P_TRY(copy_trace(tr.cnt[l], obj0, g.nc[l], ws.gt.cnt[l], n, st));
        if (tr.sa_out[l] && n > 0) {   // [features | xyz 0] of every row; the pad columns behind are left as the caller set them
            const int rows = l == 2 ? g.gp : g.nc[l];   // (level 3: the gp - nc[2] padding rows of an object stay behind)
            const size_t ld = Geo::LD[l] * sizeof(float);
            hipError_t e = hipSuccess;
            if (rows == g.nc[l])
                e = hipMemcpy2DAsync(tr.sa_out[l] + obj0 * g.nc[l] * Geo::LD[l], ld, ws.F[l], ld, (Geo::C[l] + 4) * sizeof(float),
                                     (size_t)n * g.nc[l], hipMemcpyDeviceToDevice, st);
            for (int cc = 0; rows != g.nc[l] && cc < g.nc[l] && e == hipSuccess; cc++)   // centroid cc of every object
                e = hipMemcpy2DAsync(tr.sa_out[l] + (obj0 * g.nc[l] + cc) * Geo::LD[l], g.nc[l] * ld, ws.F[l] + (size_t)cc * Geo::LD[l],
                                     rows * ld, (Geo::C[l] + 4) * sizeof(float), (size_t)n, hipMemcpyDeviceToDevice, st);
            if (e != hipSuccess) {
                set_error("encode_cells: trace copy failed: %s", hipGetErrorString(e));
                return (int)e;
            }
        }
    }
    if (trunk_ran) {
        T2P_TRY(copy_trace(tr.features0, obj0, 1024, ws.f0, n, st));
        T2P_TRY(copy_trace(tr.features1, obj0, 512, ws.f1, n, st));
        T2P_TRY(copy_trace(tr.features2, obj0, 256, ws.f2, n, st));
    }
    if (emb != nullptr) {
        T2P_TRY(copy_trace(tr.obj_emb, obj0, cfg.embed_dim, emb, n, st));
        // knn indices are chunk-local object rows; tests use a single chunk or add the chunk offset themselves
        T2P_TRY(copy_trace(tr.knn_idx, obj0, cfg.knn_k, ws.knn, n, st));
    }
    if (emb != nullptr && !cfg.objects_only) {
        const size_t D = cfg.embed_dim;
        T2P_TRY(copy_trace(tr.head_in, obj0, D, ws.embn, n, st));
        T2P_TRY(copy_trace(tr.head_edge, obj0, D, ws.x1, n, st));
        T2P_TRY(copy_trace(tr.head_pool, cell0, D, ws.pool, nb, st));
        T2P_TRY(copy_trace(tr.head_l1, cell0, D, ws.l1, nb, st));
        T2P_TRY(copy_trace(tr.head_l2, cell0, D, ws.l2, nb, st));
    }
    return 0;
}

// Whole cells per chunk, at most `chunk` objects (a single larger cell still forms its own chunk).
int64_t next_chunk_end(const int32_t* cp, int64_t c0, int64_t n_cells, int chunk) {
    int64_t c1 = c0 + 1;
    while (c1 < n_cells && (cp[c1 + 1] - cp[c0]) <= chunk) c1++;
    return c1;
}

// GroupTables of a row-list export for n_pts points per object.  rows / n_rows, or nbr / cnt, may be NULL as a whole (that
// form is not wanted); with rows given, a NULL table of one level is refused under the export's name.
int fill_group_tables(const char* what, GroupTables& gt, int n_pts, int self_loops, int share_mask, uint8_t* const* fps_idx,
                      uint16_t* const* rows, uint16_t* const* n_rows, uint8_t* const* nbr, uint8_t* const* cnt) {
    const Geo g(n_pts);
    gt = GroupTables{};
    gt.self_loops = self_loops ? 1 : 0;
    for (int l = 0; l < 3; l++) {
        if (rows) T2P_CHECK_ARG(fps_idx[l] && rows[l] && n_rows[l], "%s: NULL table of level %d", what, l);
        gt.fps_idx[l] = fps_idx[l];
        gt.rows[l] = rows ? rows[l] : nullptr;
        gt.n_rows[l] = rows ? n_rows[l] : nullptr;
        gt.nbr[l] = nbr ? nbr[l] : nullptr;
        gt.cnt[l] = cnt ? cnt[l] : nullptr;
        gt.n_dense[l] = g.nd[l];
        gt.n_cent[l] = g.nc[l];
        gt.share_tail[l] = (share_mask >> l) & 1;
    }
    return 0;
}

// t2p_group_rows (share_mask = 0) and t2p_group_rows_shared
int group_rows(const char* what, const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host, int32_t self_loops,
               int32_t share_mask, uint8_t* const* fps_idx, uint16_t* const* rows, uint16_t* const* n_rows, t2p_stream_t stream) {
    T2P_CHECK_ARG(xyz && radius_host && fps_idx && rows && n_rows, "%s: NULL argument", what);
    T2P_CHECK_ARG((share_mask & ~2) == 0, "%s: share_mask=%#x (bit 1: SA level 2; no other level has a shared form)", what, share_mask);
    T2P_CHECK_ARG(share_mask == 0 || n_pts == 256, "%s: shared lists exist for 256 points per object (n_pts = %d)", what, n_pts);
    GroupTables gt;
    T2P_TRY(fill_group_tables(what, gt, n_pts, self_loops, share_mask, fps_idx, rows, n_rows, nullptr, nullptr));
    return launch_sample_group(xyz, n_obj, n_pts, radius_host, gt, (hipStream_t)stream);
}

// t2p_group_rows_built (prune_dup = 0) and t2p_group_rows_pruned
int group_rows_built(const char* what, const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, const float* radius_host,
                     int32_t self_loops, int32_t share_mask, int prune_dup, uint8_t* const* fps_idx, uint16_t* const* rows,
                     uint16_t* const* n_rows, t2p_stream_t stream) {
    T2P_CHECK_ARG(xyz && rgb && radius_host && fps_idx && rows && n_rows, "%s: NULL argument", what);
    T2P_CHECK_ARG(n_obj >= 0, "%s: negative size", what);
    T2P_CHECK_ARG((share_mask & ~2) == 0, "%s: share_mask=%#x (bit 1: SA level 2; no other level has a shared form)", what, share_mask);
    T2P_CHECK_ARG(n_pts == 256, "%s: built for 256 points per object (n_pts = %d)", what, n_pts);
    GroupTables gt;
    T2P_TRY(fill_group_tables(what, gt, n_pts, self_loops, share_mask, fps_idx, rows, n_rows, nullptr, nullptr));
    gt.mask_l0 = 1;
    gt.prune_dup[1] = gt.prune_dup[2] = prune_dup;
    T2P_CHECK_ARG((((uintptr_t)xyz | (uintptr_t)rgb | (uintptr_t)rows[0] | (uintptr_t)rows[1] | (uintptr_t)rows[2]) & 15) == 0,
                  "%s: xyz, rgb and rows must be 16-byte aligned", what);
    T2P_TRY(launch_sample_group(xyz, n_obj, n_pts, radius_host, gt, (hipStream_t)stream));
    return launch_build_rows(xyz, rgb, n_obj, n_pts, radius_host, gt, (hipStream_t)stream);
}

}  // namespace
}  // namespace t2p

using namespace t2p;

extern "C" {

size_t t2p_encode_cells_workspace_bytes(int64_t n_obj, int64_t n_cells, const t2p_cell_config* cfg) {
    if (cfg == nullptr || n_obj <= 0) return 256;
    // a chunk holds at most max(chunk_objects, largest cell) objects; the caller may not know the largest cell here,
    // so size for min(n_obj, chunk) and let t2p_encode_cells re-check against the actual partition.
    int64_t n = default_chunk(*cfg);
    if (n > n_obj) n = n_obj;
    int64_t nb = n_cells < n ? n_cells : n;
    Bump b{nullptr, 0, 0};
    return carve_cells(b, n, nb > 0 ? nb : 1, *cfg, nullptr) + 256;
}

int t2p_encode_cells(const float* xyz, const float* rgb, const float* center, const float* mean_rgb,
                     const int32_t* cell_ptr_host, const int32_t* cell_ptr, int64_t n_obj, int64_t n_cells,
                     const t2p_cell_weights* w, const t2p_cell_config* cfg, float* out, const t2p_cell_trace* trace,
                     void* workspace, size_t workspace_bytes, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_TRY(check_cfg(cfg));
    T2P_CHECK_ARG(w != nullptr && cell_ptr_host != nullptr && cell_ptr != nullptr, "encode_cells: NULL argument");
    T2P_CHECK_ARG(n_cells >= 0 && n_obj >= 0, "encode_cells: negative size");
    if (n_cells == 0) return 0;  // an empty batch has no output rows (and its buffers may be NULL)
    if (cfg->objects_only)
        T2P_CHECK_ARG(trace != nullptr && trace->obj_emb != nullptr, "encode_cells: objects_only needs trace->obj_emb");
    else
        T2P_CHECK_ARG(out != nullptr, "encode_cells: out is NULL");
    T2P_CHECK_ARG(!cfg->class_embed || w->class_embedding != nullptr, "encode_cells: class_embedding weights missing");
    T2P_CHECK_ARG(!cfg->color_embed || w->color_embedding != nullptr, "encode_cells: color_embedding weights missing");
    T2P_TRY(check_x3_weights("encode_cells", *w, *cfg));
    T2P_CHECK_ARG(cell_ptr_host[0] == 0 && cell_ptr_host[n_cells] == n_obj,
                  "encode_cells: cell_ptr must start at 0 and end at n_obj=%lld (got %d..%d)", (long long)n_obj,
                  cell_ptr_host[0], cell_ptr_host[n_cells]);
    for (int64_t c = 0; c < n_cells; c++)
        T2P_CHECK_ARG(cell_ptr_host[c + 1] > cell_ptr_host[c],
                      "encode_cells: cell %lld is empty (the reference asserts >= 1 object per cell, "
                      "dataloading/kitti360pose/utils.py:108)", (long long)c);
    T2P_CHECK_ARG((((uintptr_t)xyz | (uintptr_t)rgb | (uintptr_t)workspace) & 15) == 0,
                  "encode_cells: xyz, rgb and workspace must be 16-byte aligned");
    // models/object_encoder.py:86: the PointNet++ only runs when the "class" feature does not come from class_embedding
    const bool run_pointnet = cfg->use_class && !cfg->class_embed;
    // objects_only: the fine stage consumes ObjectEncoder.forward's output as is, and nothing else is handed back
    t2p_cell_trace tr{};
    if (cfg->objects_only)
        tr.obj_emb = trace->obj_emb;
    else if (trace != nullptr)
        tr = *trace;
    const bool want_nbr = trace != nullptr && (trace->nbr[0] || trace->nbr[1] || trace->nbr[2] || trace->cnt[0] || trace->cnt[1] || trace->cnt[2]);
    const int chunk = default_chunk(*cfg);
    for (int64_t c0 = 0; c0 < n_cells;) {
        const int64_t c1 = next_chunk_end(cell_ptr_host, c0, n_cells, chunk);
        const int32_t o_lo = cell_ptr_host[c0], o_hi = cell_ptr_host[c1];
        const int64_t n = o_hi - o_lo, nb = c1 - c0;
        int max_cell = 0;
        for (int64_t c = c0; c < c1; c++) {
            const int m = cell_ptr_host[c + 1] - cell_ptr_host[c];
            max_cell = m > max_cell ? m : max_cell;
        }
        T2P_CHECK_ARG(n <= T2P_MAX_CHUNK_OBJECTS,
                      "encode_cells: cell %lld alone holds %lld objects; a chunk (whole cells) is limited to %d objects",
                      (long long)c0, (long long)n, T2P_MAX_CHUNK_OBJECTS);
        Bump b{(char*)workspace, 0, workspace_bytes};
        CellWs ws;
        const size_t need = carve_cells(b, n, nb, *cfg, &ws);
        if (need > workspace_bytes) {
            set_error("encode_cells: workspace %zu B < %zu B needed for a chunk of %lld objects / %lld cells",
                      workspace_bytes, need, (long long)n, (long long)nb);
            return T2P_E_WORKSPACE;
        }
        const Chunk c(st, n, nb, *cfg, *w, ws);
        const int64_t P3 = (int64_t)cfg->n_pts * 3;
        T2P_TRY(launch_cell_index(cell_ptr + c0, (int)nb, o_lo, ws.seg_ptr, ws.first, st, c.guard));
        if (run_pointnet) T2P_TRY(c.trunk(xyz + o_lo * P3, rgb + o_lo * P3, want_nbr));
        const float* emb = nullptr;
        T2P_TRY(c.object_encoder(center + (int64_t)o_lo * 3, mean_rgb + (int64_t)o_lo * 3, o_lo, &emb));
        if (!cfg->objects_only) T2P_TRY(c.cell_head(emb, max_cell, out + c0 * cfg->embed_dim));
        T2P_TRY(c.guard_check());
        T2P_TRY(c.copy_traces(tr, o_lo, c0, run_pointnet, emb));
        c0 = c1;
    }
    return 0;
}

// ---- PointNet++ as a classifier of its own (models/pointcloud/pointnet2.py:80-100): the trunk stages on ONE cell of n_obj objects

size_t t2p_pointnet2_workspace_bytes(int64_t n_obj, const t2p_cell_config* cfg) {
    if (cfg == nullptr || n_obj <= 0) return 256;
    Bump b{nullptr, 0, 0};
    return carve_trunk(b, n_obj, *cfg, nullptr) + 256;
}

int t2p_pointnet2_forward(const float* xyz, const float* rgb, int64_t n_obj, const t2p_cell_weights* w, const t2p_cell_config* cfg,
                          const float* head_w, const float* head_b, int32_t n_classes, int32_t n_colors, float* features0,
                          float* features1, float* features2, float* class_pred, float* color_pred, void* workspace,
                          size_t workspace_bytes, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(cfg != nullptr && w != nullptr, "pointnet2_forward: NULL argument");
    T2P_TRY(check_n_pts(*cfg));
    T2P_TRY(check_plan(*cfg));
    T2P_CHECK_ARG(n_obj >= 0, "pointnet2_forward: negative size");
    T2P_CHECK_ARG(n_obj <= T2P_MAX_CHUNK_OBJECTS,
                  "pointnet2_forward: %lld objects in one batch; the batch is one cell, limited to %d objects", (long long)n_obj,
                  T2P_MAX_CHUNK_OBJECTS);
    const bool heads = head_w != nullptr;
    if (heads) {
        T2P_CHECK_ARG(head_b != nullptr && class_pred != nullptr && color_pred != nullptr,
                      "pointnet2_forward: the heads need head_b, class_pred and color_pred");
        if (n_classes < 1 || n_classes > 64 || n_colors < 1 || n_colors > 64) {
            set_error("pointnet2_forward: n_classes=%d / n_colors=%d outside [1, 64]", n_classes, n_colors);
            return T2P_E_UNSUPPORTED;
        }
    }
    if (n_obj == 0) return 0;
    T2P_CHECK_ARG(xyz != nullptr && rgb != nullptr && workspace != nullptr, "pointnet2_forward: NULL argument");
    T2P_TRY(check_x3_weights("pointnet2_forward", *w, *cfg));
    T2P_CHECK_ARG((((uintptr_t)xyz | (uintptr_t)rgb | (uintptr_t)workspace) & 15) == 0,
                  "pointnet2_forward: xyz, rgb and workspace must be 16-byte aligned");
    Bump b{(char*)workspace, 0, workspace_bytes};
    CellWs ws;
    const size_t need = carve_trunk(b, n_obj, *cfg, &ws);
    if (need > workspace_bytes) {
        set_error("pointnet2_forward: workspace %zu B < %zu B needed for %lld objects", workspace_bytes, need, (long long)n_obj);
        return T2P_E_WORKSPACE;
    }
    t2p_cell_trace tr{};
    tr.features0 = features0;
    tr.features1 = features1;
    tr.features2 = features2;
    const Chunk c(st, n_obj, 1, *cfg, *w, ws);
    T2P_TRY(launch_one_cell_index(n_obj, ws.seg_ptr, ws.first, st, c.guard));
    T2P_TRY(c.trunk(xyz, rgb, false));
    T2P_TRY(c.guard_check());
    T2P_TRY(c.copy_traces(tr, 0, 0, true, nullptr));
    if (heads)   // (on the workspace's copy of features2: the caller need not ask for it)
        T2P_TRY(launch_classifier_heads(ws.f2, head_w, head_b, n_obj, n_classes, n_colors, class_pred, color_pred, st));
    return 0;
}

// ---- row-list exports ---------------------------------------------------------------------------------------------------

int t2p_sample_group(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host,
                     uint8_t* const* fps_idx, uint8_t* const* nbr, uint8_t* const* cnt, t2p_stream_t stream) {
    T2P_CHECK_ARG(xyz && radius_host && fps_idx && nbr && cnt, "sample_group: NULL argument");
    GroupTables gt;
    T2P_TRY(fill_group_tables("sample_group", gt, n_pts, 0, 0, fps_idx, nullptr, nullptr, nbr, cnt));
    return launch_sample_group(xyz, n_obj, n_pts, radius_host, gt, (hipStream_t)stream);
}

int t2p_group_rows(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host, int32_t self_loops,
                   uint8_t* const* fps_idx, uint16_t* const* rows, uint16_t* const* n_rows, t2p_stream_t stream) {
    return group_rows("group_rows", xyz, n_obj, n_pts, radius_host, self_loops, 0, fps_idx, rows, n_rows, stream);
}

int t2p_group_rows_shared(const float* xyz, int64_t n_obj, int32_t n_pts, const float* radius_host, int32_t self_loops,
                          int32_t share_mask, uint8_t* const* fps_idx, uint16_t* const* rows, uint16_t* const* n_rows,
                          t2p_stream_t stream) {
    return group_rows("group_rows_shared", xyz, n_obj, n_pts, radius_host, self_loops, share_mask, fps_idx, rows, n_rows, stream);
}

int t2p_group_rows_built(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, const float* radius_host,
                         int32_t self_loops, int32_t share_mask, uint8_t* const* fps_idx, uint16_t* const* rows,
                         uint16_t* const* n_rows, t2p_stream_t stream) {
    return group_rows_built("group_rows_built", xyz, rgb, n_obj, n_pts, radius_host, self_loops, share_mask, 0, fps_idx, rows, n_rows, stream);
}

int t2p_group_rows_pruned(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, const float* radius_host,
                          int32_t self_loops, int32_t share_mask, uint8_t* const* fps_idx, uint16_t* const* rows,
                          uint16_t* const* n_rows, t2p_stream_t stream) {
    return group_rows_built("group_rows_pruned", xyz, rgb, n_obj, n_pts, radius_host, self_loops, share_mask, 1, fps_idx, rows, n_rows, stream);
}

}  // extern "C"
