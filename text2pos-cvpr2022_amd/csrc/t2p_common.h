// Internal helpers shared by the gfx950 kernels of libt2p_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

namespace t2p {

void set_error(const char* fmt, ...);

// All launch wrappers return 0 on success, a hipError_t (>0) on a HIP failure or a negative
// T2P_E_* code on an argument error; the message is kept for t2p_last_error().
#define T2P_E_ARG (-1)
#define T2P_E_WORKSPACE (-2)
#define T2P_E_UNSUPPORTED (-3)

#define T2P_CHECK_ARG(cond, ...)                  \
    do {                                          \
        if (!(cond)) {                            \
            ::t2p::set_error(__VA_ARGS__);        \
            return T2P_E_ARG;                     \
        }                                         \
    } while (0)

#define T2P_CHECK_LAUNCH(name)                                                   \
    do {                                                                         \
        hipError_t e__ = hipGetLastError();                                      \
        if (e__ != hipSuccess) {                                                 \
            ::t2p::set_error("%s: launch failed: %s", name, hipGetErrorString(e__)); \
            return (int)e__;                                                     \
        }                                                                        \
    } while (0)

#define T2P_TRY(expr)             \
    do {                          \
        int rc__ = (expr);        \
        if (rc__ != 0) return rc__; \
    } while (0)

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));
typedef __fp16 fp16x2 __attribute__((ext_vector_type(2)));

// fp32 pair -> packed fp16 pair, round to NEAREST even (gfx950's v_cvt_pk_f16_f32; the f16x3 split x = hi + lo then carries
// |error| <= 2^-22 |x| - v_cvt_pkrtz_f16_f32, round toward zero, leaves 2^-20 and a bias that adds up along k).
__device__ __forceinline__ fp16x2 cvt_pk_f16(float a, float b) {
    typedef float f32x2_ __attribute__((ext_vector_type(2)));
    typedef _Float16 h16x2_ __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(fp16x2, __builtin_convertvector((f32x2_){a, b}, h16x2_));
}
// v - (float)h[SEL] in one VALU op (exact): the fp32 difference behind the low piece of the f16x3 split, as a stand-alone statement
template <int SEL>
__device__ __forceinline__ float sub_half(float v, fp16x2 h) {
    float r;
    if constexpr (SEL == 0)
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[0,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(v));
    else
        asm("v_fma_mix_f32 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "=v"(r) : "v"(h), "v"(v));
    return r;
}
// Low piece of the f16x3 split of a pair: fp16(v0 - hi[0]) | fp16(v1 - hi[1]) << 16, the two differences formed exactly in fp32
// by v_fma_mix_f32 (hi half extended, times -1, plus v).  ONE asm statement: behind a stand-alone inline-asm v_fma_mix hipcc puts an
// s_nop in front of the dependent v_cvt_pk (it cannot see that the asm writes whole dwords) - one wait state per pair, in the
// staging arithmetic that rides beside the MFMA stream of the SA kernels.
// CAUTION (round 6, found the hard way): gfx950 needs two wait states between a VALU write of a VGPR and an MFMA that reads it as its
// A / B operand.  hipcc guarantees them between instructions it KNOWS; an asm statement is one opaque non-VALU instruction to its hazard
// recogniser, so nothing separates this statement's final v_cvt_pk from an MFMA that consumes `lo` next.  In k_sa_points the merged
// statement sat one instruction in front of the MFMA that read the four lo registers: SA1 outputs ~1e4 off (libt2p_hip_s1a; a
// different register assignment, s1b, happened to put two instructions between and passed).  Use it only where the consumer is an LDS /
// global store (k_sa3) or is provably far away (k_sa_rows: the pieces of step s + 1 are converted during step s and first multiplied in
// step s + 1, behind an explicit s_nop - see mfma_w there); k_sa_points and k_gemm_x3 keep the separate statements, behind which
// hipcc's own v_cvt_pk -> MFMA spacing applies.  (`lo` is an early-clobber output as well: it then never shares a register with an input.)
__device__ __forceinline__ uint32_t split_lo_pk(fp16x2 hi, float v0, float v1) {
    uint32_t lo;
    float t0, t1;
    asm("v_fma_mix_f32 %1, %3, -1.0, %4 op_sel:[0,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_fma_mix_f32 %2, %3, -1.0, %5 op_sel:[1,0,0] op_sel_hi:[1,0,0]\n\t"
        "v_cvt_pk_f16_f32 %0, %1, %2"
        : "=&v"(lo), "=&v"(t0), "=&v"(t1) : "v"(hi), "v"(v0), "v"(v1));
    return lo;
}
// workgroup barrier that orders LDS traffic only (no vmcnt: loads and LDS-DMA pieces in flight survive it)
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
// Sum over the wavefront's 64 lanes by the xor butterfly 32, 16, ... 1: the same tree every time.  Every lane must call it, all
// receive the sum.
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}
typedef double f64x4 __attribute__((ext_vector_type(4)));

int num_cus();  // cached multiProcessorCount of the current device
int matrix_wgs(); // workgroups of the persistent matrix kernels (= num_cus() unless T2P_MATRIX_WGS says otherwise)
// hipFuncAttributeMaxDynamicSharedMemorySize is a per-DEVICE attribute of a kernel: set once per (device, kernel), under a
// lock; returns 0 or the hipError_t (message kept for t2p_last_error)
int reserve_lds(const void* kernel, size_t bytes, const char* what);

// Caller-provided workspaces are carved by bumping a 256-byte-aligned offset; base == nullptr only measures
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
struct Bump {
    char* base;
    size_t off, cap;
    template <typename T>
    T* take(size_t n) {
        off = align_up(off, 256);
        T* p = (T*)(base ? base + off : nullptr);
        off += n * sizeof(T);
        return p;
    }
};

// ---- fp16-range guard of the f16x3 path -------------------------------------------------------------------------
// The split-precision path converts fp32 activations to fp16 (hi = fp16(v) to nearest: a value past 65504 would
// become inf).  Every kernel that performs such a conversion reports the largest magnitude it converted into one
// of these per-chunk device words (float bits, atomicMax on the unsigned pattern); k_guard_check turns them into the
// caller's sticky overflow flag.  The SA edge kernels convert relu(A_j - B_i) and are covered by the bound
// max|A_l| + max|B_l| taken where the tables are produced, so their inner loop carries no check.
enum GuardSlot {
    G_INPUT = 0,               // max(|xyz|, |rgb|) of the call's inputs when above 1 (normalised inputs: never published).
                               // Bounds the geometry-only layer-1 tables: |B_l| <= ||W1p_l||_1 max|xyz|,
                               // |A_1| <= ||W1_1||_1 max(|rgb|, |xyz|) + max|b1|
    G_A2 = 2, G_A3 = 4,        // layer-1 point tables of SA levels 2 and 3, reported by the dense kernels that write them
    G_F1 = 6, G_F2 = 7, G_F3 = 8,  // SA outputs F_l = the rows the dense weight-stationary kernels split on the fly; exact
                                   // maxima, reported by the SA kernels (their xyz tail is bounded by 1).  GA layer 1's
                                   // output (handed on as fp16 planes) is bounded by ||W||_1 max(F_3, 1) + max|b|
    G_GEMM_IN = 9,    // unit-norm rows split on the fly by the LDS-tiled f16x3 GEMM (cat, emb): high side only
    // exact maxima of the stages that are split on the fly downstream of the SA levels, one slot each (a warm stage must not
    // hide a cold one): GA layer 1's output (the fp16 planes GA2 reads), the PointNet2 features f0 / f1 / f2 as the LDS-tiled
    // f16x3 GEMMs split them (lin1, lin2, mlp_pointnet), and the kNN edge rows relu(P_i + Q_j) of DynamicEdgeConv
    G_GA_H = 10, G_PN_F0 = 11, G_PN_F1 = 12, G_PN_F2 = 13, G_EDGE = 14,
    G_SLOTS = 16
};
struct GuardBounds {   // host-side norms of the folded weights (packing.py), passed by value to k_guard_check
    float wp_l1[3];     // per SA level: max over columns of |W1p[0][c]| + |W1p[1][c]| + |W1p[2][c]|
    float a1_l1;        // SA1 layer 1 over all 6 inputs: max over columns of sum_k |W1[k][c]|
    float a1_bmax;      // max |b1| of SA1
    float ga1_l1;       // GA layer 1: max over columns of sum_k |W[k][c]|
    float ga1_bmax;
};
// High side of SA levels 2 and 3: k_guard_check counts the point table's maximum as at least kGuardFloor (a margin far above
// the activations of a trained, batch-normalised network, O(1..100)).
constexpr float kGuardFloor = 16384.f;
// Low side: fp16 pieces hi = fp16(v), lo = fp16(v - hi) carry an ABSOLUTE error of ~2^-25 (fp16's subnormal spacing) once
// |v| < 2^-3; harmless while a layer's largest activations are O(1), but a layer whose LARGEST magnitude is below 2^-7 keeps
// fewer than ~18 bits of its own scale (and below 2^-14 the hi piece itself goes subnormal).  k_guard_check sets bit 7 then,
// for every stage with an exact maximum (SA outputs, the layer-1 tables of SA levels 2 and 3, and slots G_GA_H .. G_EDGE).
constexpr float kGuardTiny = 0.0078125f;
#ifdef __HIPCC__
// m >= 0 (a magnitude; NaN compares false everywhere and is caught by the table producers' own inputs); at most one
// atomic per wavefront, and only when some lane saw a magnitude above the floor
__device__ __forceinline__ void guard_publish_above(uint32_t* slot, float m, float floor_) {
    if (slot == nullptr) return;
    if (!__any(m > floor_)) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) atomicMax(slot, __float_as_uint(m));
}
// The same on the bit pattern of a magnitude (|v| as an unsigned integer; NaN patterns are the largest and DO get published)
__device__ __forceinline__ void guard_publish_bits_above(uint32_t* slot, uint32_t bits, uint32_t floor_bits) {
    if (slot == nullptr) return;
    if (!__any(bits > floor_bits)) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)bits, o, 64);
        bits = other > bits ? other : bits;
    }
    if ((threadIdx.x & 63) == 0) atomicMax(slot, bits);
}
// Exact running maximum without a floor, for sites that report once per wave (or rarely): the wave's maximum goes to the slot
// only when it exceeds what the slot already holds (a relaxed load first: after the first few waves almost no atomic is left).
// The exact maxima also serve the LOW side of the guard (k_guard_check: a level whose largest magnitude is below kGuardTiny
// would put the hi pieces of its activations into fp16's subnormals and lose the lo pieces altogether).
__device__ __forceinline__ void guard_publish_exact(uint32_t* slot, float m) {
    if (slot == nullptr) return;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) {
        const uint32_t b = __float_as_uint(m);
        if (b > __atomic_load_n(slot, __ATOMIC_RELAXED)) atomicMax(slot, b);
    }
}
// Exact form for the persistent SA kernels: `acc` is a wave-uniform bit pattern (an SGPR) that lives across the whole
// launch; guard_flush publishes it once per wave at the end (no floor, no contention: ~2 k atomics per launch).
__device__ __forceinline__ void guard_track_bits(uint32_t& acc, int lane_bits /* pattern of a non-negative float */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const int other = __shfl_xor(lane_bits, o, 64);
        lane_bits = other > lane_bits ? other : lane_bits;
    }
    const uint32_t b = (uint32_t)__builtin_amdgcn_readfirstlane(lane_bits);
    acc = b > acc ? b : acc;
}
#endif
int launch_guard_check(const uint32_t* guard, int32_t* overflow_flag, const GuardBounds& b, hipStream_t st);  // small_kernels.hip

// Opt-in per-kernel timing (t2p_profile_enable): brackets a launch with hipEvents on the launch stream.
struct ProfScope {
    ProfScope(const char* name, hipStream_t st);
    ~ProfScope();
    int slot;
    hipStream_t st;
    void* ev_end;  // hipEvent_t recorded by the destructor
    int reps;      // 1, or t2p_profile_repeat's count for this scope: the launch sites of the large kernels issue their launch
                   // `reps` times back to back (same arguments: every one of them rewrites its outputs from its inputs), which
                   // is how profiles/energy_table.py holds ONE kernel on the chip for seconds under the power sampler
};
#define T2P_REPEAT(ps) for (int rep_ = (ps).reps; rep_ > 0; --rep_)

// ---- sample_group.hip -------------------------------------------------------------------------------------
// Compact per-object group tables produced by the fused FPS + ball-query kernel.
// Level l (0..2): n_dense[l] dense points -> n_cent[l] = ceil(n_dense[l]/2) centroids; indices are LOCAL to the
// object and refer to the level's dense ordering (level 0: input order; level l>0: FPS order of level l-1).
struct GroupTables {
    uint8_t* fps_idx[3];  // [n_obj, n_cent[l]]
    uint8_t* nbr[3];      // [n_obj, n_cent[l], 32]
    uint8_t* cnt[3];      // [n_obj, n_cent[l]]
    // compact edge-row lists consumed by the SA edge kernel (nullptr = not wanted):
    uint16_t* rows[3];    // [n_obj, n_cent[l]*33]  (centroid | self-loop flag 0x80) << 8 | source index, sorted by centroid
    uint16_t* n_rows[3];  // [n_obj] rows in the list (ball-query hits + one self loop per centroid when self_loops)
    int self_loops;
    // share_tail[l] != 0 (level index 1 = SA level 2 of the 256-point fast path only; level_fast): the object's TAIL centroids - c > 0 with
    // fps_idx[c] == 0: FPS has run out of distinct positions and picks point 0 again, for the rest of the level - share one copy of
    // their ball-query hits.  A tail centroid stands at centroid 0's position, so its hits are centroid 0's hits and each of its
    // edge rows relu(A_j - B_c) is centroid 0's, bit for bit; only its self-loop row (dense row `c` of the cell's batch) is its
    // own.  The first tail centroid's hits are listed ONCE under the pseudo-centroid code kSaTailCode (a shared
    // accumulator slot whose B row is centroid 0's), every tail centroid keeps its self-loop row, and the consumer's drain takes
    // max(acc[c], acc[code]) for tail centroids.  The list is then no longer sorted by centroid.
    int share_tail[3];
    // prune_dup[l] != 0 (level index 1 and 2, mask-mode plan of the 256-point fast path only): rows whose SOURCE is a dense point
    // j >= k_prev leave the list, the shared copy of level index 1's tail rows included; self-loop rows stay.  k1 = level 0's first
    // tail centroid; k_prev = k1 at level index 1, min(k1, 64) at level index 2 (its dense points are the prefix of level 1's
    // picks, so its tail starts at k1 too).  Such a point is a tail centroid of the level below: it stands at dense point 0's
    // position and its feature row is row 0's bit for bit, so its table row A_j is A_0; dense point 0 is in range whenever j is
    // and is first in index order, always inside the 32-cap, so relu(A_j - B_i) W2 repeats a row centroid i already has.  The
    // repeats are a suffix of the index order: "first 32 hits, then drop them" is "first 32 hits among j < k_prev".
    // "Row 0's features" holds WITHOUT self-loop rows only (a self-loop row reads another object's dense row, so with them every
    // tail centroid's output row is its own): Chunk::group sets the field only then.
    int prune_dup[3];
    // mask_l0 != 0 (256-point fast path only): level 0 leaves no list.  The kernel writes each centroid's point-ordered 256-bit
    // hit mask, [centroid][4 x u64], to the start of the object's rows[0] slice (4,096 of its 8,448 bytes) - up to the first
    // tail centroid, where it stops - and n_rows[0] is not written.  launch_build_rows turns the masks into the final list.
    int mask_l0;
    int n_dense[3];
    int n_cent[3];
    // Optional layer-1 tables written by the same kernel (it is VALU-bound and leaves the memory pipes idle; as separate
    // kernels these tables were pure HBM-write time).  B[l] = nullptr / A1 = nullptr: not wanted.
    float* B[3];            // centroid tables  B_l[o*n_cent + c][H_l] = W1p_l pos_c
    const float* wp[3];     // [3][H_l] position rows of the level's layer-1 weights
    int H[3];
    float* tail[3];         // SA output rows F_l: the [xyz | 0] quad at column tail_col0[l]; the 28 pad columns behind it are never written, their readers mask them (WsParams::k_live) (row stride ld_tail[l])
    int ld_tail[3], tail_col0[3];
    int tail_rows[3];       // rows per object of the tail table (0 = n_cent); rows past n_cent repeat centroid n_cent - 1
    float* A1;              // SA1 point table A_1[o*n_pts + j][H1] = W1 [rgb_j | xyz_j] + b1
    const float* w1;        // [6][H1]
    const float* b1;
    const float* rgb;       // [n_obj][n_pts][3]
    int H1;
    uint32_t* guard;        // nullptr, or the chunk's GuardSlot words (the input magnitude is reported here)
};
int launch_sample_group(const float* xyz, int64_t n_obj, int n_pts, const float radius[3], GroupTables gt,
                        hipStream_t st);
// Drops from level 0's compact row lists the edges of points that repeat an earlier point of their object bit for bit
// (identical message, so the max-aggregate is unchanged); updates n_rows.  rows [n_obj][n_cent * 33], n_pts = 256.
int launch_dedup_rows(const float* xyz, const float* rgb, int64_t n_obj, int n_pts, uint16_t* rows, uint16_t* n_rows,
                      int n_cent, hipStream_t st);
// Level 0's final row lists from the hit masks of a launch_sample_group with mask_l0 (same stream, directly behind it, same gt):
// the list launch_sample_group + launch_dedup_rows leave, bit for bit; writes n_rows[0].  It also runs the ball queries of levels
// 2 and 3, which the mask-mode scan leaves out (their centroids are the prefix of level 1's picks): rows / n_rows of level index
// 1 and 2 in the form share_tail[1] and prune_dup ask for.  n_pts = 256.
int launch_build_rows(const float* xyz, const float* rgb, int64_t n_obj, int n_pts, const float radius[3], const GroupTables& gt,
                      hipStream_t st);

// ---- tables.hip / small kernels ------------------------------------------------------------------------------
// gather level-l centroid positions: out[(o*n_cent + c), 0..2]
int launch_rownorm(const float* in, int ld_in, int64_t n_rows, int dim, float* out, int ld_out, int col0,
                   hipStream_t st);
int launch_gather_rownorm(const float* table, const int32_t* idx, int64_t n_rows, int dim, float* out, int ld_out,
                          int col0, hipStream_t st);
// first_nbr: k_knn's table of the same rows (an object without a first neighbour holds a NaN: its cell's pooled row is NaN)
int launch_segmax(const float* in, int dim, const int32_t* seg_ptr, int n_seg, float* out, int mean,
                  hipStream_t st, const int32_t* first_nbr = nullptr, int knn_k = 0, uint32_t* guard_input = nullptr);
int launch_knn(const float* x, int dim, const int32_t* seg_ptr, int n_seg, int max_seg_rows, int k,
               int32_t* out_idx, hipStream_t st);
// 3 -> 64 -> D MLP (BN folded, ReLU after both layers) + F.normalize, written into out[row*ld_out + col0 ...]
int launch_mlp3_norm(const float* in3, int64_t n_rows, const float* w1, const float* b1, const float* w2,
                     const float* b2, int D, float* out, int ld_out, int col0, hipStream_t st);
// chunk-local cell index arrays: seg_ptr_local[c] = cell_ptr[c] - o_lo (c = 0..n_cells), first[o] = start of o's cell
int launch_pack_objects(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* sample_idx,
                        const float* rot, int64_t n_obj, int n_pts, float* xyz, float* rgb, float* center, float* mean_rgb,
                        hipStream_t st);
int launch_pack_scene(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* obj_id, const uint64_t* key,
                      const float* scene_center, const float* scene_color, int64_t n_out, int n_pts, float* xyz, float* rgb,
                      float* center, float* mean_rgb, int32_t* idx_out, hipStream_t st);
int launch_pack_scene_aug(const float* raw_xyz, const float* raw_rgb, const float* raw_mirror_xy, const int32_t* obj_ptr,
                          const int32_t* obj_id, const uint64_t* key, const uint8_t* flip, const float* rot, const float* scene_center,
                          const float* center_mirror_xy, const float* scene_color, int64_t n_out, int n_pts, float* xyz, float* rgb,
                          float* center, float* mean_rgb, int32_t* idx_out, hipStream_t st);
int launch_pairwise_ranking(const float* scores, int batch, float margin, float* row_loss, float* d_scores, float* row_cnt,
                            hipStream_t st);
int launch_hardest_ranking(const float* scores, int batch, float margin, float* best, int32_t* where, float* d_scores,
                           hipStream_t st);
int launch_cell_index(const int32_t* cell_ptr, int n_cells, int32_t o_lo, int32_t* seg_ptr_local, int32_t* first,
                      hipStream_t st, uint32_t* guard_to_clear = nullptr);

// ---- tg_gemm.hip: generic tiled fp32-MFMA GEMM ------------------------------------------------------------
// C[M, N] (ldc, column offset c0) = act(A[M, K] (lda) * W[K, N] (row-major, ldw = N) + bias[N])
int launch_gemm(const float* A, int lda, const float* W, const float* bias, float* C, int ldc, int c0, int64_t M,
                int K, int N, int relu, hipStream_t st, const float* resid = nullptr, int ldr = 0);
// few rows x long K, no epilogue (tg_gemm.hip): the per-step products of the training-mode LSTM; K a multiple of 4, any N
int launch_gemm_skinny(const float* A, int lda, const float* W, float* C, int ldc, int64_t M, int K, int N, hipStream_t st);
// tg_gemm_x3.hip: the same contract on the f16x3 matrix path (W as the image of packing.py::pack_gemm_x3)
int launch_gemm_x3(const float* A, int lda, const void* Wx, float scale, const float* bias, float* C, int ldc, int c0,
                   int64_t M, int K, int N, int relu, hipStream_t st, const float* resid = nullptr, int ldr = 0,
                   uint32_t* amax_in = nullptr /* f16x3 guard word for the rows of A */);
// One dense layer's weights: the k-major fp32 matrix w, or (x3 != nullptr) its pack_gemm_x3 image and the image's scale.  The
// path is chosen where the descriptor is built; every call site is one launch_dense (amax_in goes to the f16x3 kernel only).
struct DenseW { const float* w; const void* x3; float scale; };   // x3 == nullptr: fp32-MFMA path
inline int launch_dense(const float* A, int lda, const DenseW& W, const float* bias, float* C, int ldc, int c0, int64_t M, int K, int N,
                        int relu, hipStream_t st, const float* resid = nullptr, int ldr = 0, uint32_t* amax_in = nullptr) {
    if (W.x3 != nullptr) return launch_gemm_x3(A, lda, W.x3, W.scale, bias, C, ldc, c0, M, K, N, relu, st, resid, ldr, amax_in);
    return launch_gemm(A, lda, W.w, bias, C, ldc, c0, M, K, N, relu, st, resid, ldr);
}

// tg_gemm_tn.hip: C[K1, N] = A[M, K1]^T B[M, N], rows split over the grid + fixed-order reduction (training-mode gradients)
size_t gemm_tn_workspace_bytes(int64_t M, int K1, int N);
// train_ops.hip: PointConv edge lists (source row, target row) of a level from k_sample_group's compact row lists
int launch_edge_counts(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, int64_t n_obj, int n_dense, int n_cent,
                       int self_loops, int32_t* counts, hipStream_t st);
int launch_edge_expand(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, const int32_t* cent_ptr, int64_t n_obj,
                       int n_dense, int n_cent, int self_loops, int32_t* src, int32_t* dst, hipStream_t st);
// train_gemm.hip: weight + bias gradient of the training-mode Linear layers
size_t linear_wgrad_workspace_bytes(int64_t M, int K1, int N);
int launch_linear_wgrad_f32(const float* dY, int lda, const float* X, int ldb, float* dW, int ldc, float* colsum, int64_t M, int K1, int N,
                            void* ws, size_t ws_bytes, hipStream_t st);
int launch_gemm_tn(const float* A, int lda, const float* B, int ldb, float* C, int ldc, int64_t M, int K1, int N, void* ws,
                   size_t ws_bytes, hipStream_t st);

// ---- ws_gemm.hip: weight-stationary streaming fp32-MFMA kernels ---------------------------------------------
enum WsMode { WS_DENSE_STORE = 0, WS_DENSE_GROUPMAX = 1, WS_EDGE_KNN = 3 };
struct WsParams {
    // operand tables
    const float* A;    // source rows [n_src, lda]   (dense: the GEMM's A; edge: layer-1 point table)
    int lda;
    int k_live;        // dense fp32 rows: columns >= k_live (a multiple of 4; 0 = all K) are taken as zero and never read
    const float* Bc;   // edge modes: per-destination term [n_dst, H]
    const float* W;    // [K][ldw] k-major weights (BN folded)
    int ldw;
    const void* W_x3;  // nullptr, or the packed f16x3 register image of the whole [K][ldw] matrix (dense modes)
    // f16x3 only: activations may travel between two dense kernels already split into fp16 hi / lo planes
    const void* A_hi;  // non-null: A is given as two [M][lda] fp16 planes (no conversion while staging)
    const void* A_lo;
    void* out_hi;      // non-null (DENSE_STORE): write the result as two [M][ldo] fp16 planes instead of fp32
    void* out_lo;
    const float* bias; // [N]
    float* out;        // dense_store: [M, ldo]; groupmax: [n_groups, ldo]; edge: [n_dst, ldo]
    int ldo;
    int relu;
    int64_t n_groups;  // dense: ceil(M / rows_per_group); edge SA: objects; edge kNN: ceil(n_dst/32)
    int64_t M;         // dense: total rows
    // edge kNN
    uint32_t* amax_out;     // f16x3 guard (nullable): largest output magnitude (a table the SA kernels split, or fp16 planes)
    const int32_t* knn_idx; // [n_dst, knn_k] (-1 = absent)
    int knn_k;
    int64_t n_dst;
    int mean;               // 0 = max aggregation, 1 = mean (needs knn_k == 8)
    int knn_group;          // destinations per group: 32 (0 = 32), or 8 for calls too small to fill the CUs with 32-destination groups
    int group_rows;         // DENSE_GROUPMAX: rows per max group, 1, 2, 4, 8, 16 or 32 (0 = 32); M is a multiple of it
};
int launch_ws(int mode, int K, int N, const WsParams& p, hipStream_t st);

// ---- ws_sa.hip: the set-abstraction edge kernel (flattened, fully pipelined batch stream) ----------------------------
struct SaParams {
    const float* A;   // layer-1 point table [n_obj*n_dense][H]
    const float* Bc;  // centroid table [n_obj*n_cent][H] (unused when wp is given)
    const float* wp;  // nullptr, or the [3][H] position rows of the layer-1 weights: the f16x3 kernel then builds each object's
                      // centroid table B_i = W1p pos_i in LDS itself (pos_i from the [xyz | 0] tail of the `out` rows)
    const float* W;   // [H][C] k-major (fp32 MFMA path)
    const void* W_x3; // nullptr, or the host-packed f16x3 register image of W (selects the split-precision path)
    const float* bias;  // [C]; the f16x3 path takes it pre-multiplied by the weight image's scale
    float out_scale;    // f16x3: 1 / scale of the weight image (results are drained as acc * out_scale); fp32: 1
    float* out;       // [n_obj*n_cent][ldo] rows = [features C | centroid xyz 0 | pad] (this kernel writes the features)
    int ldo;
    const uint16_t* rows;    // GroupTables::rows[l]
    const uint16_t* n_rows;  // GroupTables::n_rows[l]
    const int32_t* first;    // [n_obj] first object of the object's cell (self-loop aliasing)
    const uint8_t* fps_idx;  // [n_obj][n_cent]
    const float* pos_src;    // rows holding the dense positions of this level
    int ld_pos, pos_col0;
    const float* feat_src;   // sa_points.hip (level 1 only): the points' features [n_obj*n_dense][3] (rgb), the whole layer-1
    const float* w1;         // weight matrix [6][H] (feature rows, then position rows) and its bias [H]; nullptr: the kernels
    const float* b1;         // that gather the point table A
    int n_dense, n_cent;
    int64_t n_obj;
    int32_t* prefix_ws;      // [n_obj+1] scratch (tile prefix sums)
    int32_t* bounds_ws;      // [n_workgroups+1] scratch (balanced contiguous object ranges)
    int balanced;            // 1: bounds_ws was filled by launch_sa_balance_levels for this level's launch shape
    uint32_t* amax_out;      // f16x3 guard (nullable): largest output magnitude (the next dense kernel splits these rows)
    int out_rows;            // output rows per object (0 = n_cent); rows past n_cent repeat centroid n_cent - 1 (the stream kernel of ws_sa.hip)
};
int launch_ws_sa(int H, int C, const SaParams& p, hipStream_t st);
// k_balance alone, for a kernel launched outside launch_sa_balance_levels (p.balanced == 0)
int launch_sa_balance(const SaParams& p, int tile_rows, int n_wg, hipStream_t st);
// the same launch on bare arrays (t2p_sa_balance): prefix [n + 1], bounds [n_wg + 1]
int launch_sa_balance_arrays(const uint16_t* n_rows, int n, int tile_rows, int n_wg, int32_t* prefix, int32_t* bounds, hipStream_t st);
// Pseudo-centroid code of the shared tail rows (GroupTables::share_tail) in the centroid byte of a row of SA level 2: 64, the
// first free value of the 7-bit field behind its 64 centroids; 64 * C * 4 fits the u16 accumulator offsets of k_sa_rows.
constexpr int kSaTailCode = 64;
// sa_rows.hip: row-owning f16x3 kernel of SA level 2 (H = C = 128, LDS centroid table): true when launch_ws_sa routes p there
bool sa_rows_selected(int H, int C, const SaParams& p);
int launch_sa_rows(int H, int C, const SaParams& p, hipStream_t st);
int sa_rows_launch_shape(int64_t n_obj, int* tile_rows, int* n_wg);
// sa_points.hip: both layers per edge from the object's points in LDS, f16x3 kernel of SA level 1 (needs wp, w1, b1, feat_src)
bool sa_points_selected(int H, int C, const SaParams& p);
int launch_sa_points(int H, int C, const SaParams& p, hipStream_t st);
int sa_points_launch_shape(int64_t n_obj, int* tile_rows, int* n_wg);
// sa3.hip: SA level 3 (H = C = 256, LDS centroid table), column-slice waves with scalar per-row control
bool sa3_selected(int H, int C, const SaParams& p);
int launch_sa3(const SaParams& p, hipStream_t st);
int sa3_launch_shape(int64_t n_obj, int* tile_rows, int* n_wg);
// Whether level l's row lists may share the rows of repeated (tail) centroids: only k_sa_rows (level index 1) owns the extra
// accumulator slot, only the 256-point fast path of k_sample_group writes the shared form, and tuning bit 0x4 keeps the full
// lists.  p: the level's SaParams as launch_ws_sa will see them (W_x3, wp, n_dense, n_cent).
inline bool sa_shares_tail_rows(int l, int H, int C, const SaParams& p, int n_pts, int tuning) {
    return l == 1 && n_pts == 256 && !(tuning & 4) && p.n_dense == 128 && p.n_cent == 64 && sa_rows_selected(H, C, p);
}
// One launch that balances all three levels (their row counts are known once k_sample_group has run); fills
// prefix_ws / bounds_ws of every p[l] for the launch shape launch_ws_sa(H[l], C[l], p[l]) will use.
int launch_sa_balance_levels(const SaParams p[3], const int H[3], const int C[3], hipStream_t st);

// ---- lstm.hip ---------------------------------------------------------------------------------------------
// gate_table: [2][V][4D] with V = vocabulary + 1: the LAST row of each direction is all zeros (what rows past their length
// gather); the f16x3 path scales the table in place by whh_scale.
int launch_bilstm_impl(const float* gate_table /*[2][V][4D]*/, const float* whh /*[2][D][4D] k-major*/,
                       const void* whh_x3 /*nullable: [2 dirs] scaled f16x3 images of whh (selects the f16x3 recurrence)*/,
                       float whh_scale, const int32_t* tokens /*[B, T]*/, const int32_t* lengths, int B, int T, int V, int D,
                       float* hdir_ws /*[2][B][D]*/, float* out /*[B, D] mean of the two final hidden states*/,
                       hipStream_t st);

int launch_lstm_cell_fwd(const float* pre, const float* table, const int32_t* tokens, const int32_t* lengths, int64_t B, int T,
                         int D, int step, int reverse, const float* c_prev, const float* h_prev, float* gates, float* c,
                         float* h, hipStream_t st);
int launch_lstm_cell_bwd(const float* dh_gemm, const float* dh_carry_in, const float* dc_in, const float* gates,
                         const float* c_prev, const float* c, const int32_t* lengths, int64_t B, int D, int step, float* d_pre,
                         float* dc_out, float* dh_carry_out, hipStream_t st);

// ---- train_ops.hip --------------------------------------------------------------------------------------------
size_t bn_train_workspace_bytes(int64_t rows, int n_seg, int C);
int launch_bn_relu_train_forward(const float* x, const int32_t* seg_ptr, int n_seg, int64_t rows, int C, const float* gamma,
                                 const float* beta, float eps, int relu, float* y, float* mean, float* invstd,
                                 float* var_unbiased, double* part, hipStream_t st);
int launch_bn_relu_train_backward(const float* dy, const float* x, const float* beta, const int32_t* seg_ptr, int n_seg,
                                  int64_t rows, int C, const float* mean, const float* invstd, const float* gamma, int relu,
                                  float* dx, float* dgamma_seg, float* dbeta_seg, double* part, hipStream_t st);
int launch_edge_feat_fwd(const float* x, const float* pos, const float* pos_c, const int32_t* src, const int32_t* dst, int64_t E,
                         int C, int W, float* out, hipStream_t st);
int launch_edge_feat_bwd(const float* dout, const int32_t* src, int64_t E, int C, int W, float* dx, hipStream_t st);
int launch_pair_feat_fwd(const float* x, const int32_t* tgt, const int32_t* src, int64_t E, int D, float* out, hipStream_t st);
int launch_pair_feat_bwd(const float* dout, const int32_t* tgt, const int32_t* src, int64_t E, int D, float* dx, hipStream_t st);
int launch_segment_mean(const float* x, const int32_t* seg_ptr, int n_seg, int C, float* out, hipStream_t st);
int launch_segment_mean_backward(const float* dout, const int32_t* seg_ptr, int n_seg, int C, float* dx, hipStream_t st);
int launch_rownorm_bwd(const float* x, const float* dy, int64_t n_rows, int dim, float* dx, hipStream_t st);
int launch_segment_max(const float* x, const int32_t* seg_ptr, int n_seg, int C, float* out, int32_t* arg, hipStream_t st);
int launch_segment_max_backward(const float* dout, const int32_t* arg, const int32_t* seg_ptr, int n_seg, int C, float* dx,
                                hipStream_t st);

// ---- classify.hip: PointNet++ pre-training (classifier heads, softmax cross-entropy) -----------------------------------------
int launch_classifier_heads(const float* f2, const float* w, const float* bias, int64_t n, int C1, int C2, float* class_pred,
                            float* color_pred, hipStream_t st);
int launch_softmax_xent(const float* logits, int ld, const int32_t* labels, int64_t n, int C, float* row_loss, float* d_logits,
                        int ldd, int32_t* correct, hipStream_t st);
// launch_cell_index for a batch that is ONE cell of n objects (no device cell_ptr needed)
int launch_one_cell_index(int64_t n, int32_t* seg_ptr_local, int32_t* first, hipStream_t st, uint32_t* guard_to_clear);

// ---- sim_topk.hip -----------------------------------------------------------------------------------------
size_t sim_topk_workspace_bytes(int64_t nq, int64_t nc, int k);
int launch_sim_topk(const float* Q, const float* C, int64_t nq, int64_t nc, int dim, int k, int64_t c_index_offset,
                    int64_t* out_idx, double* out_score, void* ws, size_t ws_bytes, hipStream_t st);
// pairs whose groups differ score -inf (query_group [nq], cell_group [nc]); same workspace as launch_sim_topk
int launch_sim_topk_grouped(const float* Q, const float* C, const int32_t* query_group, const int32_t* cell_group, int64_t nq,
                            int64_t nc, int dim, int k, int64_t c_index_offset, int64_t* out_idx, double* out_score, void* ws,
                            size_t ws_bytes, hipStream_t st);
// include/t2p_serve.h: pairs outside the query's prior (distance to the cell's box, group) score -inf; the geometry pointers are
// all given or all NULL, the group pointers likewise, not both sets NULL; same workspace as launch_sim_topk
int launch_sim_topk_prior(const float* Q, const float* C, const double* query_xy, const double* query_radius, const double* cell_box,
                          const int32_t* query_group, const int32_t* cell_group, int64_t nq, int64_t nc, int dim, int k,
                          int64_t c_index_offset, int64_t* out_idx, double* out_score, void* ws, size_t ws_bytes, hipStream_t st);

}  // namespace t2p
