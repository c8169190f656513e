// Set-abstraction edge kernel for sa1/sa2/sa3, one stream kernel for both arithmetic paths: per-edge
// ReLU(A_j - B_i) -> layer-2 GEMM -> max per centroid, at runtime n_dense / n_cent (n_cent * C <= 8192), for the three levels
// (H, C) = (32, 64), (128, 128), (256, 256).
// (reference: gnn.PointConv(local_nn)(x, (pos, pos[idx]), edge_index), models/pointcloud/pointnet2.py:31-35).
//
// k_sa_stream<..., X3 = false> is the exact-fp32 path (precision = "fp32": v_mfma_f32_32x32x2_f32 fma chains), for every object size.
// k_sa_stream<..., X3 = true> is the f16x3 path of every level whose shape is NOT one of the 256-point ones (pointnet_numpoints != 256):
// those run on the specialised kernels sa_points.hip / sa_rows.hip / sa3.hip (levels 1 / 2 / 3), which build their centroid tables in
// LDS; here the centroid table B comes from HBM (k_sample_group writes B_l when the LDS centroid table is off).  This file also keeps
// the range balancing and the kernel selection.
//
// Same arithmetic and register-resident weights as ws_gemm.hip (see the design notes there); this variant removes
// every per-object bubble of the generic edge path:
//   * the per-object edge-row lists come pre-compacted from the FPS/ball-query kernel (one u16 per row), so there is
//     no in-kernel enumeration / scan;
//   * a tiny balancing kernel gives every workgroup a CONTIGUOUS object range of (nearly) equal tile count, computed
//     from the row counts -- deterministic, no atomics, no tail imbalance;
//   * the workgroup walks its range as ONE flattened stream of row batches that crosses object boundaries, software
//     pipelined three deep:  row metadata (t+2)  ->  gathers of A_j / B_i rows (t+1)  ->  MFMA + segmented max (t),
//     with double-buffered LDS staging tiles and one barrier per batch;
//   * the per-object max accumulator is double-buffered in LDS too, so the finished object's [n_cent][C] block is
//     written to HBM (and re-zeroed) underneath the MFMAs of the next object's first batch.
// The two paths share all of that and differ at four places (if constexpr (X3) below):
//   * stationary weights: fp32 keeps a [K/2][32-column] slice of W per lane half; f16x3 keeps a 32-column slice of the scaled layer-2
//     image sa_w2_x3 as hi / lo planes (packing.py::pack_f16x3_scaled, register order: lane half u of MFMA step s holds
//     k = u K/2 + 8 s .. + 7);
//   * staging: fp32 writes the tile h = relu(A_j - B_i); f16x3 splits it into fp16 hi = fp16(h) and lo = fp16(h - hi) (both to
//     nearest) and writes two fp16 planes;
//   * MFMA block: fp32 chains; f16x3 runs hi.hi, hi.lo, lo.hi per step on v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator that
//     starts at the scaled bias;
//   * f16x3 publishes the level's exact output maximum (guard slot G_F1 + l), as the specialised kernels do.
// The drain multiplies by out_scale (f16x3: 1 / scale of the weight image) and writes out_rows rows per object
// (SaParams::out_rows; rows past n_cent repeat centroid n_cent - 1: the padding that lets the GA max run over power-of-two groups).
#include <type_traits>

#include "t2p_common.h"

namespace t2p {
namespace {

constexpr int kSub = 512;   // objects whose row counts / self-loop bases are cached in LDS at a time
constexpr int NT = 512;     // threads per workgroup: 8 waves = 2 per SIMD, so one wave's VALU/LDS phases overlap the other's MFMAs

template <int K, int N, int WN, int RT, bool X3>
struct SaCfg {
    static constexpr int WM = 8 / WN;
    static constexpr int NTW = N / (32 * WN);
    static constexpr int TR = WM * RT * 32;     // rows per batch
    static constexpr int KS = K / 2;            // fp32: k-steps per lane half
    static constexpr int S16 = K / 16;          // f16x3: MFMA steps
    static constexpr int WPLANES = X3 ? 2 : 1;  // stationary weight registers w[plane][n-tile][step]: f16x3 hi / lo half8, fp32 floats
    static constexpr int WSTEPS = X3 ? S16 : KS;
    // staging tile: fp32 one plane of floats, f16x3 a hi and a lo plane of halves; rows padded by 16 bytes.  Both are PLANE * 4 bytes.
    static constexpr int LD = X3 ? K + 8 : K + 4;   // elements per plane row
    static constexpr int PLANE = TR * LD;           // elements per plane
    static constexpr int ACC_INTS = 8192 + N;  // n_cent * N (128x64, 64x128, 32x256) + one dummy row for padding rows
    static constexpr int F4_PER_ROW = K / 4;
    static constexpr int ITERS = TR * F4_PER_ROW / NT;
    static_assert(TR * F4_PER_ROW % NT == 0, "staging must divide evenly over the workgroup");
    static_assert(ITERS == 2 || ITERS == 4, "metadata vector is 4 or 8 bytes");
    static constexpr size_t lds_bytes() {
        return (size_t)2 * PLANE * 4 + (size_t)2 * ACC_INTS * 4 + 2 * TR + kSub * 2 + kSub * 4;
    }
};

// Tile-count prefix sums over the objects and balanced contiguous ranges for n_wg workgroups.  One block of kBalT threads.
//   prefix[i] = sum over g < i of ceil(n_rows[g] / tile_rows), prefix[n] = total;
//   bounds[b] = first m in [0, n] with prefix[m] >= floor(b * total / n_wg) (b * total in 64 bits), bounds[n_wg] = n.
// The objects go through in chunks of kBalT * 8: a thread reads its 8 consecutive u16 counts as one 16-byte load (the next chunk's
// load is issued before this chunk's scan), the chunk is scanned with wave shuffles and one LDS level of 16 wave totals, and the
// thread writes its 8 prefixes as two 16-byte stores.  Every S-th prefix (S = 8 << sh, the smallest step whose table fits) is kept
// in LDS; a bound is a binary search over that table and one batch of at most S independent loads of the prefixes in between.
constexpr int kBalT = 1024;        // threads of the balancing block
constexpr int kBalCoarse = 8192;   // largest index of the LDS prefix table (n <= 65,536: every 8th prefix)

__device__ __forceinline__ void balance_body(const uint16_t* __restrict__ n_rows, int n, int tile_rows, int n_wg,
                                             int32_t* __restrict__ prefix, int32_t* __restrict__ bounds) {
    __shared__ int coarse[kBalCoarse + 1];
    __shared__ int wtot[2][kBalT / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int sh = 3;   // log2 of the table step
    while ((n >> sh) > kBalCoarse) sh++;
    const bool vec_in = (((uintptr_t)n_rows) & 15) == 0, vec_out = (((uintptr_t)prefix) & 15) == 0;
    const unsigned tr = (unsigned)tile_rows;

    typedef uint16_t u16x8 __attribute__((ext_vector_type(8)));
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    auto load8 = [&](int i0) -> u16x8 {   // counts i0 .. i0 + 7, zero past n
        u16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
        if (i0 + 8 <= n && vec_in) v = *(const u16x8*)(n_rows + i0);
        else {
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (i0 + e < n) v[e] = n_rows[i0 + e];
        }
        return v;
    };

    int carry = 0;   // tiles of the chunks before this one (the same in every thread)
    u16x8 cur = load8(tid * 8);
    for (int base = 0, it = 0; base < n; base += kBalT * 8, it++) {
        const int i0 = base + tid * 8;
        u16x8 nxt = {0, 0, 0, 0, 0, 0, 0, 0};
        if (base + kBalT * 8 < n) nxt = load8(i0 + kBalT * 8);
        int t[8], s = 0;
#pragma unroll
        for (int e = 0; e < 8; e++) {
            t[e] = (int)(((unsigned)cur[e] + tr - 1) / tr);
            s += t[e];
        }
        int inc = s;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (lane == 63) wtot[it & 1][wave] = inc;
        __syncthreads();   // (one barrier per chunk: the wave totals alternate between two buffers)
        int before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kBalT / 64; w++) {
            const int v = wtot[it & 1][w];
            before += w < wave ? v : 0;
            all += v;
        }
        int run = carry + before + inc - s;   // exclusive prefix of object i0
        carry += all;
        if (i0 < n && (i0 & ((1 << sh) - 1)) == 0) coarse[i0 >> sh] = run;
        int p[8];
#pragma unroll
        for (int e = 0; e < 8; e++) {
            p[e] = run;
            run += t[e];
        }
        if (i0 + 8 <= n && vec_out) {
            *(i32x4*)(prefix + i0) = i32x4{p[0], p[1], p[2], p[3]};
            *(i32x4*)(prefix + i0 + 4) = i32x4{p[4], p[5], p[6], p[7]};
        } else {
#pragma unroll
            for (int e = 0; e < 8; e++)
                if (i0 + e < n) prefix[i0 + e] = p[e];
        }
        cur = nxt;
    }
    const int total = carry;
    if (tid == 0) {
        prefix[n] = total;
        if ((n & ((1 << sh) - 1)) == 0) coarse[n >> sh] = total;
    }
    __syncthreads();   // the table, and this block's prefix stores for the loads below
    const int n_coarse = (n >> sh) + 1;   // table entries: prefix[j << sh], (j << sh) <= n
    for (int b = tid; b <= n_wg; b += kBalT) {
        // first object whose prefix >= b * total / n_wg
        const long long target = ((long long)b * total) / n_wg;
        int l = 0, r = n_coarse;   // first table entry >= target (n_coarse: none)
        while (l < r) {
            const int m = (l + r) >> 1;
            if (coarse[m] < target) l = m + 1; else r = m;
        }
        int ans = 0;
        if (l > 0) {
            // prefix[lo - 1] < target, and prefix[hi] >= target (the table entry, or prefix[n] = total): the answer is lo + the
            // number of prefixes below the target in [lo, hi) - they are non-decreasing
            const int lo = ((l - 1) << sh) + 1;
            const int hi = l < n_coarse ? (l << sh) : n;
            int cnt = 0;
            for (int x0 = lo; x0 < hi; x0 += 8) {
                int v[8];
#pragma unroll
                for (int e = 0; e < 8; e++) v[e] = prefix[(x0 + e) < hi ? (x0 + e) : hi];
#pragma unroll
                for (int e = 0; e < 8; e++) cnt += ((x0 + e) < hi && v[e] < target) ? 1 : 0;
            }
            ans = lo + cnt;
        }
        bounds[b] = b == n_wg ? n : ans;
    }
}

__global__ __launch_bounds__(kBalT) void k_balance(const uint16_t* __restrict__ n_rows, int n, int tile_rows, int n_wg,
                                                  int32_t* __restrict__ prefix, int32_t* __restrict__ bounds) {
    balance_body(n_rows, n, tile_rows, n_wg, prefix, bounds);
}

struct BalanceJobs {
    const uint16_t* n_rows[3];
    int32_t* prefix[3];
    int32_t* bounds[3];
    int tile_rows[3], n_wg[3];
    int n;
};
__global__ __launch_bounds__(kBalT) void k_balance_levels(BalanceJobs j) {  // one block per level
    const int l = blockIdx.x;
    balance_body(j.n_rows[l], j.n, j.tile_rows[l], j.n_wg[l], j.prefix[l], j.bounds[l]);
}

struct BatchIt {  // position in the flattened batch stream of a sub-range
    int gi;       // object index inside the cached sub-range
    int r0;       // first row of the batch inside the object
    int n;        // rows of the object
};

template <int K, int N, int WN, int RT, bool X3>
__global__ __launch_bounds__(NT, 2) void k_sa_stream(SaParams p) {
    using C = SaCfg<K, N, WN, RT, X3>;
    using TileT = std::conditional_t<X3, _Float16, float>;
    using WReg = std::conditional_t<X3, half8, float>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    TileT* tile = (TileT*)lds;                              // [2 buffers][fp32: PLANE floats | f16x3: hi plane, lo plane]
    int* acc_lds = (int*)(lds + 2 * C::PLANE);              // [2][ACC_INTS]
    uint8_t* dstl = (uint8_t*)(acc_lds + 2 * C::ACC_INTS);  // [2][TR] destination (centroid) of every staged row
    uint16_t* nr = (uint16_t*)(dstl + 2 * C::TR);           // [kSub] rows per object
    int* sbase = (int*)(nr + kSub);                         // [kSub] source row of centroid 0's self loop
    constexpr int TILE_ELEMS = C::WPLANES * C::PLANE;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % WN, wm = wave / WN, h = lane >> 5, l31 = lane & 31;
    const int nc = p.n_cent;
    const int maxr = nc * 33;
    const int rows_out = p.out_rows > 0 ? p.out_rows : nc;

    // stationary weights: the wave's NTW column tiles, all K
    WReg w[C::WPLANES][C::NTW][C::WSTEPS];
    if constexpr (X3) {
        const uint4* wp = (const uint4*)p.W_x3;
        constexpr int PLANE_U4 = (N / 32) * C::S16 * 64;
#pragma unroll
        for (int nt = 0; nt < C::NTW; nt++)
#pragma unroll
            for (int s = 0; s < C::S16; s++) {
                const int idx = (((wn * C::NTW + nt) * C::S16 + s) * 2 + h) * 32 + l31;
                w[0][nt][s] = __builtin_bit_cast(half8, wp[idx]);
                w[1][nt][s] = __builtin_bit_cast(half8, wp[PLANE_U4 + idx]);
            }
    } else {
#pragma unroll
        for (int nt = 0; nt < C::NTW; nt++)
#pragma unroll
            for (int s = 0; s < C::KS; s++)
                w[0][nt][s] = p.W[(int64_t)(h * C::KS + s) * N + wn * C::NTW * 32 + nt * 32 + l31];
    }
    float bias[C::NTW];
#pragma unroll
    for (int nt = 0; nt < C::NTW; nt++) bias[nt] = p.bias[wn * C::NTW * 32 + nt * 32 + l31];

    for (int i = tid; i < 2 * C::ACC_INTS; i += NT) acc_lds[i] = 0;
    [[maybe_unused]] float gmax = 0.f;   // f16x3: fp16-range guard, largest output this thread drained

    const int g_begin = p.bounds_ws[blockIdx.x], g_end = p.bounds_ws[blockIdx.x + 1];

    for (int ga = g_begin; ga < g_end; ga += kSub) {
        const int cnt = (g_end - ga) < kSub ? (g_end - ga) : kSub;
        __syncthreads();
        for (int i = tid; i < cnt; i += NT) {
            const int g = ga + i;
            nr[i] = p.n_rows[g];
            const int first = p.first[g];
            sbase[i] = first * p.n_dense + (g - first) * nc;
        }
        __syncthreads();

        auto advance = [&](BatchIt it) -> BatchIt {
            it.r0 += C::TR;
            if (it.r0 >= it.n) {
                it.gi++;
                it.r0 = 0;
                it.n = it.gi < cnt ? (int)nr[it.gi] : 0;
            }
            return it;
        };
        auto valid = [&](const BatchIt& it) { return it.gi < cnt; };

        // Each thread stages ITERS consecutive rows (lr = (tid / F4_PER_ROW) * ITERS + k) at a fixed column quad, so its
        // row metadata is ONE aligned vector load of ITERS u16.
        const int rgrp = (tid / C::F4_PER_ROW) * C::ITERS;   // first staged row of this thread inside the batch
        const int c4 = tid % C::F4_PER_ROW;
        typedef uint16_t metav __attribute__((ext_vector_type(C::ITERS)));
        metav meta_d, meta_m;                                 // metadata of the batch being gathered / the one after
        f32x4 sa[C::ITERS], sb[C::ITERS];

        // M: metadata of one batch -> registers (0xFFFF = padding row).  Split in two: the load is ISSUED at the top of a
        // batch, the clean-up of the rows past the object's end runs after the MFMA block -- touching the loaded value
        // any earlier puts an s_waitcnt vmcnt(0) in front of the MFMAs, which also waits for the gathers just issued
        // (measured: that exposed the whole gather latency, 28 % of the SA3 kernel).
        auto load_meta = [&](const BatchIt& it, metav& m) {
#pragma unroll
            for (int k = 0; k < C::ITERS; k++) m[k] = 0xFFFF;
            if (valid(it) && it.r0 + rgrp < it.n) {
                const uint32_t off = (uint32_t)(ga + it.gi) * (uint32_t)maxr + (uint32_t)(it.r0 + rgrp);
                if ((maxr & 3) == 0) {   // (n_cent % 4 == 0: the vector is aligned for every object)
                    m = *(const metav*)(p.rows + off);
                } else {
#pragma unroll
                    for (int k = 0; k < C::ITERS; k++) m[k] = p.rows[off + k];
                }
            }
        };
        auto fix_meta = [&](const BatchIt& it, metav& m) {
#pragma unroll
            for (int k = 0; k < C::ITERS; k++)
                if (it.r0 + rgrp + k >= it.n) m[k] = 0xFFFF;
        };
        // D: gathers of the batch's A_j and B_i rows -> registers (32-bit element offsets from uniform bases)
        auto load_data = [&](const BatchIt& it, const metav& m) {
            const uint32_t g = (uint32_t)(ga + it.gi);
            const uint32_t sb0 = valid(it) ? (uint32_t)sbase[it.gi] : 0u;
#pragma unroll
            for (int k = 0; k < C::ITERS; k++) {
                sa[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                sb[k] = f32x4{0.f, 0.f, 0.f, 0.f};
                if (m[k] != 0xFFFF) {
                    const uint32_t src = m[k] & 0xFF, d = m[k] >> 8, dl = d & 127;
                    const uint32_t srow = (d & 0x80) ? (sb0 + src) : (g * (uint32_t)p.n_dense + src);
                    sa[k] = *(const f32x4*)(p.A + (srow * (uint32_t)K + (uint32_t)c4 * 4u));
                    sb[k] = *(const f32x4*)(p.Bc + ((g * (uint32_t)nc + dl) * (uint32_t)K + (uint32_t)c4 * 4u));
                }
            }
        };
        // W: h = relu(A_j - B_i) -> LDS tile (f16x3: as fp16 hi / lo planes), plus the destination byte of every row
        auto write_tile = [&](int buf, const metav& m) {
            TileT* dst = tile + buf * TILE_ELEMS;
#pragma unroll
            for (int k = 0; k < C::ITERS; k++) {
                const int lr = rgrp + k;
                const f32x4 t = sa[k] - sb[k];
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaxf(t[e], 0.f);
                if constexpr (X3) {
                    const half4 hv = __builtin_convertvector(v, half4);
                    const half4 lv = __builtin_convertvector(v - __builtin_convertvector(hv, f32x4), half4);
                    *(half4*)(dst + lr * C::LD + c4 * 4) = hv;
                    *(half4*)(dst + C::PLANE + lr * C::LD + c4 * 4) = lv;
                } else {
                    *(f32x4*)(dst + lr * C::LD + c4 * 4) = v;
                }
                // destination of the row; padding rows go to the accumulator's dummy row n_cent
                if (c4 == 0) dstl[buf * C::TR + lr] = m[k] == 0xFFFF ? (uint8_t)nc : (uint8_t)((m[k] >> 8) & 127);
            }
        };
        // flush one finished object's accumulator (feature columns; the [xyz 0] quad of the rows is written
        // by the centroid-table kernel), re-zero
        // (out_rows > n_cent: the rows behind repeat centroid n_cent - 1, the padding of the GA max groups)
        auto flush = [&](int64_t g, int abuf) {
            int* a = acc_lds + abuf * C::ACC_INTS;
            float* o = p.out + g * rows_out * (int64_t)p.ldo;
            for (int i = tid; i < nc * N; i += NT) {
                const int c = i / N, col = i % N;
                const float v = __int_as_float(a[i]) * p.out_scale;
                if constexpr (X3) gmax = fmaxf(gmax, v);
                o[c * (int64_t)p.ldo + col] = v;
                if (c == nc - 1)
                    for (int r = nc; r < rows_out; r++) o[r * (int64_t)p.ldo + col] = v;
                a[i] = 0;
            }
        };

        BatchIt it_c{0, 0, cnt > 0 ? (int)nr[0] : 0};
        BatchIt it_d = advance(it_c);
        BatchIt it_m = advance(it_d);
        // prologue: M(0), M(1), D(0), W(0)
        load_meta(it_c, meta_d);
        load_meta(it_d, meta_m);
        fix_meta(it_c, meta_d);
        fix_meta(it_d, meta_m);
        load_data(it_c, meta_d);
        write_tile(0, meta_d);
        meta_d = meta_m;
        __syncthreads();

        int64_t flush_g = -1;
        int flush_buf = 0;
        for (int t = 0; valid(it_c); t++) {
            // the object finished in the previous batch drains to HBM underneath this batch's MFMAs
            if (flush_g >= 0) {
                flush(flush_g, flush_buf);
                flush_g = -1;
            }
            if (valid(it_d)) load_data(it_d, meta_d);      // D(t+1): gathers go out first ...
            load_meta(it_m, meta_m);                       // M(t+2): ... the younger metadata loads stay in flight

            // C(t): MFMA block on tile t & 1
            f32x16 acc[RT][C::NTW];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int nt = 0; nt < C::NTW; nt++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[rt][nt][e] = bias[nt];  // bias rides in the accumulator
            const int buf = t & 1;
            const TileT* hrow = tile + buf * TILE_ELEMS + ((wm * RT) * 32 + l31) * C::LD + h * (K / 2);
            if constexpr (X3) {
#pragma unroll
                for (int s = 0; s < C::S16; s++) {
                    half8 a_hi[RT], a_lo[RT];
#pragma unroll
                    for (int rt = 0; rt < RT; rt++) {
                        a_hi[rt] = *(const half8*)(hrow + rt * 32 * C::LD + 8 * s);
                        a_lo[rt] = *(const half8*)(hrow + C::PLANE + rt * 32 * C::LD + 8 * s);
                    }
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
#pragma unroll
                        for (int nt = 0; nt < C::NTW; nt++) {
                            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[rt], w[0][nt][s], acc[rt][nt], 0, 0, 0);
                            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[rt], w[1][nt][s], acc[rt][nt], 0, 0, 0);
                            acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[rt], w[0][nt][s], acc[rt][nt], 0, 0, 0);
                        }
                }
            } else {
                constexpr int QC = 4;                 // k-quads (16 k-steps) fetched per LDS round
                constexpr int NCH = C::KS / 4 / QC;   // chunks
                static_assert((C::KS / 4) % QC == 0, "K/8 must be a multiple of the LDS prefetch chunk");
                f32x4 a_cur[RT][QC], a_nxt[RT][QC];
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int qi = 0; qi < QC; qi++) a_cur[rt][qi] = *(const f32x4*)(hrow + rt * 32 * C::LD + qi * 4);
#pragma unroll
                for (int ch = 0; ch < NCH; ch++) {
                    if (ch + 1 < NCH) {
#pragma unroll
                        for (int rt = 0; rt < RT; rt++)
#pragma unroll
                            for (int qi = 0; qi < QC; qi++)
                                a_nxt[rt][qi] = *(const f32x4*)(hrow + rt * 32 * C::LD + ((ch + 1) * QC + qi) * 4);
                    }
#pragma unroll
                    for (int qi = 0; qi < QC; qi++)
#pragma unroll
                        for (int j = 0; j < 4; j++)
#pragma unroll
                            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                                for (int nt = 0; nt < C::NTW; nt++)
                                    acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(
                                        a_cur[rt][qi][j], w[0][nt][(ch * QC + qi) * 4 + j], acc[rt][nt], 0, 0, 0);
#pragma unroll
                    for (int rt = 0; rt < RT; rt++)
#pragma unroll
                        for (int qi = 0; qi < QC; qi++) a_cur[rt][qi] = a_nxt[rt][qi];
                }
            }

            // max-aggregation: every accumulator row goes straight to its destination's LDS slot with an integer atomic
            // max (non-returning; the signed-int max against +0 is also the ReLU - the f16x3 scale is a positive power of two).
            // No run detection, no branches: padding rows carry destination n_cent = the accumulator's dummy row.
            const int abuf = it_c.gi & 1;
            int* accb = acc_lds + abuf * C::ACC_INTS;
            const uint8_t* dl = dstl + buf * C::TR;
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const int trow0 = (wm * RT + rt) * 32;
                if (it_c.r0 + trow0 >= it_c.n) continue;
                int doff[16];  // destination row offsets (ints) of this lane's 16 rows: 4 quads of 4 consecutive rows
#pragma unroll
                for (int q = 0; q < 4; q++) {
                    const uint32_t four = *(const uint32_t*)(dl + trow0 + 8 * q + 4 * h);
#pragma unroll
                    for (int e = 0; e < 4; e++) doff[4 * q + e] = (int)((four >> (8 * e)) & 0xFF) * N;
                }
#pragma unroll
                for (int nt = 0; nt < C::NTW; nt++) {
                    int* col = accb + wn * C::NTW * 32 + nt * 32 + l31;
#pragma unroll
                    for (int e = 0; e < 16; e++) atomicMax(col + doff[e], __float_as_int(acc[rt][nt][e]));
                }
            }
            if (it_c.r0 + C::TR >= it_c.n) {  // last batch of this object
                flush_g = ga + it_c.gi;
                flush_buf = abuf;
            }
            if (valid(it_d)) write_tile((t + 1) & 1, meta_d);  // W(t+1)
            fix_meta(it_m, meta_m);
            meta_d = meta_m;
            it_c = it_d;
            it_d = it_m;
            it_m = advance(it_m);
            __syncthreads();
        }
        if (flush_g >= 0) flush(flush_g, flush_buf);
    }
    // f16x3: the level's exact output maximum (high and low side of the guard), once per wave
    if constexpr (X3) guard_publish_exact(p.amax_out, gmax);
}

}  // namespace

int launch_sa_balance_arrays(const uint16_t* n_rows, int n, int tile_rows, int n_wg, int32_t* prefix, int32_t* bounds, hipStream_t st) {
    ProfScope ps_("sa_balance", st);
    hipLaunchKernelGGL(k_balance, dim3(1), dim3(kBalT), 0, st, n_rows, n, tile_rows, n_wg, prefix, bounds);
    T2P_CHECK_LAUNCH("sa_balance");
    return 0;
}

int launch_sa_balance(const SaParams& p, int tile_rows, int n_wg, hipStream_t st) {
    return launch_sa_balance_arrays(p.n_rows, (int)p.n_obj, tile_rows, n_wg, p.prefix_ws, p.bounds_ws, st);
}

namespace {

// The stream kernel's instantiations (K = H, N = C, WN, RT), both arithmetic paths: launch and launch shape go through this one list
#define SA_STREAM_CASES(X) X(32, 64, 2, 2) X(128, 128, 4, 1) X(256, 256, 8, 1)

// tile rows / workgroup count (bounds_ws holds 1,025 entries) of the stream kernel for (H, Cout)
int sa_stream_shape(int H, int Cout, bool x3, int64_t n_obj, int* tile_rows, int* n_wg) {
    int n = num_cus();
    if (n > 1024) n = 1024;
    if (n > n_obj) n = (int)n_obj;
    *n_wg = n;
#define SA_CASE(K_, N_, WN_, RT_)                           \
    if (H == K_ && Cout == N_) {                            \
        *tile_rows = SaCfg<K_, N_, WN_, RT_, false>::TR;    \
        return 0;                                           \
    }
    SA_STREAM_CASES(SA_CASE)
#undef SA_CASE
    if (x3) set_error("sa_x3: no instantiation for H=%d C=%d (built: 32/64, 128/128, 256/256)", H, Cout);
    else set_error("ws_sa: no instantiation for H=%d C=%d", H, Cout);
    return T2P_E_UNSUPPORTED;
}

template <int K, int N, int WN, int RT, bool X3>
int launch_sa_cfg(const SaParams& p, hipStream_t st, const char* name) {
    using C = SaCfg<K, N, WN, RT, X3>;
    static_assert(C::TR == SaCfg<K, N, WN, RT, !X3>::TR, "one launch shape for both paths");
    constexpr const char* who = X3 ? "sa_x3" : "ws_sa";
    auto kern = k_sa_stream<K, N, WN, RT, X3>;
    T2P_TRY(reserve_lds((const void*)kern, C::lds_bytes(), who));
    if (p.n_obj <= 0) return 0;
    // the kernel forms srow * K in 32 bits
    T2P_CHECK_ARG(p.n_obj < (1 << 30) && p.n_obj * p.n_dense * (int64_t)K < 0xffffffffLL,
                  X3 ? "sa_x3: chunk too large for 32-bit table offsets" : "ws_sa: chunk too large for 32-bit rows");
    int tr = 0, n_wg = 0;
    T2P_TRY(sa_stream_shape(K, N, X3, p.n_obj, &tr, &n_wg));
    if (!p.balanced) T2P_TRY(launch_sa_balance(p, tr, n_wg, st));
    ProfScope ps_(name, st);
    T2P_REPEAT(ps_) hipLaunchKernelGGL(kern, dim3(n_wg), dim3(NT), C::lds_bytes(), st, p);
    T2P_CHECK_LAUNCH(who);
    return 0;
}

int launch_sa_stream(int H, int Cout, const SaParams& p, hipStream_t st) {
    const bool x3 = p.W_x3 != nullptr;
    if (x3) {
        T2P_CHECK_ARG(p.Bc != nullptr && p.wp == nullptr, "sa_x3: reads the centroid table B from HBM (Bc set, wp unset)");
        T2P_CHECK_ARG(p.n_cent >= 1 && p.n_cent <= 128 && p.n_dense >= p.n_cent && p.n_dense <= 256 && (int64_t)p.n_cent * Cout <= 8192,
                      "sa_x3: n_dense=%d n_cent=%d C=%d outside the accumulator (n_cent * C <= 8192)", p.n_dense, p.n_cent, Cout);
        T2P_CHECK_ARG(p.out_rows == 0 || p.out_rows >= p.n_cent, "sa_x3: out_rows=%d < n_cent=%d", p.out_rows, p.n_cent);
        T2P_CHECK_ARG((((uintptr_t)p.A | (uintptr_t)p.Bc | (uintptr_t)p.W_x3 | (uintptr_t)p.rows) & 15) == 0,
                      "sa_x3: tables and weights must be 16-byte aligned");
    }
#define SA_CASE(K_, N_, WN_, RT_)                                                                                  \
    if (H == K_ && Cout == N_)                                                                                     \
        return x3 ? launch_sa_cfg<K_, N_, WN_, RT_, true>(p, st, "sa_x3_k" #K_ "_n" #N_)                           \
                  : launch_sa_cfg<K_, N_, WN_, RT_, false>(p, st, "ws_edge_sa_k" #K_ "_n" #N_);
    SA_STREAM_CASES(SA_CASE)
#undef SA_CASE
    int tr, n_wg;
    return sa_stream_shape(H, Cout, x3, 1, &tr, &n_wg);   // no such instantiation: its error
}

// f16x3: the specialised kernels take exactly the level shape of 256 points per object they are built for (with the LDS centroid
// table); every other shape runs on the stream kernel, which gathers the centroid table from HBM
enum SaKernel { SA_FP32, SA_POINTS, SA_ROWS, SA_3, SA_X3, SA_NONE };
SaKernel sa_pick(int H, int Cout, const SaParams& p) {
    if (p.W_x3 == nullptr) return SA_FP32;
    if (p.n_dense == 128 && p.n_cent == 64 && sa_rows_selected(H, Cout, p)) return SA_ROWS;
    if (p.n_dense == 256 && p.n_cent == 128 && sa_points_selected(H, Cout, p)) return SA_POINTS;
    if (p.n_dense == 64 && p.n_cent == 32 && sa3_selected(H, Cout, p)) return SA_3;
    if (p.wp == nullptr) return SA_X3;
    set_error("ws_sa: no f16x3 kernel with an LDS centroid table for H=%d C=%d n_dense=%d n_cent=%d (built: the level shapes of "
              "256 points; other shapes gather the table from HBM: wp unset)", H, Cout, p.n_dense, p.n_cent);
    return SA_NONE;
}

// tile rows / workgroup count of the kernel launch_ws_sa will pick for (H, Cout)
int sa_launch_shape(int H, int Cout, const SaParams& p, int64_t n_obj, int* tile_rows, int* n_wg) {
    switch (sa_pick(H, Cout, p)) {
        case SA_ROWS: return sa_rows_launch_shape(n_obj, tile_rows, n_wg);
        case SA_POINTS: return sa_points_launch_shape(n_obj, tile_rows, n_wg);
        case SA_3: return sa3_launch_shape(n_obj, tile_rows, n_wg);
        case SA_X3: return sa_stream_shape(H, Cout, true, n_obj, tile_rows, n_wg);
        case SA_FP32: return sa_stream_shape(H, Cout, false, n_obj, tile_rows, n_wg);
        case SA_NONE: break;
    }
    return T2P_E_UNSUPPORTED;
}

}  // namespace

int launch_sa_balance_levels(const SaParams p[3], const int H[3], const int C[3], hipStream_t st) {
    if (p[0].n_obj <= 0) return 0;
    BalanceJobs j;
    j.n = (int)p[0].n_obj;
    for (int l = 0; l < 3; l++) {
        j.n_rows[l] = p[l].n_rows;
        j.prefix[l] = p[l].prefix_ws;
        j.bounds[l] = p[l].bounds_ws;
        T2P_TRY(sa_launch_shape(H[l], C[l], p[l], p[l].n_obj, &j.tile_rows[l], &j.n_wg[l]));
    }
    ProfScope ps_("sa_balance", st);
    hipLaunchKernelGGL(k_balance_levels, dim3(3), dim3(kBalT), 0, st, j);
    T2P_CHECK_LAUNCH("sa_balance");
    return 0;
}

int launch_ws_sa(int H, int Cout, const SaParams& p, hipStream_t st) {
    T2P_CHECK_ARG((((uintptr_t)p.A | (uintptr_t)p.Bc) & 15) == 0, "ws_sa: tables must be 16-byte aligned");
    if (p.W_x3 != nullptr) T2P_CHECK_ARG(((uintptr_t)p.W_x3 & 15) == 0, "ws_sa: packed f16x3 weights must be 16-byte aligned");
    switch (sa_pick(H, Cout, p)) {   // f16x3: one kernel per level
        case SA_ROWS: return launch_sa_rows(H, Cout, p, st);
        case SA_POINTS: return launch_sa_points(H, Cout, p, st);
        case SA_3: return launch_sa3(p, st);
        case SA_X3:
        case SA_FP32: return launch_sa_stream(H, Cout, p, st);
        case SA_NONE: break;
    }
    return T2P_E_UNSUPPORTED;
}

}  // namespace t2p
