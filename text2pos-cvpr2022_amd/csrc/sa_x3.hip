// Set-abstraction edge kernel, f16x3 path, for ANY object size: per-edge ReLU(A_j - B_i) -> layer-2 GEMM -> max per centroid at
// runtime n_dense / n_cent (n_cent * C <= 8192), for the three levels (H, C) = (32, 64), (128, 128), (256, 256).
// (reference: gnn.PointConv(local_nn)(x, (pos, pos[idx]), edge_index), models/pointcloud/pointnet2.py:31-35).
//
// The specialised f16x3 kernels (sa_points.hip, sa_rows.hip, sa3.hip) are built for the level shapes of 256 points per object and
// build their centroid tables in LDS.  Every other shape (pointnet_numpoints != 256) runs here, with the data flow of the exact-fp32
// kernel of ws_sa.hip: balanced contiguous object ranges (k_balance_levels), one flattened stream of row batches that crosses object
// boundaries, A_j / B_i rows gathered from the HBM tables (k_sample_group writes B_l when the LDS centroid table is off), a
// double-buffered LDS max-accumulator per object.  Only the arithmetic differs:
//   * staging splits h = relu(A_j - B_i) into fp16 hi = fp16(h) and lo = fp16(h - hi) (both to nearest) and writes two fp16 planes;
//   * each wave keeps a 32-column slice of the scaled layer-2 image sa_w2_x3 in registers (packing.py::pack_f16x3_scaled, register
//     order: lane half u of MFMA step s holds k = u K/2 + 8 s .. + 7) and runs hi.hi, hi.lo, lo.hi per step on
//     v_mfma_f32_32x32x16_f16 into ONE fp32 accumulator that starts at the scaled bias;
//   * the drain multiplies by 1 / scale and publishes the level's exact output maximum (guard slot G_F1 + l), as the specialised
//     kernels do.
// The drain writes out_rows rows per object (SaParams::out_rows; rows past n_cent repeat centroid n_cent - 1: the padding that lets
// the GA max run over power-of-two groups).
#include "t2p_common.h"

namespace t2p {
int launch_sa_balance(const SaParams& p, int tile_rows, int n_wg, hipStream_t st);  // ws_sa.hip

namespace {

typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int kSub = 512;   // objects whose row counts / self-loop bases are cached in LDS at a time
constexpr int NT = 512;     // 8 waves: one workgroup per CU (LDS), two waves per SIMD

template <int K, int N, int WN, int RT>
struct X3Cfg {
    static constexpr int WM = 8 / WN;
    static constexpr int NTW = N / (32 * WN);
    static constexpr int S16 = K / 16;          // MFMA steps
    static constexpr int TR = WM * RT * 32;     // rows per batch
    static constexpr int LDHH = K + 8;          // halves per plane row (16-byte pad)
    static constexpr int PLANE = TR * LDHH;     // halves per plane
    static constexpr int TILE_HALVES = 2 * PLANE;
    static constexpr int ACC_INTS = 8192 + N;   // n_cent * N + one dummy row for padding rows
    static constexpr int F4_PER_ROW = K / 4;
    static constexpr int ITERS = TR * F4_PER_ROW / NT;
    static_assert(TR * F4_PER_ROW % NT == 0, "staging must divide evenly over the workgroup");
    static_assert(ITERS == 2 || ITERS == 4, "metadata vector is 4 or 8 bytes");
    static constexpr size_t lds_bytes() {
        return (size_t)2 * TILE_HALVES * 2 + (size_t)2 * ACC_INTS * 4 + 2 * TR + kSub * 2 + kSub * 4;
    }
};

struct BatchIt {  // position in the flattened batch stream of a sub-range
    int gi;       // object index inside the cached sub-range
    int r0;       // first row of the batch inside the object
    int n;        // rows of the object
};

template <int K, int N, int WN, int RT>
__global__ __launch_bounds__(NT, 2) void k_sa_x3(SaParams p) {
    using C = X3Cfg<K, N, WN, RT>;
    extern __shared__ __attribute__((aligned(16))) float lds[];
    _Float16* tile = (_Float16*)lds;                        // [2 buffers][hi plane | lo plane]
    int* acc_lds = (int*)(tile + 2 * C::TILE_HALVES);       // [2][ACC_INTS]
    uint8_t* dstl = (uint8_t*)(acc_lds + 2 * C::ACC_INTS);  // [2][TR] destination (centroid) of every staged row
    uint16_t* nr = (uint16_t*)(dstl + 2 * C::TR);           // [kSub] rows per object
    int* sbase = (int*)(nr + kSub);                         // [kSub] source row of centroid 0's self loop

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wn = wave % WN, wm = wave / WN, h = lane >> 5, l31 = lane & 31;
    const int nc = p.n_cent;
    const int maxr = nc * 33;
    const int rows_out = p.out_rows > 0 ? p.out_rows : nc;

    // stationary weights: the wave's NTW column tiles, all K, hi / lo planes of the register-order image
    half8 w_hi[C::NTW][C::S16], w_lo[C::NTW][C::S16];
    {
        const uint4* wp = (const uint4*)p.W_x3;
        constexpr int PLANE_U4 = (N / 32) * C::S16 * 64;
#pragma unroll
        for (int nt = 0; nt < C::NTW; nt++)
#pragma unroll
            for (int s = 0; s < C::S16; s++) {
                const int idx = (((wn * C::NTW + nt) * C::S16 + s) * 2 + h) * 32 + l31;
                w_hi[nt][s] = __builtin_bit_cast(half8, wp[idx]);
                w_lo[nt][s] = __builtin_bit_cast(half8, wp[PLANE_U4 + idx]);
            }
    }
    float bias[C::NTW];
#pragma unroll
    for (int nt = 0; nt < C::NTW; nt++) bias[nt] = p.bias[wn * C::NTW * 32 + nt * 32 + l31];

    for (int i = tid; i < 2 * C::ACC_INTS; i += NT) acc_lds[i] = 0;
    float gmax = 0.f;   // fp16-range guard: largest output this thread drained

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

        // each thread stages ITERS consecutive rows at a fixed column quad: its row metadata is one aligned vector load
        const int rgrp = (tid / C::F4_PER_ROW) * C::ITERS;
        const int c4 = tid % C::F4_PER_ROW;
        typedef uint16_t metav __attribute__((ext_vector_type(C::ITERS)));
        metav meta_d, meta_m;
        f32x4 sa[C::ITERS], sb[C::ITERS];

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
        // h = relu(A_j - B_i) -> fp16 hi / lo planes, plus the destination byte of every row
        auto write_tile = [&](int buf, const metav& m) {
            _Float16* hi_pl = tile + buf * C::TILE_HALVES;
            _Float16* lo_pl = hi_pl + C::PLANE;
#pragma unroll
            for (int k = 0; k < C::ITERS; k++) {
                const int lr = rgrp + k;
                const f32x4 t = sa[k] - sb[k];
                f32x4 v;
#pragma unroll
                for (int e = 0; e < 4; e++) v[e] = fmaxf(t[e], 0.f);
                const half4 hv = __builtin_convertvector(v, half4);
                const half4 lv = __builtin_convertvector(v - __builtin_convertvector(hv, f32x4), half4);
                *(half4*)(hi_pl + lr * C::LDHH + c4 * 4) = hv;
                *(half4*)(lo_pl + lr * C::LDHH + c4 * 4) = lv;
                // padding rows go to the accumulator's dummy row n_cent
                if (c4 == 0) dstl[buf * C::TR + lr] = m[k] == 0xFFFF ? (uint8_t)nc : (uint8_t)((m[k] >> 8) & 127);
            }
        };
        // drain one finished object's accumulator (feature columns; the [xyz 0] tail is k_sample_group's), re-zero
        auto flush = [&](int64_t g, int abuf) {
            int* a = acc_lds + abuf * C::ACC_INTS;
            float* o = p.out + g * rows_out * (int64_t)p.ldo;
            for (int i = tid; i < nc * N; i += NT) {
                const int c = i / N, col = i % N;
                const float v = __int_as_float(a[i]) * p.out_scale;
                gmax = fmaxf(gmax, v);
                o[c * (int64_t)p.ldo + col] = v;
                if (c == nc - 1)
                    for (int r = nc; r < rows_out; r++) o[r * (int64_t)p.ldo + col] = v;
                a[i] = 0;
            }
        };

        BatchIt it_c{0, 0, cnt > 0 ? (int)nr[0] : 0};
        BatchIt it_d = advance(it_c);
        BatchIt it_m = advance(it_d);
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
            if (flush_g >= 0) {
                flush(flush_g, flush_buf);
                flush_g = -1;
            }
            if (valid(it_d)) load_data(it_d, meta_d);      // gathers of batch t + 1 first ...
            load_meta(it_m, meta_m);                       // ... metadata of batch t + 2 behind them

            // MFMA block on tile t & 1: the bias rides in the accumulator
            f32x16 acc[RT][C::NTW];
#pragma unroll
            for (int rt = 0; rt < RT; rt++)
#pragma unroll
                for (int nt = 0; nt < C::NTW; nt++)
#pragma unroll
                    for (int e = 0; e < 16; e++) acc[rt][nt][e] = bias[nt];
            const int buf = t & 1;
            const _Float16* hrow = tile + buf * C::TILE_HALVES + ((wm * RT) * 32 + l31) * C::LDHH + h * (K / 2);
#pragma unroll
            for (int s = 0; s < C::S16; s++) {
                half8 a_hi[RT], a_lo[RT];
#pragma unroll
                for (int rt = 0; rt < RT; rt++) {
                    a_hi[rt] = *(const half8*)(hrow + rt * 32 * C::LDHH + 8 * s);
                    a_lo[rt] = *(const half8*)(hrow + C::PLANE + rt * 32 * C::LDHH + 8 * s);
                }
#pragma unroll
                for (int rt = 0; rt < RT; rt++)
#pragma unroll
                    for (int nt = 0; nt < C::NTW; nt++) {
                        acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[rt], w_hi[nt][s], acc[rt][nt], 0, 0, 0);
                        acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_hi[rt], w_lo[nt][s], acc[rt][nt], 0, 0, 0);
                        acc[rt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a_lo[rt], w_hi[nt][s], acc[rt][nt], 0, 0, 0);
                    }
            }

            // max-aggregation: integer atomic max on the LDS accumulator (the scale is a positive power of two, so the signed-int
            // max against +0 is also the ReLU); padding rows carry destination n_cent = the dummy row
            const int abuf = it_c.gi & 1;
            int* accb = acc_lds + abuf * C::ACC_INTS;
            const uint8_t* dl = dstl + buf * C::TR;
#pragma unroll
            for (int rt = 0; rt < RT; rt++) {
                const int trow0 = (wm * RT + rt) * 32;
                if (it_c.r0 + trow0 >= it_c.n) continue;
                int doff[16];  // destination offsets of this lane's 16 rows: rows 8 q + 4 h + e of the 32-row tile
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
            if (valid(it_d)) write_tile((t + 1) & 1, meta_d);
            fix_meta(it_m, meta_m);
            meta_d = meta_m;
            it_c = it_d;
            it_d = it_m;
            it_m = advance(it_m);
            __syncthreads();
        }
        if (flush_g >= 0) flush(flush_g, flush_buf);
    }
    // the level's exact output maximum (high and low side of the guard), once per wave
    guard_publish_exact(p.amax_out, gmax);
}

template <int K, int N, int WN, int RT>
int launch_x3_cfg(const SaParams& p, hipStream_t st, const char* name) {
    using C = X3Cfg<K, N, WN, RT>;
    auto kern = k_sa_x3<K, N, WN, RT>;
    T2P_TRY(reserve_lds((const void*)kern, C::lds_bytes(), "sa_x3"));
    if (p.n_obj <= 0) return 0;
    int tr = 0, n_wg = 0;
    T2P_TRY(sa_x3_launch_shape(K, N, p.n_obj, &tr, &n_wg));
    if (!p.balanced) T2P_TRY(launch_sa_balance(p, tr, n_wg, st));
    ProfScope ps_(name, st);
    T2P_REPEAT(ps_) hipLaunchKernelGGL(kern, dim3(n_wg), dim3(NT), C::lds_bytes(), st, p);
    T2P_CHECK_LAUNCH("sa_x3");
    return 0;
}

}  // namespace

int sa_x3_launch_shape(int H, int Cout, int64_t n_obj, int* tile_rows, int* n_wg) {
    int n = num_cus();
    if (n > 1024) n = 1024;
    if (n > n_obj) n = (int)n_obj;
    *n_wg = n;
    if (H == 32 && Cout == 64) { *tile_rows = X3Cfg<32, 64, 2, 2>::TR; return 0; }
    if (H == 128 && Cout == 128) { *tile_rows = X3Cfg<128, 128, 4, 1>::TR; return 0; }
    if (H == 256 && Cout == 256) { *tile_rows = X3Cfg<256, 256, 8, 1>::TR; return 0; }
    set_error("sa_x3: no instantiation for H=%d C=%d (built: 32/64, 128/128, 256/256)", H, Cout);
    return T2P_E_UNSUPPORTED;
}

int launch_sa_x3(int H, int Cout, const SaParams& p, hipStream_t st) {
    T2P_CHECK_ARG(p.Bc != nullptr && p.wp == nullptr, "sa_x3: reads the centroid table B from HBM (Bc set, wp unset)");
    T2P_CHECK_ARG(p.n_cent >= 1 && p.n_cent <= 128 && p.n_dense >= p.n_cent && p.n_dense <= 256 && (int64_t)p.n_cent * Cout <= 8192,
                  "sa_x3: n_dense=%d n_cent=%d C=%d outside the accumulator (n_cent * C <= 8192)", p.n_dense, p.n_cent, Cout);
    T2P_CHECK_ARG(p.out_rows == 0 || p.out_rows >= p.n_cent, "sa_x3: out_rows=%d < n_cent=%d", p.out_rows, p.n_cent);
    T2P_CHECK_ARG(p.n_obj < (1 << 30) && p.n_obj * p.n_dense * (int64_t)H < 0xffffffffLL,
                  "sa_x3: chunk too large for 32-bit table offsets");
    T2P_CHECK_ARG((((uintptr_t)p.A | (uintptr_t)p.Bc | (uintptr_t)p.W_x3 | (uintptr_t)p.rows) & 15) == 0,
                  "sa_x3: tables and weights must be 16-byte aligned");
    if (H == 32 && Cout == 64) return launch_x3_cfg<32, 64, 2, 2>(p, st, "sa_x3_k32_n64");
    if (H == 128 && Cout == 128) return launch_x3_cfg<128, 128, 4, 1>(p, st, "sa_x3_k128_n128");
    if (H == 256 && Cout == 256) return launch_x3_cfg<256, 256, 8, 1>(p, st, "sa_x3_k256_n256");
    set_error("sa_x3: no instantiation for H=%d C=%d (built: 32/64, 128/128, 256/256)", H, Cout);
    return T2P_E_UNSUPPORTED;
}

}  // namespace t2p
