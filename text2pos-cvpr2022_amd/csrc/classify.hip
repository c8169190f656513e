// PointNet++ pre-training (stage one of the reference, training/pointcloud/pointnet2.py): the two classifier heads of
// PointNet2.forward and the softmax cross-entropy of its training loop.  Plain HIP C++, 64-lane waves.
#include "t2p_common.h"

namespace t2p {
namespace {

// ---- classifier heads ------------------------------------------------------------------------------------------
// models/pointcloud/pointnet2.py:91-92: class_pred = class_classifier(features2), color_pred = color_classifier(features2).
// One launch for both: f2 [n][256] times W [256][C] (k-major, C = C1 + C2 <= 128: the two heads side by side) plus bias.
// A skinny product (30 columns for the reference's 22 classes + 8 colours), so no MFMA tile: the weight block is staged in
// LDS once per workgroup, the rows of a pass beside it, and every lane owns ONE logit - bias first, then the 256 products
// added by fmaf in ascending k (a fixed order: the same bits whatever the batch around a row is).
constexpr int kHeadK = 256;
constexpr int kHeadThreads = 256;

__global__ __launch_bounds__(kHeadThreads) void k_classifier_heads(const float* __restrict__ f2, const float* __restrict__ w,
                                                                   const float* __restrict__ bias, int64_t n, int C1, int C2,
                                                                   float* __restrict__ class_pred, float* __restrict__ color_pred) {
    extern __shared__ __align__(16) float lds[];
    const int C = C1 + C2;
    const int rows = kHeadThreads / C < 32 ? kHeadThreads / C : 32;   // rows of a pass (C <= 128: at least 2)
    float* w_s = lds;                           // [256][C]
    float* x_s = lds + kHeadK * C;              // [rows][256]
    for (int i = threadIdx.x; i < kHeadK * C; i += kHeadThreads) w_s[i] = w[i];
    const int r = threadIdx.x / C, c = threadIdx.x - r * C;
    const float b = r < rows ? bias[c] : 0.f;   // (lanes past the last whole row of a pass idle)
    for (int64_t row0 = (int64_t)blockIdx.x * rows; row0 < n; row0 += (int64_t)gridDim.x * rows) {
        __syncthreads();                        // the weights (first pass) / the previous pass's readers
        // the pass's rows are contiguous in f2: 16-byte loads, 64 lanes = 1 KB per wave instruction
        const int64_t left = n - row0;
        const int live = left < rows ? (int)left : rows;
        const f32x4* src = (const f32x4*)(f2 + row0 * kHeadK);
        for (int i = threadIdx.x; i < live * (kHeadK / 4); i += kHeadThreads) ((f32x4*)x_s)[i] = src[i];
        __syncthreads();
        if (r < live) {
            float acc = b;
            const float* x = x_s + r * kHeadK;  // (one address per row group: LDS broadcast)
#pragma unroll 8
            for (int k = 0; k < kHeadK; k++) acc = fmaf(x[k], w_s[k * C + c], acc);
            if (c < C1)
                class_pred[(row0 + r) * C1 + c] = acc;
            else
                color_pred[(row0 + r) * C2 + (c - C1)] = acc;
        }
    }
}

// ---- softmax cross-entropy ---------------------------------------------------------------------------------------
// nn.CrossEntropyLoss()(class_pred, batch.y) (training/pointcloud/pointnet2.py:37, :134, mean reduction) and the accuracy
// line :42 in one launch: per row  row_loss = logsumexp(x) - x[label],  d_logits = (softmax(x) - onehot(label)) * inv_n,
// correct = (argmax(x) == label), ties to the lower index as torch.argmax.  G lanes per row (a power of two, 8 .. 64: 64 / G rows
// per wave for small C), lane g holds columns g, g + G, ...; the row maximum (subtracted before exp), the arg-max and the sum
// are reduced across the G lanes by __shfl_xor butterflies - every lane of a group ends with the same bits, no atomics.
// A label outside [0, C) gives NaN in row_loss and in the row's d_logits (and correct = 0); nothing is read through it.
template <int G>
__global__ __launch_bounds__(256) void k_softmax_xent(const float* __restrict__ logits, int ld, const int32_t* __restrict__ labels,
                                                      int64_t n, int C, float inv_n, float* __restrict__ row_loss,
                                                      float* __restrict__ d_logits, int ldd, int32_t* __restrict__ correct) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t row = t / G;
    const int g = (int)(t % G);
    const bool live = row < n;                  // (a dead group still takes part in the shuffles of its wave)
    const float* x = logits + (live ? row : 0) * (int64_t)ld;
    float m = -__builtin_inff();
    int arg = 0x7fffffff;
    if (live)
        for (int c = g; c < C; c += G) {
            const float v = x[c];
            if (v > m || arg == 0x7fffffff) {   // strict: the first of equal values stays
                m = v;
                arg = c;
            }
        }
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) {
        const float mo = __shfl_xor(m, o, 64);
        const int ao = __shfl_xor(arg, o, 64);
        if (mo > m || (mo == m && ao < arg)) {
            m = mo;
            arg = ao;
        }
    }
    float s = 0.f;
    if (live)
        for (int c = g; c < C; c += G) s += expf(x[c] - m);
#pragma unroll
    for (int o = G / 2; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (!live) return;
    const int label = labels[row];
    const bool ok = label >= 0 && label < C;
    const float nan = __builtin_nanf("");
    const float inv_s = 1.f / s;
    float* d = d_logits + row * (int64_t)ldd;
    for (int c = g; c < C; c += G) d[c] = ok ? (expf(x[c] - m) * inv_s - (c == label ? 1.f : 0.f)) * inv_n : nan;
    if (g == 0) {
        row_loss[row] = ok ? (logf(s) + m) - x[label] : nan;
        correct[row] = ok && arg == label ? 1 : 0;
    }
}

// The one-cell index arrays of a classifier batch (launch_cell_index for cell_ptr = [0, n] without a device cell_ptr): the
// reference hands the whole DataLoader batch to PointNet2.forward as ONE PyG batch, so every object's cell starts at object 0.
__global__ void k_one_cell_index(int32_t n, int32_t* __restrict__ seg_ptr_local, int32_t* __restrict__ first, uint32_t* guard) {
    if (guard != nullptr && blockIdx.x == 0 && threadIdx.x < G_SLOTS) guard[threadIdx.x] = 0u;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        seg_ptr_local[0] = 0;
        seg_ptr_local[1] = n;
    }
    for (int o = blockIdx.x * blockDim.x + threadIdx.x; o < n; o += gridDim.x * blockDim.x) first[o] = 0;
}

}  // namespace

int launch_classifier_heads(const float* f2, const float* w, const float* bias, int64_t n, int C1, int C2, float* class_pred,
                            float* color_pred, hipStream_t st) {
    if (n == 0) return 0;
    const int C = C1 + C2;
    const int rows = kHeadThreads / C < 32 ? kHeadThreads / C : 32;
    const size_t lds = ((size_t)kHeadK * C + (size_t)rows * kHeadK) * sizeof(float);   // <= 130 KB at C = 128
    // (the attribute is set once per device: reserve what the widest supported pair of heads takes, C = 128)
    T2P_TRY(reserve_lds((const void*)k_classifier_heads, ((size_t)kHeadK * 128 + 2 * kHeadK) * sizeof(float), "classifier_heads"));
    int64_t wgs = (n + rows - 1) / rows;
    const int64_t cap = 2 * (int64_t)num_cus();
    if (wgs > cap) wgs = cap;
    ProfScope ps_("classifier_heads", st);
    hipLaunchKernelGGL(k_classifier_heads, dim3((unsigned)wgs), dim3(kHeadThreads), lds, st, f2, w, bias, n, C1, C2, class_pred,
                       color_pred);
    T2P_CHECK_LAUNCH("classifier_heads");
    return 0;
}

int launch_softmax_xent(const float* logits, int ld, const int32_t* labels, int64_t n, int C, float* row_loss, float* d_logits,
                        int ldd, int32_t* correct, hipStream_t st) {
    if (n == 0) return 0;
    const float inv_n = 1.f / (float)n;
    const int G = C > 32 ? 64 : (C > 16 ? 32 : (C > 8 ? 16 : 8));
    const unsigned blocks = (unsigned)((n * G + 255) / 256);
    ProfScope ps_("softmax_xent", st);
#define T2P_XENT(GG)                                                                                                       \
    hipLaunchKernelGGL(k_softmax_xent<GG>, dim3(blocks), dim3(256), 0, st, logits, ld, labels, n, C, inv_n, row_loss, d_logits, \
                       ldd, correct)
    if (G == 64)
        T2P_XENT(64);
    else if (G == 32)
        T2P_XENT(32);
    else if (G == 16)
        T2P_XENT(16);
    else
        T2P_XENT(8);
#undef T2P_XENT
    T2P_CHECK_LAUNCH("softmax_xent");
    return 0;
}

int launch_one_cell_index(int64_t n, int32_t* seg_ptr_local, int32_t* first, hipStream_t st, uint32_t* guard_to_clear) {
    const unsigned blocks = (unsigned)((n + 255) / 256 > 0 ? (n + 255) / 256 : 1);
    hipLaunchKernelGGL(k_one_cell_index, dim3(blocks > 1024 ? 1024 : blocks), dim3(256), 0, st, (int32_t)n, seg_ptr_local, first,
                       guard_to_clear);
    T2P_CHECK_LAUNCH("one_cell_index");
    return 0;
}

}  // namespace t2p
