// The per-step statistics of the fine stage's training loop in one launch (t2p_fine_step_stats).
//
// Replaces (reference): calc_recall_precision training/losses.py:33-62, calc_pose_error training/losses.py:81-123 with
// get_pos_in_cell models/superglue_matcher.py:139-161, as training/fine.py:77-112 calls them once per step on host copies of
// matches0, matches1 and offsets.  Here the model's outputs stay on the device: the ground truth comes from three tables the feed
// uploads once (training.SceneFineFeed), indexed by the batch's pose indices, and the seven figures of a step leave as ONE row of
// float64 (56 bytes) - the loop's only device-to-host copy.
//
// A latency kernel: B samples of at most 63 slots.  One workgroup of kStatThreads; wavefront w takes samples w, w + 16, ..., lane i
// slot i of the sample (and, for the range check of matches1, hint i).  Counts and the float64 sums of the pose estimate are reduced
// over the wavefront with a fixed xor butterfly; lane 0 writes the sample's row to sample_stats and to LDS.  Behind one barrier,
// thread k < 5 sums column k of the LDS rows in ascending sample order and divides by B; threads 5 and 6 widen the two fp32 losses.
// No atomics: the same bits from call to call.  Every output element is written on every path.
// A sample with a pose index outside the tables, a matches0 value outside [-1, N), a matches1 value outside [-1, M) or a table
// entry gt_hint outside [-1, N) gets a row of NaN; nothing is read through such an index (the loads behind it are predicated off).
#include "t2p_common.h"

#include "../../include/t2p.h"

namespace t2p {
namespace {

constexpr int kStatThreads = 1024;       // 16 wavefronts: a sample is a chain of dependent loads, so samples run side by side
constexpr int kStatCols = 5;             // recall, precision, pose_mid, pose_mean, pose_offsets
constexpr int kStatMaxBatch = 1024;      // the LDS rows of the batch reduction: 1024 x 5 doubles = 40 KiB (T2P_FINE_STATS_MAX_BATCH)
constexpr int kStatMaxTokens = 63;       // t2p_match_attention's limit: a wavefront's lanes cover a set

__global__ __launch_bounds__(kStatThreads) void k_fine_step_stats(
    const int64_t* __restrict__ matches0, const int64_t* __restrict__ matches1, const float* __restrict__ offsets,
    const int32_t* __restrict__ pose_idx, const int32_t* __restrict__ gt_hint, const double* __restrict__ pose_xy,
    const double* __restrict__ slot_center_xy, int64_t n_rows, int B, int M, int N, const float* __restrict__ loss,
    const float* __restrict__ loss_offsets, double* __restrict__ sample_stats, double* __restrict__ step_row) {
    __shared__ double rows[kStatMaxBatch * kStatCols];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const double nan = __builtin_nan("");
    for (int b = wave; b < B; b += kStatThreads / 64) {
        const int64_t p = pose_idx[b];
        const bool pose_ok = p >= 0 && p < n_rows;
        bool ok = pose_ok;
        int64_t m0 = -1;
        int gt = -1;
        if (lane < M) {
            m0 = matches0[(int64_t)b * M + lane];
            if (m0 < -1 || m0 >= N) ok = false;
            if (pose_ok) {
                gt = gt_hint[p * M + lane];
                if (gt < -1 || gt >= N) ok = false;
            }
        }
        if (lane < N) {
            const int64_t m1 = matches1[(int64_t)b * N + lane];
            if (m1 < -1 || m1 >= M) ok = false;
        }
        ok = __all(ok);                                      // from here on every index of the sample is in range, or nothing is read
        int pair = 0, found = 0, assigned = 0, right = 0;
        double cx = 0.0, cy = 0.0, ox = 0.0, oy = 0.0;
        if (ok && lane < M) {
            if (gt >= 0) {
                pair = 1;
                found = (m0 == gt || matches1[(int64_t)b * N + gt] == lane) ? 1 : 0;
            }
            if (m0 >= 0) {
                assigned = 1;
                right = gt == (int)m0 ? 1 : 0;
                const double* c = slot_center_xy + ((int64_t)p * M + lane) * 2;
                const float* o = offsets + ((int64_t)b * N + m0) * 2;
                cx = c[0];
                cy = c[1];
                ox = cx + (double)o[0];
                oy = cy + (double)o[1];
            }
        }
        pair = wave_sum(pair);
        found = wave_sum(found);
        assigned = wave_sum(assigned);
        right = wave_sum(right);
        cx = wave_sum(cx);
        cy = wave_sum(cy);
        ox = wave_sum(ox);
        oy = wave_sum(oy);
        if (lane == 0) {
            double r[kStatCols];
            if (ok) {
                const double tx = pose_xy[2 * p], ty = pose_xy[2 * p + 1];
                const double k = (double)assigned;
                const double mx = assigned ? cx / k : 0.5, my = assigned ? cy / k : 0.5;
                const double fx = assigned ? ox / k : 0.5, fy = assigned ? oy / k : 0.5;
                r[0] = pair ? (double)found / (double)pair : 0.0;
                r[1] = assigned ? (double)right / k : 0.0;
                r[2] = sqrt((tx - 0.5) * (tx - 0.5) + (ty - 0.5) * (ty - 0.5));
                r[3] = sqrt((tx - mx) * (tx - mx) + (ty - my) * (ty - my));
                r[4] = sqrt((tx - fx) * (tx - fx) + (ty - fy) * (ty - fy));
            } else {
#pragma unroll
                for (int k = 0; k < kStatCols; k++) r[k] = nan;
            }
#pragma unroll
            for (int k = 0; k < kStatCols; k++) {
                sample_stats[(int64_t)b * kStatCols + k] = r[k];
                rows[b * kStatCols + k] = r[k];
            }
        }
    }
    __syncthreads();
    if (threadIdx.x < kStatCols) {
        double t = 0.0;
        for (int b = 0; b < B; b++) t += rows[b * kStatCols + threadIdx.x];       // ascending sample order
        step_row[2 + threadIdx.x] = t / (double)B;
    } else if (threadIdx.x == kStatCols) {
        step_row[0] = loss ? (double)loss[0] : nan;
    } else if (threadIdx.x == kStatCols + 1) {
        step_row[1] = loss_offsets ? (double)loss_offsets[0] : nan;
    }
}

}  // namespace
}  // namespace t2p

using namespace t2p;

extern "C" {

int t2p_fine_step_stats(const int64_t* matches0, const int64_t* matches1, const float* offsets, const int32_t* pose_idx,
                        int64_t batch, int32_t n_obj, int32_t n_hints, const int32_t* gt_hint, const double* pose_xy,
                        const double* slot_center_xy, int64_t n_rows, const float* loss, const float* loss_offsets,
                        double* sample_stats, double* step_row, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(matches0 && matches1 && offsets && pose_idx && gt_hint && pose_xy && slot_center_xy && sample_stats && step_row,
                  "fine_step_stats: NULL argument");
    T2P_CHECK_ARG(batch >= 1 && n_obj >= 1 && n_hints >= 1, "fine_step_stats: need batch, n_obj, n_hints >= 1 (got %lld, %d, %d)",
                  (long long)batch, n_obj, n_hints);
    T2P_CHECK_ARG(n_obj <= kStatMaxTokens && n_hints <= kStatMaxTokens,
                  "fine_step_stats: n_obj and n_hints must not exceed 63, the token limit of t2p_match_attention (got %d, %d)", n_obj,
                  n_hints);
    T2P_CHECK_ARG(batch <= kStatMaxBatch, "fine_step_stats: batch %lld exceeds %d, the samples the batch reduction holds in LDS",
                  (long long)batch, kStatMaxBatch);
    T2P_CHECK_ARG(n_rows >= 1 && n_rows <= 0x3fffffff, "fine_step_stats: need 1 <= n_rows < 2^30 table rows (got %lld)", (long long)n_rows);
    ProfScope ps_("fine_step_stats", st);
    hipLaunchKernelGGL(k_fine_step_stats, dim3(1), dim3(kStatThreads), 0, st, matches0, matches1, offsets, pose_idx, gt_hint, pose_xy,
                       slot_center_xy, n_rows, (int)batch, n_obj, n_hints, loss, loss_offsets, sample_stats, step_row);
    T2P_CHECK_LAUNCH("fine_step_stats");
    return 0;
}

}  // extern "C"
