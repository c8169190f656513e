// Library infrastructure (error text, device caches, opt-in kernel timing) and the extern "C" entry points of libt2p_hip.so
// (include/t2p.h) other than the cell encoder's (cell_encoder.hip): the text encoder, the LSTM training loops, thin exports.
#include <stdarg.h>
#include <stdlib.h>
#include <math.h>
#include <string.h>

#include <mutex>
#include <set>
#include <utility>

#include "../../include/t2p.h"
#include "../../include/t2p_serve.h"
#include "../../include/t2p_select.h"
#include "t2p_common.h"

namespace t2p {

static thread_local char g_err[512] = "";

void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}

int num_cus() {
    static int cached = 0;
    if (cached == 0) {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess)
            cached = prop.multiProcessorCount;
        if (cached <= 0) cached = 256;
    }
    return cached;
}

// Workgroups of the three persistent matrix kernels (k_sa3, k_sa_rows, k_ga2: one workgroup fills a CU).  Development switch
// T2P_MATRIX_WGS=<n>: fewer than one per CU leaves whole CUs to the kernels of the other HIP stream (notebook, round 4).
int matrix_wgs() {
    static int cached = 0;
    if (cached == 0) {
        cached = num_cus();
        const char* e = getenv("T2P_MATRIX_WGS");
        if (e != nullptr && atoi(e) >= 8 && atoi(e) <= cached) cached = atoi(e) / 8 * 8;
    }
    return cached;
}

int reserve_lds(const void* kernel, size_t bytes, const char* what) {
    static std::mutex mu;
    static std::set<std::pair<int, const void*>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.count({dev, kernel})) return 0;
    hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) {
        set_error("%s: cannot reserve %zu B of LDS on device %d: %s", what, bytes, dev, hipGetErrorString(e));
        return (int)e;
    }
    done.insert({dev, kernel});
    return 0;
}

// ---- opt-in kernel timing ---------------------------------------------------------------------------------------
// The only process-global state of the library besides the caches above: a ring of event pairs, guarded by one mutex
// (launches from several host threads may be recorded; the lock is taken only while profiling is on).
struct ProfRec {
    const char* name;
    hipEvent_t a, b;
};
static std::mutex g_prof_mu;
static volatile bool g_prof_on = false;
static ProfRec g_prof[8192];
static int g_prof_n = 0;

static char g_repeat_name[64] = {0};
static volatile int g_repeat_n = 1;

ProfScope::ProfScope(const char* name, hipStream_t s) : slot(-1), st(s), reps(1) {
    if (g_repeat_n > 1 && strncmp(name, g_repeat_name, sizeof(g_repeat_name)) == 0) reps = g_repeat_n;
    if (!g_prof_on) return;
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess) return;
    if (hipEventCreate(&b) != hipSuccess) {
        (void)hipEventDestroy(a);
        return;
    }
    {
        std::lock_guard<std::mutex> lock(g_prof_mu);
        if (g_prof_n < 8192) {
            slot = g_prof_n++;
            g_prof[slot].name = name;
            g_prof[slot].a = a;
            g_prof[slot].b = b;
        }
    }
    if (slot < 0) {
        (void)hipEventDestroy(a);
        (void)hipEventDestroy(b);
        return;
    }
    ev_end = b;
    (void)hipEventRecord(a, st);
}
ProfScope::~ProfScope() {
    if (slot >= 0) (void)hipEventRecord((hipEvent_t)ev_end, st);
}

}  // namespace t2p

using namespace t2p;

extern "C" {

int t2p_abi_version(void) { return T2P_ABI_VERSION; }
int t2p_serve_abi_version(void) { return T2P_SERVE_ABI_VERSION; }
int t2p_select_abi_version(void) { return T2P_SELECT_ABI_VERSION; }

void t2p_profile_enable(int on) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_prof_on = on != 0;
}

// Measurement hook (profiles/energy_table.py): launches recorded under `scope` are issued `reps` times back to back.
void t2p_profile_repeat(const char* scope, int reps) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    g_repeat_n = 1;
    if (scope != nullptr && reps > 1) {
        strncpy(g_repeat_name, scope, sizeof(g_repeat_name) - 1);
        g_repeat_name[sizeof(g_repeat_name) - 1] = 0;
        g_repeat_n = reps;
    }
}

// Waits for the recorded launches, writes one line per kernel name: "<name> <launches> <total_ms>\n", clears.
int t2p_profile_report(char* buf, size_t n) {
    std::lock_guard<std::mutex> lock(g_prof_mu);
    size_t off = 0;
    if (n > 0) buf[0] = 0;
    for (int i = 0; i < g_prof_n; i++) {
        if (g_prof[i].name == nullptr) continue;
        int cnt = 0;
        double tot = 0.0;
        for (int j = i; j < g_prof_n; j++) {
            if (g_prof[j].name == nullptr || strcmp(g_prof[j].name, g_prof[i].name) != 0) continue;
            float ms = 0.f;
            if (hipEventSynchronize(g_prof[j].b) == hipSuccess && hipEventElapsedTime(&ms, g_prof[j].a, g_prof[j].b) == hipSuccess) {
                tot += ms;
                cnt++;
            }
            (void)hipEventDestroy(g_prof[j].a);
            (void)hipEventDestroy(g_prof[j].b);
            if (j != i) g_prof[j].name = nullptr;
        }
        int w = snprintf(buf + off, off < n ? n - off : 0, "%s %d %.6f\n", g_prof[i].name, cnt, tot);
        if (w > 0) off += (size_t)w;
        g_prof[i].name = nullptr;
    }
    g_prof_n = 0;
    return 0;
}
const char* t2p_last_error(void) { return g_err; }

int t2p_classifier_heads(const float* features2, const float* head_w, const float* head_b, int64_t n, int32_t n_classes,
                         int32_t n_colors, float* class_pred, float* color_pred, t2p_stream_t stream) {
    T2P_CHECK_ARG(features2 && head_w && head_b && class_pred && color_pred, "classifier_heads: NULL argument");
    T2P_CHECK_ARG(n >= 0, "classifier_heads: negative size");
    if (n_classes < 1 || n_classes > 64 || n_colors < 1 || n_colors > 64) {
        set_error("classifier_heads: n_classes=%d / n_colors=%d outside [1, 64]", n_classes, n_colors);
        return T2P_E_UNSUPPORTED;
    }
    T2P_CHECK_ARG(((uintptr_t)features2 & 15) == 0, "classifier_heads: features2 must be 16-byte aligned");
    return launch_classifier_heads(features2, head_w, head_b, n, n_classes, n_colors, class_pred, color_pred, (hipStream_t)stream);
}

int t2p_softmax_xent(const float* logits, int32_t ld_logits, const int32_t* labels, int64_t n, int32_t n_classes, float* row_loss,
                     float* d_logits, int32_t ld_d, int32_t* correct, t2p_stream_t stream) {
    T2P_CHECK_ARG(logits && labels && row_loss && d_logits && correct, "softmax_xent: NULL argument");
    T2P_CHECK_ARG(n >= 0 && n_classes >= 1, "softmax_xent: n=%lld, n_classes=%d", (long long)n, n_classes);
    T2P_CHECK_ARG(ld_logits >= n_classes && ld_d >= n_classes, "softmax_xent: row pitch below n_classes=%d", n_classes);
    return launch_softmax_xent(logits, ld_logits, labels, n, n_classes, row_loss, d_logits, ld_d, correct, (hipStream_t)stream);
}

size_t t2p_encode_text_workspace_bytes(int64_t batch, int32_t vocab, int32_t embed_dim) {
    const size_t D = embed_dim;
    return align_up((size_t)2 * (vocab + 1) * 4 * D * sizeof(float), 256) + align_up((size_t)2 * batch * D * sizeof(float), 256) +
           align_up((size_t)batch * D * sizeof(float), 256) + 256;
}

int t2p_encode_text(const int32_t* tokens, const int32_t* lengths, int64_t batch, int32_t max_len, int32_t vocab,
                    int32_t embed_dim, const t2p_text_weights* w, float* out_raw, float* out, void* workspace,
                    size_t workspace_bytes, t2p_stream_t stream) {
    hipStream_t st = (hipStream_t)stream;
    T2P_CHECK_ARG(w != nullptr && tokens != nullptr && lengths != nullptr && out != nullptr, "encode_text: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && batch < (1 << 30) && max_len >= 1 && vocab >= 1, "encode_text: bad sizes");
    if (batch == 0) return 0;
    const size_t need = t2p_encode_text_workspace_bytes(batch, vocab, embed_dim);
    if (workspace == nullptr || workspace_bytes < need) {
        set_error("encode_text: workspace %zu B < required %zu B", workspace_bytes, need);
        return T2P_E_WORKSPACE;
    }
    const int D = embed_dim;
    Bump b{(char*)workspace, 0, workspace_bytes};
    const int rows = vocab + 1;   // + one zero row per direction (lstm.hip)
    float* table = b.take<float>((size_t)2 * rows * 4 * D);
    float* hdir = b.take<float>((size_t)2 * batch * D);
    float* raw = out_raw ? out_raw : b.take<float>((size_t)batch * D);
    // gate table [dir][V][4D] = embedding [V][D] x W_ih^T [D][4D] + (b_ih + b_hh)
    for (int dir = 0; dir < 2; dir++) {
        T2P_TRY(launch_gemm(w->embedding, D, w->w_ih + (size_t)dir * D * 4 * D, w->bias + (size_t)dir * 4 * D,
                            table + (size_t)dir * rows * 4 * D, 4 * D, 0, vocab, D, 4 * D, 0, st));
        hipError_t e = hipMemsetAsync(table + ((size_t)dir * rows + vocab) * 4 * D, 0, (size_t)4 * D * sizeof(float), st);
        if (e != hipSuccess) {
            set_error("encode_text: memset failed: %s", hipGetErrorString(e));
            return (int)e;
        }
    }
    T2P_TRY(launch_bilstm_impl(table, w->w_hh, w->w_hh_x3, w->w_hh_scale, tokens, lengths, (int)batch, max_len, rows, D, hdir, raw, st));
    T2P_TRY(launch_rownorm(raw, D, batch, D, out, D, 0, st));
    return 0;
}

int t2p_lstm_cell_forward(const float* pre, const float* gate_table, const int32_t* tokens, const int32_t* lengths,
                          int64_t batch, int32_t max_len, int32_t embed_dim, int32_t step, int32_t reverse, const float* c_prev,
                          const float* h_prev, float* gates, float* c, float* h, t2p_stream_t stream) {
    T2P_CHECK_ARG(pre && gate_table && tokens && lengths && c_prev && h_prev && gates && c && h, "lstm_cell_forward: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && max_len >= 1 && embed_dim >= 1 && step >= 0 && step < max_len, "lstm_cell_forward: bad sizes");
    return launch_lstm_cell_fwd(pre, gate_table, tokens, lengths, batch, max_len, embed_dim, step, reverse, c_prev, h_prev, gates,
                                c, h, (hipStream_t)stream);
}

int t2p_lstm_cell_backward(const float* dh_gemm, const float* dh_carry_in, const float* dc_in, const float* gates,
                           const float* c_prev, const float* c, const int32_t* lengths, int64_t batch, int32_t embed_dim,
                           int32_t step, float* d_pre, float* dc_out, float* dh_carry_out, t2p_stream_t stream) {
    T2P_CHECK_ARG(dh_carry_in && dc_in && gates && c_prev && c && lengths && d_pre && dc_out && dh_carry_out,
                  "lstm_cell_backward: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && embed_dim >= 1 && step >= 0, "lstm_cell_backward: bad sizes");
    return launch_lstm_cell_bwd(dh_gemm, dh_carry_in, dc_in, gates, c_prev, c, lengths, batch, embed_dim, step, d_pre, dc_out,
                                dh_carry_out, (hipStream_t)stream);
}

int t2p_lstm_train_forward(const float* gate_table, const float* w_hh_k, const int32_t* tokens, const int32_t* lengths,
                           int64_t batch, int32_t max_len, int32_t embed_dim, int32_t reverse, float* gates, float* cs, float* hs,
                           float* pre_ws, t2p_stream_t stream) {
    T2P_CHECK_ARG(gate_table && w_hh_k && tokens && lengths && gates && cs && hs && pre_ws, "lstm_train_forward: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && max_len >= 1 && embed_dim >= 1, "lstm_train_forward: bad sizes");
    if (embed_dim % 4 != 0) {
        set_error("lstm_train_forward: embed_dim=%d is not a multiple of 4", embed_dim);
        return T2P_E_UNSUPPORTED;
    }
    if (batch == 0) return 0;
    const int D = embed_dim;
    const size_t bd = (size_t)batch * D;
    hipStream_t st = (hipStream_t)stream;
    for (int s = 0; s < max_len; s++) {       // the time loop of modules._LstmTrainFn.forward, one launch pair per step
        T2P_TRY(launch_gemm_skinny(hs + s * bd, D, w_hh_k, pre_ws, 4 * D, batch, D, 4 * D, st));
        T2P_TRY(launch_lstm_cell_fwd(pre_ws, gate_table, tokens, lengths, batch, max_len, D, s, reverse, cs + s * bd, hs + s * bd,
                                     gates + (size_t)s * batch * 4 * D, cs + (s + 1) * bd, hs + (s + 1) * bd, st));
    }
    return 0;
}

int t2p_lstm_train_backward(const float* dh_last, const float* w_hh_t, const float* gates, const float* cs, const int32_t* lengths,
                            int64_t batch, int32_t max_len, int32_t embed_dim, float* d_pre, float* ws, t2p_stream_t stream) {
    T2P_CHECK_ARG(dh_last && w_hh_t && gates && cs && lengths && d_pre && ws, "lstm_train_backward: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && max_len >= 1 && embed_dim >= 1, "lstm_train_backward: bad sizes");
    if (embed_dim % 4 != 0) {
        set_error("lstm_train_backward: embed_dim=%d is not a multiple of 4", embed_dim);
        return T2P_E_UNSUPPORTED;
    }
    if (batch == 0) return 0;
    const int D = embed_dim;
    const size_t bd = (size_t)batch * D;
    hipStream_t st = (hipStream_t)stream;
    float* dc[2] = {ws, ws + bd};              // ws: [5][B][D] = dc ping-pong | dh_carry ping-pong | dh_gemm
    float* carry[2] = {ws + 2 * bd, ws + 3 * bd};
    float* dh_gemm = ws + 4 * bd;
    hipError_t e = hipMemsetAsync(dc[0], 0, bd * sizeof(float), st);
    if (e == hipSuccess) e = hipMemcpyAsync(carry[0], dh_last, bd * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) {
        set_error("lstm_train_backward: %s", hipGetErrorString(e));
        return (int)e;
    }
    int cur = 0;
    for (int s = max_len - 1; s >= 0; s--) {
        T2P_TRY(launch_lstm_cell_bwd(s == max_len - 1 ? nullptr : dh_gemm, carry[cur], dc[cur], gates + (size_t)s * batch * 4 * D,
                                     cs + s * bd, cs + (s + 1) * bd, lengths, batch, D, s, d_pre + (size_t)s * batch * 4 * D,
                                     dc[cur ^ 1], carry[cur ^ 1], st));
        if (s > 0) T2P_TRY(launch_gemm_skinny(d_pre + (size_t)s * batch * 4 * D, 4 * D, w_hh_t, dh_gemm, D, batch, 4 * D, D, st));
        cur ^= 1;
    }
    return 0;
}

int t2p_pairwise_ranking(const float* scores, int32_t batch, float margin, float* row_loss, float* d_scores, float* row_count,
                         t2p_stream_t stream) {
    T2P_CHECK_ARG(scores && row_loss && d_scores && row_count, "pairwise_ranking: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && batch <= 32768, "pairwise_ranking: batch=%d outside [0, 32768]", batch);
    return launch_pairwise_ranking(scores, batch, margin, row_loss, d_scores, row_count, (hipStream_t)stream);
}

size_t t2p_bn_train_workspace_bytes(int64_t rows, int32_t n_seg, int32_t channels) {
    return bn_train_workspace_bytes(rows, n_seg, channels);
}

int t2p_bn_relu_train_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int64_t rows, int32_t channels,
                              const float* gamma, const float* beta, float eps, int32_t relu, float* y, float* mean,
                              float* invstd, float* var_unbiased, void* workspace, size_t workspace_bytes,
                              t2p_stream_t stream) {
    T2P_CHECK_ARG(x && seg_ptr && gamma && beta && y && mean && invstd && var_unbiased, "bn_relu_train_forward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1 && rows >= 0, "bn_relu_train_forward: bad sizes");
    if (n_seg > 0 && (workspace == nullptr || workspace_bytes < bn_train_workspace_bytes(rows, n_seg, channels))) {
        set_error("bn_relu_train_forward: workspace %zu B < required %zu B", workspace_bytes,
                  bn_train_workspace_bytes(rows, n_seg, channels));
        return T2P_E_WORKSPACE;
    }
    return launch_bn_relu_train_forward(x, seg_ptr, n_seg, rows, channels, gamma, beta, eps, relu, y, mean, invstd,
                                        var_unbiased, (double*)workspace, (hipStream_t)stream);
}

int t2p_bn_relu_train_backward(const float* dy, const float* x, const float* beta, const int32_t* seg_ptr, int32_t n_seg,
                               int64_t rows, int32_t channels, const float* mean, const float* invstd, const float* gamma,
                               int32_t relu, float* dx, float* dgamma_seg, float* dbeta_seg, void* workspace,
                               size_t workspace_bytes, t2p_stream_t stream) {
    T2P_CHECK_ARG(dy && x && beta && seg_ptr && mean && invstd && gamma && dx && dgamma_seg && dbeta_seg,
                  "bn_relu_train_backward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1 && rows >= 0, "bn_relu_train_backward: bad sizes");
    if (n_seg > 0 && (workspace == nullptr || workspace_bytes < bn_train_workspace_bytes(rows, n_seg, channels))) {
        set_error("bn_relu_train_backward: workspace %zu B < required %zu B", workspace_bytes,
                  bn_train_workspace_bytes(rows, n_seg, channels));
        return T2P_E_WORKSPACE;
    }
    return launch_bn_relu_train_backward(dy, x, beta, seg_ptr, n_seg, rows, channels, mean, invstd, gamma, relu, dx, dgamma_seg,
                                         dbeta_seg, (double*)workspace, (hipStream_t)stream);
}

int t2p_edge_features_forward(const float* x, const float* pos, const float* pos_c, const int32_t* src, const int32_t* dst,
                              int64_t n_edges, int32_t channels, int32_t width, float* out, t2p_stream_t stream) {
    T2P_CHECK_ARG(pos && pos_c && src && dst && out && (x || channels == 0), "edge_features_forward: NULL argument");
    T2P_CHECK_ARG(n_edges >= 0 && channels >= 0, "edge_features_forward: bad sizes");
    return launch_edge_feat_fwd(x, pos, pos_c, src, dst, n_edges, channels, width, out, (hipStream_t)stream);
}
int t2p_edge_features_backward(const float* d_out, const int32_t* src, int64_t n_edges, int32_t channels, int32_t width, float* dx,
                               t2p_stream_t stream) {
    T2P_CHECK_ARG(d_out && src && (dx || channels == 0), "edge_features_backward: NULL argument");
    T2P_CHECK_ARG(n_edges >= 0 && channels >= 0, "edge_features_backward: bad sizes");
    return launch_edge_feat_bwd(d_out, src, n_edges, channels, width, dx, (hipStream_t)stream);
}
int t2p_pair_features_forward(const float* x, const int32_t* tgt, const int32_t* src, int64_t n_edges, int32_t dim, float* out,
                              t2p_stream_t stream) {
    T2P_CHECK_ARG(x && tgt && src && out, "pair_features_forward: NULL argument");
    T2P_CHECK_ARG(n_edges >= 0 && dim >= 1, "pair_features_forward: bad sizes");
    return launch_pair_feat_fwd(x, tgt, src, n_edges, dim, out, (hipStream_t)stream);
}
int t2p_pair_features_backward(const float* d_out, const int32_t* tgt, const int32_t* src, int64_t n_edges, int32_t dim,
                               float* dx, t2p_stream_t stream) {
    T2P_CHECK_ARG(d_out && tgt && src && dx, "pair_features_backward: NULL argument");
    T2P_CHECK_ARG(n_edges >= 0 && dim >= 1, "pair_features_backward: bad sizes");
    return launch_pair_feat_bwd(d_out, tgt, src, n_edges, dim, dx, (hipStream_t)stream);
}
int t2p_rownorm_backward(const float* x, const float* dy, int64_t n_rows, int32_t dim, float* dx, t2p_stream_t stream) {
    T2P_CHECK_ARG(x && dy && dx, "rownorm_backward: NULL argument");
    T2P_CHECK_ARG(n_rows >= 0 && dim >= 1, "rownorm_backward: bad sizes");
    return launch_rownorm_bwd(x, dy, n_rows, dim, dx, (hipStream_t)stream);
}

int t2p_segment_mean_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* out,
                             t2p_stream_t stream) {
    T2P_CHECK_ARG(x && seg_ptr && out, "segment_mean_forward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1, "segment_mean_forward: bad sizes");
    return launch_segment_mean(x, seg_ptr, n_seg, channels, out, (hipStream_t)stream);
}
int t2p_segment_mean_backward(const float* dout, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* dx,
                              t2p_stream_t stream) {
    T2P_CHECK_ARG(dout && seg_ptr && dx, "segment_mean_backward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1, "segment_mean_backward: bad sizes");
    return launch_segment_mean_backward(dout, seg_ptr, n_seg, channels, dx, (hipStream_t)stream);
}

int t2p_segment_max_forward(const float* x, const int32_t* seg_ptr, int32_t n_seg, int32_t channels, float* out, int32_t* arg,
                            t2p_stream_t stream) {
    T2P_CHECK_ARG(x && seg_ptr && out && arg, "segment_max_forward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1, "segment_max_forward: bad sizes");
    return launch_segment_max(x, seg_ptr, n_seg, channels, out, arg, (hipStream_t)stream);
}

int t2p_segment_max_backward(const float* dout, const int32_t* arg, const int32_t* seg_ptr, int32_t n_seg, int32_t channels,
                             float* dx, t2p_stream_t stream) {
    T2P_CHECK_ARG(dout && arg && seg_ptr && dx, "segment_max_backward: NULL argument");
    T2P_CHECK_ARG(n_seg >= 0 && channels >= 1, "segment_max_backward: bad sizes");
    return launch_segment_max_backward(dout, arg, seg_ptr, n_seg, channels, dx, (hipStream_t)stream);
}

int t2p_hardest_ranking(const float* scores, int32_t batch, float margin, float* best, int32_t* where, float* d_scores,
                        t2p_stream_t stream) {
    T2P_CHECK_ARG(scores && best && where && d_scores, "hardest_ranking: NULL argument");
    T2P_CHECK_ARG(batch >= 0 && batch <= 32768, "hardest_ranking: batch=%d outside [0, 32768]", batch);
    return launch_hardest_ranking(scores, batch, margin, best, where, d_scores, (hipStream_t)stream);
}

size_t t2p_sim_topk_workspace_bytes(int64_t nq, int64_t nc, int32_t k) { return sim_topk_workspace_bytes(nq, nc, k); }

// (the three calls' sizes and pointers are checked in sim_topk.hip, once, under each call's name)

int t2p_sim_topk(const float* queries, const float* cells, int64_t nq, int64_t nc, int32_t dim, int32_t k,
                 int64_t index_offset, int64_t* out_idx, double* out_score, void* workspace, size_t workspace_bytes,
                 t2p_stream_t stream) {
    return launch_sim_topk(queries, cells, nq, nc, dim, k, index_offset, out_idx, out_score, workspace, workspace_bytes,
                           (hipStream_t)stream);
}

int t2p_sim_topk_grouped(const float* queries, const float* cells, const int32_t* query_group, const int32_t* cell_group,
                         int64_t nq, int64_t nc, int32_t dim, int32_t k, int64_t index_offset, int64_t* out_idx,
                         double* out_score, void* workspace, size_t workspace_bytes, t2p_stream_t stream) {
    return launch_sim_topk_grouped(queries, cells, query_group, cell_group, nq, nc, dim, k, index_offset, out_idx, out_score,
                                   workspace, workspace_bytes, (hipStream_t)stream);
}

int t2p_sim_topk_prior(const float* queries, const float* cells, const double* query_xy, const double* query_radius,
                       const double* cell_box, const int32_t* query_group, const int32_t* cell_group, int64_t nq, int64_t nc,
                       int32_t dim, int32_t k, int64_t index_offset, int64_t* out_idx, double* out_score, void* workspace,
                       size_t workspace_bytes, t2p_stream_t stream) {
    return launch_sim_topk_prior(queries, cells, query_xy, query_radius, cell_box, query_group, cell_group, nq, nc, dim, k,
                                 index_offset, out_idx, out_score, workspace, workspace_bytes, (hipStream_t)stream);
}

int t2p_sa_balance(const uint16_t* n_rows, int32_t n, int32_t tile_rows, int32_t n_wg, int32_t* prefix, int32_t* bounds,
                   t2p_stream_t stream) {
    T2P_CHECK_ARG(n >= 0 && tile_rows >= 1 && n_wg >= 1, "sa_balance: n=%d tile_rows=%d n_wg=%d (n >= 0, tile_rows >= 1, n_wg >= 1)", n,
                  tile_rows, n_wg);
    T2P_CHECK_ARG((n_rows != nullptr || n == 0) && prefix != nullptr && bounds != nullptr, "sa_balance: NULL argument");
    return launch_sa_balance_arrays(n_rows, n, tile_rows, n_wg, prefix, bounds, (hipStream_t)stream);
}

int t2p_edge_counts(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, int64_t n_obj, int32_t n_dense,
                    int32_t n_cent, int32_t self_loops, int32_t* counts, t2p_stream_t stream) {
    T2P_CHECK_ARG(n_obj >= 0 && (n_obj == 0 || (rows && n_rows && first_obj && counts)), "edge_counts: NULL argument");
    return launch_edge_counts(rows, n_rows, first_obj, n_obj, n_dense, n_cent, self_loops, counts, (hipStream_t)stream);
}

int t2p_edge_expand(const uint16_t* rows, const uint16_t* n_rows, const int32_t* first_obj, const int32_t* cent_ptr, int64_t n_obj,
                    int32_t n_dense, int32_t n_cent, int32_t self_loops, int32_t* src, int32_t* dst, t2p_stream_t stream) {
    T2P_CHECK_ARG(n_obj >= 0 && (n_obj == 0 || (rows && n_rows && first_obj && cent_ptr)), "edge_expand: NULL argument");
    return launch_edge_expand(rows, n_rows, first_obj, cent_ptr, n_obj, n_dense, n_cent, self_loops, src, dst, (hipStream_t)stream);
}

int t2p_pack_objects(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* sample_idx,
                     const float* rot_cos_sin, int64_t n_obj, int32_t n_pts, float* xyz, float* rgb, float* center, float* mean_rgb,
                     t2p_stream_t stream) {
    T2P_CHECK_ARG(raw_xyz && raw_rgb && obj_ptr && sample_idx && xyz && rgb && center && mean_rgb, "pack_objects: NULL argument");
    T2P_CHECK_ARG(n_obj >= 0 && n_pts >= 1, "pack_objects: bad sizes");
    return launch_pack_objects(raw_xyz, raw_rgb, obj_ptr, sample_idx, rot_cos_sin, n_obj, n_pts, xyz, rgb, center, mean_rgb,
                               (hipStream_t)stream);
}

int t2p_pack_scene_objects(const float* raw_xyz, const float* raw_rgb, const int32_t* obj_ptr, const int32_t* obj_id,
                           const uint64_t* key, const float* scene_center, const float* scene_color, int64_t n_out, int32_t n_pts,
                           float* xyz, float* rgb, float* center, float* mean_rgb, int32_t* sample_idx_out, t2p_stream_t stream) {
    T2P_CHECK_ARG(n_out >= 0 && n_pts >= 1, "pack_scene_objects: bad sizes");
    T2P_CHECK_ARG(n_out == 0 || (raw_xyz && obj_ptr && obj_id && key && xyz), "pack_scene_objects: NULL argument");
    T2P_CHECK_ARG(n_out == 0 || rgb == nullptr || raw_rgb != nullptr, "pack_scene_objects: rgb wanted but raw_rgb is NULL");
    T2P_CHECK_ARG(n_out == 0 || ((center == nullptr || scene_center != nullptr) && (mean_rgb == nullptr || scene_color != nullptr)),
                  "pack_scene_objects: center / mean_rgb wanted but the scene table is NULL");
    return launch_pack_scene(raw_xyz, raw_rgb, obj_ptr, obj_id, key, scene_center, scene_color, n_out, n_pts, xyz, rgb, center,
                             mean_rgb, sample_idx_out, (hipStream_t)stream);
}

int t2p_pack_scene_objects_aug(const float* raw_xyz, const float* raw_rgb, const float* raw_mirror_xy, const int32_t* obj_ptr,
                               const int32_t* obj_id, const uint64_t* key, const uint8_t* flip, const float* rot_cos_sin,
                               const float* scene_center, const float* scene_center_mirror_xy, const float* scene_color,
                               int64_t n_out, int32_t n_pts, float* xyz, float* rgb, float* center, float* mean_rgb,
                               int32_t* sample_idx_out, t2p_stream_t stream) {
    T2P_CHECK_ARG(n_out >= 0 && n_pts >= 1, "pack_scene_objects_aug: bad sizes");
    T2P_CHECK_ARG(n_pts <= 1024, "pack_scene_objects_aug: n_pts=%d > 1024 (the sampled points of an object are staged in LDS)", n_pts);
    T2P_CHECK_ARG(flip == nullptr || raw_mirror_xy != nullptr,
                  "pack_scene_objects_aug: flip given but the scene has no mirror image (raw_mirror_xy is NULL)");
    T2P_CHECK_ARG(flip == nullptr || center == nullptr || scene_center_mirror_xy != nullptr,
                  "pack_scene_objects_aug: flip given and center wanted but scene_center_mirror_xy is NULL");
    T2P_CHECK_ARG(n_out == 0 || (raw_xyz && obj_ptr && obj_id && key && xyz), "pack_scene_objects_aug: NULL argument");
    T2P_CHECK_ARG(n_out == 0 || rgb == nullptr || raw_rgb != nullptr, "pack_scene_objects_aug: rgb wanted but raw_rgb is NULL");
    T2P_CHECK_ARG(n_out == 0 || ((center == nullptr || scene_center != nullptr) && (mean_rgb == nullptr || scene_color != nullptr)),
                  "pack_scene_objects_aug: center / mean_rgb wanted but the scene table is NULL");
    return launch_pack_scene_aug(raw_xyz, raw_rgb, raw_mirror_xy, obj_ptr, obj_id, key, flip, rot_cos_sin, scene_center,
                                 scene_center_mirror_xy, scene_color, n_out, n_pts, xyz, rgb, center, mean_rgb, sample_idx_out,
                                 (hipStream_t)stream);
}

int t2p_dedup_rows(const float* xyz, const float* rgb, int64_t n_obj, int32_t n_pts, uint16_t* rows, uint16_t* n_rows,
                   t2p_stream_t stream) {
    T2P_CHECK_ARG(n_obj >= 0, "dedup_rows: negative size");
    T2P_CHECK_ARG((((uintptr_t)xyz | (uintptr_t)rgb | (uintptr_t)rows) & 15) == 0, "dedup_rows: xyz, rgb and rows must be 16-byte aligned");
    return launch_dedup_rows(xyz, rgb, n_obj, n_pts, rows, n_rows, (n_pts + 1) / 2, (hipStream_t)stream);
}

int t2p_knn(const float* x, int32_t dim, const int32_t* seg_ptr, int32_t n_seg, int32_t max_seg_rows, int32_t k,
            int32_t* out_idx, t2p_stream_t stream) {
    return launch_knn(x, dim, seg_ptr, n_seg, max_seg_rows, k, out_idx, (hipStream_t)stream);
}

int t2p_gemm(const float* a, int32_t lda, const float* w, const float* bias, float* c, int32_t ldc, int32_t c0,
             int64_t m, int32_t k, int32_t n, int32_t relu, t2p_stream_t stream) {
    return launch_gemm(a, lda, w, bias, c, ldc, c0, m, k, n, relu, (hipStream_t)stream);
}

// sizes, operands and pitches of the stage-level GEMM exports (a NULL operand is allowed only for an empty product)
static int check_gemm_args(const char* what, const void* a, int lda, const void* w, const void* c, int ldc, int c0, int64_t m, int k, int n) {
    T2P_CHECK_ARG(m >= 0 && k >= 1 && n >= 1, "%s: bad sizes m=%lld k=%d n=%d", what, (long long)m, k, n);
    T2P_CHECK_ARG(m == 0 || (a && w && c), "%s: NULL argument", what);
    T2P_CHECK_ARG(lda >= k && c0 >= 0 && ldc >= c0 + n, "%s: lda=%d < k=%d or ldc=%d < c0 + n = %d", what, lda, k, ldc, c0 + n);
    return 0;
}

int t2p_gemm_residual(const float* a, int32_t lda, const float* w, const float* bias, float* c, int32_t ldc, int32_t c0,
                      int64_t m, int32_t k, int32_t n, int32_t relu, const float* resid, int32_t ldr, t2p_stream_t stream) {
    T2P_TRY(check_gemm_args("gemm_residual", a, lda, w, c, ldc, c0, m, k, n));
    T2P_CHECK_ARG(resid == nullptr || ldr >= n, "gemm_residual: ldr=%d < n=%d", ldr, n);
    return launch_gemm(a, lda, w, bias, c, ldc, c0, m, k, n, relu, (hipStream_t)stream, resid, ldr);
}

int t2p_gemm_x3(const float* a, int32_t lda, const void* wx, float scale, const float* bias, float* c, int32_t ldc, int32_t c0,
                int64_t m, int32_t k, int32_t n, int32_t relu, const float* resid, int32_t ldr, uint32_t* amax_in,
                t2p_stream_t stream) {
    T2P_TRY(check_gemm_args("gemm_x3", a, lda, wx, c, ldc, c0, m, k, n));
    T2P_CHECK_ARG(resid == nullptr || ldr >= n, "gemm_x3: ldr=%d < n=%d", ldr, n);
    int exp2_ = 0;
    T2P_CHECK_ARG(scale > 0.f && frexpf(scale, &exp2_) == 0.5f, "gemm_x3: scale=%g must be a power of two", (double)scale);
    return launch_gemm_x3(a, lda, wx, scale, bias, c, ldc, c0, m, k, n, relu, (hipStream_t)stream, resid, ldr, amax_in);
}

int t2p_gemm_skinny(const float* a, int32_t lda, const float* w, float* c, int32_t ldc, int64_t m, int32_t k, int32_t n,
                    t2p_stream_t stream) {
    T2P_TRY(check_gemm_args("gemm_skinny", a, lda, w, c, ldc, 0, m, k, n));
    return launch_gemm_skinny(a, lda, w, c, ldc, m, k, n, (hipStream_t)stream);
}

size_t t2p_gemm_tn_workspace_bytes(int64_t m, int32_t k1, int32_t n) { return gemm_tn_workspace_bytes(m, k1, n); }

int t2p_gemm_tn(const float* a, int32_t lda, const float* b, int32_t ldb, float* c, int32_t ldc, int64_t m, int32_t k1, int32_t n,
                void* workspace, size_t workspace_bytes, t2p_stream_t stream) {
    return launch_gemm_tn(a, lda, b, ldb, c, ldc, m, k1, n, workspace, workspace_bytes, (hipStream_t)stream);
}

size_t t2p_linear_wgrad_workspace_bytes(int64_t m, int32_t k1, int32_t n) { return linear_wgrad_workspace_bytes(m, k1, n); }

int t2p_linear_wgrad_f32(const float* dy, int32_t lda, const float* x, int32_t ldb, float* dw, int32_t ldc, float* colsum, int64_t m,
                         int32_t k1, int32_t n, void* workspace, size_t workspace_bytes, t2p_stream_t stream) {
    return launch_linear_wgrad_f32(dy, lda, x, ldb, dw, ldc, colsum, m, k1, n, workspace, workspace_bytes, (hipStream_t)stream);
}

int t2p_rownorm(const float* x, int64_t n_rows, int32_t dim, float* out, t2p_stream_t stream) {
    return launch_rownorm(x, dim, n_rows, dim, out, dim, 0, (hipStream_t)stream);
}

}  // extern "C"
