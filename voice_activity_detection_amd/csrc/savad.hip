// savad.hip -- host side of libsavad.so: the C ABI declared in include/savad.h.
// Owns the packed weights and the positional-encoding cache, and launches what savad_schedule.h plans for a forward: one of four
// kernel families (generic, fp32, bf16, fp32s), each as a single launch for the whole forward (T <= 32), or as
//   input_qkv -> [attention(l) -> row(l)] x L      (row(L-1) ends in classifier + log-softmax)
// with attention and row chain of a layer in one launch (fused) or in two.
// the order of the kernel headers is the order of the kernels in the code object
#include "savad_kernels.h"
#include "savad_aux_kernels.h"
#include "savad_batch_kernels.h"
#include "savad_kernels_bf16.h"
#include "savad_attn_pw_bf16.h"
#include "savad_packed_bf16.h"
#include "savad_kernels_f32s.h"
#include "savad_generic.h"
#include <type_traits>
#include "savad_logmel.h"
#include "savad_frontend.h"
#include "savad_ingest.h"
#include "savad_post.h"
#include "savad_post_device.h"
#include "savad_post_batch.h"
#include "savad_eval_device.h"
#include "savad_eval_batch.h"
#include "savad_schedule.h"
#include "savad_weights.h"
#include "savad_live.h"
#include "savad_live_post.h"
#include "savad_logmel_batch.h"

#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <functional>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <utility>
#include <variant>
#include <vector>

#include "../../include/savad.h"

#define SAVAD_EXPORT extern "C" __attribute__((visibility("default")))

namespace {

thread_local char g_err[512] = "";

int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(SAVAD_E_HIP, "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                                          __FILE__, __LINE__);                                        \
    } while (0)

constexpr int MAX_EVENTS = 64;

}  // namespace

// a fragment image: the weights in the operand order of one kernel family's MFMAs (bf16, or the three bf16 pieces of fp32s)
struct FragImage {
    const savad::weights::FragLayout* at = nullptr;  // byte offsets into d (the handle's w.bf16 / w.f32s)
    char* d = nullptr;
    bool dirty = true;           // the raw parameters changed since it was packed
    bool lds_attrs_set = false;  // hipFuncSetAttribute(MaxDynamicSharedMemorySize) done for the family's kernels
};

struct savad_model {
    savad_config cfg;
    savad::weights::Layout w;    // where every weight lies (savad_weights.h); w.generic: d_model != 128, the plain fp32 kernels of savad_generic.h
    std::vector<char> param_set;  // per w.params entry
    float* d_raw = nullptr;      // parameters exactly as handed over (state_dict layout)
    float* d_packed = nullptr;   // LayerNorm-folded weights
    bool dirty = true;
    FragImage bf16;  // savad_kernels_bf16.h, filled when precision == 1
    FragImage f32s;  // savad_kernels_f32s.h, filled when precision == 2
    // positional-encoding cache (mirrors SinusoidalPositionalEncoding: rebuilt when T grows,
    // vad/modeling/transformer.py:392-397; initial length 10: vad/models/self_attention.py:14)
    float* d_pe = nullptr;
    int pe_len = 0;
    std::vector<float> h_pe;
    int splits = 0;
    int row_mode = 0;  // savad_set_row_mode: 0 automatic, 1 - 8 pin a form or variant of the precision's kernel family (include/savad.h; savad_schedule.h)
    bool batch_invariant = false;   // bf16: the persistent attention kernel without key-split tail items (savad_set_batch_invariant)
    int precision = 0;  // 0 = fp32 MFMA, 1 = bf16 MFMA operands (fp32 accumulate / statistics / residual stream),
                        // 2 = "fp32s": fp32 parity on the bf16 pipe, every operand as three bf16 pieces (savad_kernels_f32s.h)
    unsigned* d_sat = nullptr;  // bf16 path: elements of the fp16-stored residual stream that saturated since the last query
    int n_cu = 256;             // compute units of the handle's device (launch-shape decisions)
    // profiling
    int prof_capacity = 0, prof_used = 0, prof_nk = 0, prof_skip = 0;
    std::vector<hipEvent_t> events;  // prof_capacity * MAX_EVENTS
    std::vector<const char*> knames;

    void weights_changed() { dirty = bf16.dirty = f32s.dirty = true; }
};

namespace {

using namespace savad;

// blocks of 256 threads for `work` elements, at most `cap` (the kernels stride over the rest)
int grid_for(long work, int cap = 4096) { return (int)((work + 255) / 256 < cap ? (work + 255) / 256 : cap); }

sched::Knobs knobs_of(const savad_model* m) {
    sched::Knobs k;
    k.precision = m->precision;
    k.row_mode = m->row_mode;
    k.splits = m->splits;
    k.batch_invariant = m->batch_invariant;
    k.n_cu = m->n_cu;
    k.num_layers = m->cfg.num_layers;
    k.feature_size = m->cfg.feature_size;
    k.FP = m->w.FP;
    k.generic = m->w.generic;
    k.d_model = m->cfg.d_model;
    return k;
}

float qscale() { return (float)(1.4426950408889634 / sqrt((double)D)); }  // log2(e) / sqrt(d_head): the softmax runs on exp2

// a3: vad/modeling/transformer.py:403-414 (fp32 semantics), pre-divided by sqrt(D) (:389,401)
void build_pe(std::vector<float>& pe, int T) {
    pe.resize((size_t)T * D);
    const float cexp = (float)(-(log(10000.0) / (double)D));
    const float scale = (float)sqrt((double)D);
    for (int i = 0; i < D / 2; ++i) {
        const float arg = (float)(2 * i) * cexp;
        const float wv = (float)exp((double)arg);
        for (int t = 0; t < T; ++t) {
            const float a = (float)t * wv;
            pe[(size_t)t * D + 2 * i] = (float)sin((double)a) / scale;
            pe[(size_t)t * D + 2 * i + 1] = (float)cos((double)a) / scale;
        }
    }
}

int ensure_pe(savad_model* m, int T, hipStream_t st) {
    if (T <= m->pe_len) return SAVAD_OK;
    int cap = m->pe_len > 0 ? m->pe_len : 10;
    while (cap < T) cap *= 2;
    if (m->d_pe) {
        HIP_TRY(hipStreamSynchronize(st));  // kernels of earlier forwards may still read the old table
        HIP_TRY(hipFree(m->d_pe));
        m->d_pe = nullptr;
        m->pe_len = 0;
    }
    const size_t Dm = m->cfg.d_model;
    HIP_TRY(hipMalloc(&m->d_pe, sizeof(float) * (size_t)cap * Dm));
    if (m->w.generic) {
        m->h_pe.resize((size_t)cap * Dm);
        gen::build_pe_host(m->h_pe.data(), cap, (int)Dm);
    } else {
        build_pe(m->h_pe, cap);
    }
    HIP_TRY(hipMemcpyAsync(m->d_pe, m->h_pe.data(), sizeof(float) * (size_t)cap * Dm, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));  // h_pe is pageable and reused
    m->pe_len = cap;
    return SAVAD_OK;
}

int fold(savad_model* m, hipStream_t st, size_t w, size_t b, size_t g, size_t be, size_t wout, size_t bout, int N,
         int K) {
    hipLaunchKernelGGL(fold_ln_kernel, dim3(N), dim3(128), 0, st, m->d_raw + w, m->d_raw + b, m->d_raw + g,
                       m->d_raw + be, m->d_packed + wout, m->d_packed + bout, K);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

int prepare_weights(savad_model* m, hipStream_t st) {
    if (!m->dirty) return SAVAD_OK;
    const weights::Layout& w = m->w;
    for (size_t i = 0; i < w.params.size(); ++i)
        if (!m->param_set[i]) return fail(SAVAD_E_STATE, "parameter '%s' was never set", w.params[i].key.c_str());
    const int L = m->cfg.num_layers;
    for (int l = 0; l < L; ++l) {
        const auto& r = w.lr[l];
        const auto& p = w.lp[l];
        int rc;
        if ((rc = fold(m, st, r.wq, r.bq, r.ln1w, r.ln1b, p.wqkv, p.bqkv, D, D))) return rc;
        if ((rc = fold(m, st, r.wk, r.bk, r.ln1w, r.ln1b, p.wqkv + (size_t)D * D, p.bqkv + D, D, D))) return rc;
        if ((rc = fold(m, st, r.wv, r.bv, r.ln1w, r.ln1b, p.wqkv + (size_t)2 * D * D, p.bqkv + 2 * D, D, D))) return rc;
        if ((rc = fold(m, st, r.w1, r.b1, r.ln2w, r.ln2b, p.w1, p.b1, DFF, D))) return rc;
        float* frag = m->d_packed + p.frag;
        hipLaunchKernelGGL(pack_frag32_kernel, dim3(192), dim3(256), 0, st, m->d_packed + p.wqkv, 0, 12, frag);
        hipLaunchKernelGGL(pack_frag32_kernel, dim3(64), dim3(256), 0, st, m->d_raw + r.wo, 0, 4, frag + 12 * FRAG_BLOCK);
        hipLaunchKernelGGL(pack_frag32_kernel, dim3(256), dim3(256), 0, st, m->d_packed + p.w1, 0, 16, frag + 16 * FRAG_BLOCK);
        hipLaunchKernelGGL(pack_frag32_kernel, dim3(256), dim3(256), 0, st, m->d_raw + r.w2, 1, 16, frag + 32 * FRAG_BLOCK);
        HIP_TRY(hipGetLastError());
        float* lb = m->d_packed + w.p_bias + (size_t)l * LBIAS;
        const size_t f = sizeof(float);
        HIP_TRY(hipMemcpyAsync(lb, m->d_packed + p.b1, DFF * f, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(lb + DFF, m->d_raw + r.b2, D * f, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(lb + DFF + D, m->d_packed + p.bqkv, 3 * D * f, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipMemcpyAsync(lb + DFF + 4 * D, m->d_raw + r.bo, D * f, hipMemcpyDeviceToDevice, st));
    }
    int rc = fold(m, st, w.r_wc, w.r_bc, w.r_lnf_w, w.r_lnf_b, w.p_wc, w.p_bc, 2, D);
    if (rc) return rc;
    if (w.FP != m->cfg.feature_size) {
        hipLaunchKernelGGL(pad_rows_kernel<float>, dim3(64), dim3(256), 0, st, m->d_raw + w.r_win, (size_t)D,
                           m->cfg.feature_size, w.FP, m->d_packed + w.p_win_pad);
        HIP_TRY(hipGetLastError());
    }
    m->dirty = false;
    return SAVAD_OK;
}

// input weight as the kernels read it: [D][FP], the raw tensor itself when no padding is needed
const float* win_fp32(const savad_model* m) {
    return m->w.FP == m->cfg.feature_size ? m->d_raw + m->w.r_win : m->d_packed + m->w.p_win_pad;
}

using PackKernel = void (*)(const float*, int, int, __bf16*);  // bf::pack_weight_frags_kernel, fs::pack_weight_frags3_kernel

int pack_frags(FragImage& im, PackKernel pack, hipStream_t st, const float* W, int N, int K, size_t off) {
    hipLaunchKernelGGL(pack, dim3(grid_for((long)N * K, 1024)), dim3(256), 0, st, W, N, K, reinterpret_cast<__bf16*>(im.d + off));
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// the folded fp32 weights (prepare_weights) into the image `im`, in the operand format `pack` writes
int prepare_frags(savad_model* m, FragImage& im, PackKernel pack, hipStream_t st) {
    if (!im.dirty) return SAVAD_OK;
    const int L = m->cfg.num_layers;
    const float *R = m->d_raw, *P = m->d_packed;
    int rc;
    if ((rc = pack_frags(im, pack, st, win_fp32(m), D, m->w.FP, im.at->win))) return rc;
    for (int l = 0; l < L; ++l) {
        const auto& r = m->w.lr[l];
        const auto& p = m->w.lp[l];
        const auto& f = im.at->layer[l];
        if ((rc = pack_frags(im, pack, st, P + p.wqkv, 3 * D, D, f.wqkv))) return rc;
        if ((rc = pack_frags(im, pack, st, R + r.wo, D, D, f.wo))) return rc;
        if ((rc = pack_frags(im, pack, st, P + p.w1, DFF, D, f.w1))) return rc;
        if ((rc = pack_frags(im, pack, st, R + r.w2, D, DFF, f.w2))) return rc;
        if (!im.at->folded) continue;
        // the fused fp32s launches of T > 32 never issue the out-projection: one head, softmax rows sum to 1, so
        //   Wo (P (x Wv'^T + bv')) + bo = P (x (Wo Wv')^T + Wo bv') + bo
        // nor the key projection: the part of a score that depends on the key is [c Wk'^T (Wq' x_i + bq')] . x_j, so the query is
        // projected with Wq~ = c Wk'^T Wq' (bias c Wk'^T bq') and the key is the normalised row itself.  A SECOND image per layer holds
        // Wq~ | Wvo (bias image: bq~ | Wo bv'); products in fp64, rounded once.  The plain images stay: the T <= 32 kernels read them.
        const float* wqkv = P + p.wqkv;
        hipLaunchKernelGGL(fs::fold_qk_kernel, dim3(D), dim3(D), 0, st, wqkv, wqkv + (size_t)D * D, P + p.bqkv,
                           1.4426950408889634 / sqrt((double)D), m->d_packed + p.wq_vo, m->d_packed + p.bq_vo);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(fs::fold_vo_kernel, dim3(D), dim3(D), 0, st, R + r.wo, wqkv + (size_t)2 * D * D, P + p.bqkv,
                           m->d_packed + p.wq_vo + (size_t)D * D, m->d_packed + p.bq_vo + D);
        HIP_TRY(hipGetLastError());
        if ((rc = pack_frags(im, pack, st, P + p.wq_vo, 2 * D, D, f.wq_vo))) return rc;
    }
    im.dirty = false;
    return SAVAD_OK;
}

template <typename KernelT>
int allow_lds(KernelT kernel, int bytes) {
    HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    return SAVAD_OK;
}

struct Prof {
    savad_model* m;
    hipStream_t st;
    hipEvent_t* ev;
    int n;
    Prof(savad_model* mm, hipStream_t s) : m(mm), st(s), ev(nullptr), n(0) {
        if (m->prof_capacity > 0 && m->prof_skip > 0) {
            --m->prof_skip;  // settle-in forwards after savad_set_profiling: launched as usual, not recorded
        } else if (m->prof_capacity > 0 && m->prof_used < m->prof_capacity) {
            ev = m->events.data() + (size_t)m->prof_used * MAX_EVENTS;
            m->knames.clear();
            hipEventRecord(ev[0], st);
        }
    }
    void mark(const char* name) {
        if (!ev || n + 1 >= MAX_EVENTS) return;
        ++n;
        hipEventRecord(ev[n], st);
        m->knames.push_back(name);
    }
    void done() {
        if (!ev) return;
        m->prof_nk = n;
        m->prof_used++;
    }
};


void launch_gemm(hipStream_t st, const gen::GemmArgs& g, int batch) {
    hipLaunchKernelGGL(gen::gemm_kernel, dim3((g.N + gen::GT - 1) / gen::GT, (g.M + gen::GT - 1) / gen::GT, batch), dim3(256), 0, st, g);
}

// nn.Linear on `rows` rows: y = act(x W^T + b [+ pe]) [+ res]
void launch_linear(hipStream_t st, const float* x, long rows, int K, const float* W, const float* b, int N, float* y, const float* res,
                   bool relu, const float* pe, int T) {
    // rows per launch: a multiple of T (the positional-encoding row of output row m is m % T) that keeps grid.y inside its limit
    const long step = T >= (1L << 21) ? T : (1L << 21) / T * T;
    for (long r0 = 0; r0 < rows; r0 += step) {
        gen::GemmArgs g{};
        g.M = (int)(rows - r0 < step ? rows - r0 : step);
        g.N = N;
        g.K = K;
        g.A = x + r0 * K;
        g.lda = K;
        g.Bm = W;
        g.ldk = 1;
        g.ldn = K;
        g.C = y + r0 * N;
        g.ldc = N;
        g.alpha = 1.0f;
        g.bias = b;
        g.add = pe;
        g.add_rows = pe ? T : 1;
        g.res = res ? res + r0 * N : nullptr;
        g.relu = relu ? 1 : 0;
        launch_gemm(st, g, 1);
    }
}

// SelfAttentiveVAD.forward for any d_model, the reference's operation sequence (vad/models/self_attention.py:23-28) kernel by kernel
void forward_generic(savad_model* m, const sched::ForwardPlan& p, const float* x, int B, int T, float* out, void* workspace, hipStream_t st, Prof& prof) {
    const int Dm = m->cfg.d_model, F = m->cfg.feature_size, L = m->cfg.num_layers;
    char* W = (char*)workspace;
    auto at = [W](size_t off) { return (float*)(W + off); };
    float *h = at(p.h), *n = at(p.n), *q = at(p.q), *k = at(p.k), *v = at(p.v), *ctx = at(p.ctx), *ff = at(p.ff), *sc = at(p.scores);
    const float* R = m->d_raw;
    const weights::Layout& w = m->w;
    const long rows = (long)B * T;
    const int ln_grid = (int)((rows + 3) / 4);
    // input Linear + positional encoding / sqrt(d_model) (self_attention.py:13-15, transformer.py:401); dropout = identity
    launch_linear(st, x, rows, F, R + w.r_win, R + w.r_bin, Dm, h, nullptr, false, m->d_pe, T);
    prof.mark("input_generic");
    const float alpha = (float)(1.0 / sqrt((double)Dm));  // / sqrt(d_head), one head (transformer.py:362)
    for (int l = 0; l < L; ++l) {
        const auto& r = w.lr[l];
        hipLaunchKernelGGL(gen::layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, h, R + r.ln1w, R + r.ln1b, n, rows, Dm);
        launch_linear(st, n, rows, Dm, R + r.wq, R + r.bq, Dm, q, nullptr, false, nullptr, T);
        launch_linear(st, n, rows, Dm, R + r.wk, R + r.bk, Dm, k, nullptr, false, nullptr, T);
        launch_linear(st, n, rows, Dm, R + r.wv, R + r.bv, Dm, v, nullptr, false, nullptr, T);
        prof.mark("qkv_generic");
        for (int b0 = 0; b0 < B; b0 += p.cb) {
            const int nb = B - b0 < p.cb ? B - b0 : p.cb;
            for (int t0 = 0; t0 < T; t0 += p.tq) {
                const int nq = T - t0 < p.tq ? T - t0 : p.tq;
                gen::GemmArgs g{};
                g.A = q + ((size_t)b0 * T + t0) * Dm;  // scores = q k^T / sqrt(d) (transformer.py:351-363)
                g.lda = Dm;
                g.sA = (long)T * Dm;
                g.Bm = k + (size_t)b0 * T * Dm;
                g.ldk = 1;
                g.ldn = Dm;
                g.sB = (long)T * Dm;
                g.C = sc;
                g.ldc = T;
                g.sC = (long)nq * T;
                g.M = nq;
                g.N = T;
                g.K = Dm;
                g.alpha = alpha;
                g.add_rows = 1;
                launch_gemm(st, g, nb);
                const long srows = (long)nb * nq;
                hipLaunchKernelGGL(gen::softmax_kernel, dim3((unsigned)((srows + 3) / 4)), dim3(256), 0, st, sc, srows, T);
                gen::GemmArgs c{};
                c.A = sc;  // context = A V (transformer.py:338-346)
                c.lda = T;
                c.sA = (long)nq * T;
                c.Bm = v + (size_t)b0 * T * Dm;
                c.ldk = Dm;
                c.ldn = 1;
                c.sB = (long)T * Dm;
                c.C = ctx + ((size_t)b0 * T + t0) * Dm;
                c.ldc = Dm;
                c.sC = (long)T * Dm;
                c.M = nq;
                c.N = Dm;
                c.K = T;
                c.alpha = 1.0f;
                c.add_rows = 1;
                launch_gemm(st, c, nb);
            }
        }
        prof.mark("attention_generic");
        // final_projection + residual onto the un-normalised x (transformer.py:347,237); FFN sublayer (:366-382)
        launch_linear(st, ctx, rows, Dm, R + r.wo, R + r.bo, Dm, h, h, false, nullptr, T);
        hipLaunchKernelGGL(gen::layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, h, R + r.ln2w, R + r.ln2b, n, rows, Dm);
        launch_linear(st, n, rows, Dm, R + r.w1, R + r.b1, 4 * Dm, ff, nullptr, true, nullptr, T);
        launch_linear(st, ff, rows, 4 * Dm, R + r.w2, R + r.b2, Dm, h, h, false, nullptr, T);
        prof.mark("row_generic");
    }
    hipLaunchKernelGGL(gen::layernorm_kernel, dim3(ln_grid), dim3(256), 0, st, h, R + w.r_lnf_w, R + w.r_lnf_b, n, rows, Dm);
    hipLaunchKernelGGL(gen::classifier_kernel, dim3(ln_grid), dim3(256), 0, st, n, R + w.r_wc, R + w.r_bc, out, rows, Dm);
    prof.mark("classifier_generic");
}

}  // namespace

SAVAD_EXPORT const char* savad_last_error(void) { return g_err; }
SAVAD_EXPORT const char* savad_version(void) { return "savad 0.1 (gfx950, fp32 MFMA)"; }

SAVAD_EXPORT void savad_destroy(savad_handle m) {
    if (!m) return;
    for (hipEvent_t e : m->events) hipEventDestroy(e);
    for (void* d : {(void*)m->d_raw, (void*)m->d_packed, (void*)m->bf16.d, (void*)m->f32s.d, (void*)m->d_sat, (void*)m->d_pe})
        if (d) hipFree(d);
    delete m;
}

SAVAD_EXPORT int savad_create(const savad_config* cfg, savad_handle* out) {
    if (!cfg || !out) return fail(SAVAD_E_INVALID, "null argument");
    if (cfg->d_model < 2 || cfg->d_model > 4096 || cfg->d_model % 2)  // the reference's positional encoding pairs sin / cos columns
        return fail(SAVAD_E_INVALID, "d_model=%d (an even value in [2, 4096])", cfg->d_model);
    if (cfg->feature_size <= 0 || cfg->feature_size > 4096)
        return fail(SAVAD_E_INVALID, "feature_size=%d", cfg->feature_size);
    if (cfg->num_layers < 1 || cfg->num_layers > 64) return fail(SAVAD_E_INVALID, "num_layers=%d", cfg->num_layers);
    savad_model* m = new savad_model();
    m->cfg = *cfg;
    {
        int dev = 0, n = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) m->n_cu = n;
    }
    m->w = weights::make_layout(cfg->feature_size, cfg->num_layers, cfg->d_model);
    const weights::Layout& w = m->w;
    m->param_set.assign(w.params.size(), 0);
    m->bf16.at = &w.bf16;
    m->f32s.at = &w.f32s;
    // every buffer of the handle now: a forward allocates nothing (d_model != 128: the raw parameters are all there is)
    hipError_t e = hipMalloc(&m->d_raw, sizeof(float) * w.raw_floats);
    if (!w.generic) {
        if (e == hipSuccess) e = hipMalloc(&m->bf16.d, w.bf16.bytes);
        if (e == hipSuccess) e = hipMalloc(&m->f32s.d, w.f32s.bytes);
        if (e == hipSuccess) e = hipMalloc(&m->d_sat, sizeof(unsigned));
        if (e == hipSuccess) e = hipMemset(m->d_sat, 0, sizeof(unsigned));
        if (e == hipSuccess) e = hipMalloc(&m->d_packed, sizeof(float) * w.packed_floats);
    }
    if (e != hipSuccess) {
        savad_destroy(m);
        return fail(SAVAD_E_HIP, "hipMalloc(weights): %s", hipGetErrorString(e));
    }
    *out = m;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_num_params(savad_handle m) { return m ? (int)m->w.params.size() : 0; }
SAVAD_EXPORT const char* savad_param_key(savad_handle m, int i) {
    return (m && i >= 0 && i < (int)m->w.params.size()) ? m->w.params[i].key.c_str() : nullptr;
}
SAVAD_EXPORT size_t savad_param_numel(savad_handle m, int i) {
    return (m && i >= 0 && i < (int)m->w.params.size()) ? m->w.params[i].numel : 0;
}

SAVAD_EXPORT int savad_set_param(savad_handle m, const char* key, const float* data, size_t numel, void* stream) {
    if (!m || !key || !data) return fail(SAVAD_E_INVALID, "null argument");
    for (size_t i = 0; i < m->w.params.size(); ++i) {
        const weights::Param& p = m->w.params[i];
        if (p.key != key) continue;
        if (p.numel != numel)
            return fail(SAVAD_E_INVALID, "size mismatch for '%s': got %zu elements, expected %zu", key, numel, p.numel);
        HIP_TRY(hipMemcpyAsync(m->d_raw + p.off, data, sizeof(float) * numel, hipMemcpyDefault, (hipStream_t)stream));
        m->param_set[i] = 1;
        m->weights_changed();
        return SAVAD_OK;
    }
    return fail(SAVAD_E_NOKEY, "unexpected key '%s' in state_dict", key);
}

SAVAD_EXPORT int savad_set_attention_splits(savad_handle m, int splits) {
    if (!m || splits < 0 || splits > 64) return fail(SAVAD_E_INVALID, "splits=%d", splits);
    m->splits = splits;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_set_row_mode(savad_handle m, int mode) {
    if (!m || mode < 0 || mode > 8) return fail(SAVAD_E_INVALID, "row mode %d", mode);
    m->row_mode = mode;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_set_batch_invariant(savad_handle m, int on) {
    if (!m || on < 0 || on > 1) return fail(SAVAD_E_INVALID, "batch_invariant %d (0 or 1)", on);
    m->batch_invariant = on != 0;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_workspace_bytes(savad_handle m, int B, int T, size_t* bytes) {
    if (!m || !bytes || B < 0 || T < 0) return fail(SAVAD_E_INVALID, "bad argument");
    if ((double)B * T * D >= 2.0e9) return fail(SAVAD_E_UNSUPPORTED, "B*T=%ld rows exceed the 32-bit tile index range", (long)B * T);
    *bytes = sched::plan_forward(knobs_of(m), B, T, false, 0).total;
    return SAVAD_OK;
}

// Sizes everything savad_forward may otherwise have to (re)allocate for sequences of up to T_max frames -- today the
// positional-encoding table -- so that later forwards with T <= T_max neither allocate nor synchronise.
// Once every parameter has been set it also folds / packs the weights for the selected precision (and raises the bf16
// kernels' LDS limits), so that even the FIRST forward after it launches nothing but its own kernels and can be captured
// into a HIP graph.  With parameters still missing only the table is sized (the forward reports the missing key).
namespace {
int ensure_ready(savad_model* m, int family, int T, hipStream_t st);
}
SAVAD_EXPORT int savad_reserve(savad_handle m, int T_max, void* stream) {
    if (!m || T_max < 0) return fail(SAVAD_E_INVALID, "bad argument");
    if ((double)T_max * D >= 2.0e9) return fail(SAVAD_E_UNSUPPORTED, "T_max=%d too large", T_max);
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = ensure_pe(m, T_max, st))) return rc;
    if (m->w.generic) return SAVAD_OK;  // nothing to fold or pack: the generic kernels read the raw parameters
    for (char set : m->param_set)
        if (!set) return SAVAD_OK;
    return ensure_ready(m, m->precision == 1 ? sched::BF16 : m->precision == 2 ? sched::F32S : sched::F32, T_max, st);
}

// bf16 precision stores the residual stream between kernels as fp16 (+-65504); every element that had to be clamped is
// counted.  Reads the count accumulated since the last call and clears it; synchronises `stream`.
SAVAD_EXPORT int savad_residual_saturations(savad_handle m, unsigned long long* count, void* stream) {
    if (!m || !count) return fail(SAVAD_E_INVALID, "null argument");
    if (!m->d_sat) {  // fp32-only handle (d_model != 128): no fp16-stored residual stream, nothing can saturate
        *count = 0;
        return SAVAD_OK;
    }
    unsigned c = 0;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(&c, m->d_sat, sizeof(c), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemsetAsync(m->d_sat, 0, sizeof(unsigned), st));
    HIP_TRY(hipStreamSynchronize(st));
    *count = c;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_set_precision(savad_handle m, int precision) {
    if (!m || precision < 0 || precision > 2) return fail(SAVAD_E_INVALID, "precision %d (0 = fp32, 1 = bf16, 2 = fp32s)", precision);
    if (m->w.generic && precision != 0)
        return fail(SAVAD_E_UNSUPPORTED, "bf16 / split-bf16 operands are implemented for d_model=128 only (this handle: d_model=%d, fp32)", m->cfg.d_model);
    m->precision = precision;
    return SAVAD_OK;
}

namespace {

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) for every bf16 kernel, once per handle
int prepare_bf16_launch(savad_model* m) {
    int rc;
    if (m->bf16.lds_attrs_set) return SAVAD_OK;
    constexpr int r4 = bf::Ring<4>::NRING * bf::RING_BYTES, r8 = bf::Ring<8>::NRING * bf::RING_BYTES;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16<float, 4>, r4 + 3 * D * 4))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16<__bf16, 4>, r4 + 3 * D * 4))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16_p<float, 8, 5>, bf::input_p_lds_bytes(5)))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16_p<__bf16, 8, 5>, bf::input_p_lds_bytes(5)))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16_p<float, 8, 0>, bf::input_p_lds_bytes(15)))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16_p<__bf16, 8, 0>, bf::input_p_lds_bytes(15)))) return rc;
    if ((rc = allow_lds(bf::attention_kernel_bf16<4>, r4))) return rc;
    if ((rc = allow_lds(bf::row_kernel_bf16<false, 4>, r4 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::row_kernel_bf16<true, 4>, r4 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::attention_row_kernel_bf16<false, 4>, r4 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::attention_row_kernel_bf16<true, 4>, r4 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16<float, 8>, r8 + 3 * D * 4))) return rc;
    if ((rc = allow_lds(bf::input_qkv_kernel_bf16<__bf16, 8>, r8 + 3 * D * 4))) return rc;
    if ((rc = allow_lds(bf::attention_kernel_bf16<8>, r8))) return rc;
    if ((rc = allow_lds(bf::row_kernel_bf16<false, 8>, r8 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::row_kernel_bf16<true, 8>, r8 + 9 * D * 4))) return rc;
    if ((rc = allow_lds(bf::attention_pw_kernel_bf16, bf::PW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(bf::attention_pw_kernel_bf16_nosplit, bf::PW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(bf::packed_forward_kernel_bf16<4, 2, 0>, r4 + (bf::PACKED_BF16_MAX_LAYERS * LBIAS + 2 * D + 4) * 4))) return rc;
    if ((rc = allow_lds(bf::packed_forward_kernel_bf16<4, 4, 4>, r8 + (bf::PACKED_BF16_MAX_LAYERS * LBIAS + 2 * D + 4) * 4))) return rc;
    if ((rc = allow_lds(bf::packed_forward_kernel_bf16<8, 4, 0>, r8 + (bf::PACKED_BF16_MAX_LAYERS * LBIAS + 2 * D + 4) * 4))) return rc;
    if ((rc = allow_lds(bf::packed_forward_kernel_bf16_ns, bf::ns_lds_bytes(bf::PACKED_BF16_MAX_LAYERS)))) return rc;
    m->bf16.lds_attrs_set = true;
    return SAVAD_OK;
}

int prepare_f32s_launch(savad_model* m);  // (beside forward_f32s)

// Everything a forward of `family` reads besides its input: folded weights, the family's fragment image and LDS limits, and a
// positional-encoding table of at least T rows.  Nothing is launched or allocated once it has run for the handle's current parameters.
int ensure_ready(savad_model* m, int family, int T, hipStream_t st) {
    int rc;
    if (family == sched::GENERIC) {  // nothing to fold or pack: the generic kernels read the raw parameters
        for (size_t i = 0; i < m->w.params.size(); ++i)
            if (!m->param_set[i]) return fail(SAVAD_E_NOKEY, "missing key '%s' in state_dict", m->w.params[i].key.c_str());
        return ensure_pe(m, T, st);
    }
    if ((rc = prepare_weights(m, st))) return rc;
    if (family == sched::BF16 && (rc = prepare_frags(m, m->bf16, bf::pack_weight_frags_kernel, st))) return rc;
    if (family == sched::F32S && (rc = prepare_frags(m, m->f32s, fs::pack_weight_frags3_kernel, st))) return rc;
    if ((rc = ensure_pe(m, T, st))) return rc;
    if (family == sched::BF16) return prepare_bf16_launch(m);
    if (family == sched::F32S) return prepare_f32s_launch(m);
    return SAVAD_OK;
}

// zero-pad the features to the kernels' K granularity (fp32 copy)
template <typename XT>
void pad_features(hipStream_t st, const XT* x, size_t rows, int F, int FP, float* xp) {
    hipLaunchKernelGGL(pad_rows_kernel<XT>, dim3(grid_for((long)(rows * FP))), dim3(256), 0, st, x, rows, F, FP, xp);
}

// what a forward's kernels read as their input: the caller's features, or their zero-padded fp32 copy in the workspace (plan.pad)
struct Features {
    const void* x;
    int is_bf16;
    int F;     // columns of x
    long xbs;  // elements between consecutive sequences
};

Features forward_input(savad_model* m, const sched::ForwardPlan& p, const void* x, int x_is_bf16, int B, int T, long xbs_in, char* W, hipStream_t st) {
    Features in{x, x_is_bf16, m->cfg.feature_size, 0};
    if (p.pad) {
        float* xp = (float*)(W + p.xpad);
        if (x_is_bf16)
            pad_features(st, (const __bf16*)x, (size_t)B * T, in.F, m->w.FP, xp);
        else
            pad_features(st, (const float*)x, (size_t)B * T, in.F, m->w.FP, xp);
        in = Features{xp, 0, m->w.FP, 0};
    }
    in.xbs = xbs_in > 0 ? xbs_in : (long)T * in.F;
    return in;
}

// the single-launch kernels' view of the weights: every layer's matrices in the image `im`, biases and classifier in fp32
// (the slots past L are never read: they repeat layer 0)
template <typename Model>
Model packed_model(const savad_model* m, const FragImage& im) {
    constexpr int MAX_LAYERS = (int)std::extent<decltype(Model::layer)>::value;
    const weights::Layout& w = m->w;
    const int L = m->cfg.num_layers;
    Model pm;
    for (int l = 0; l < MAX_LAYERS; ++l) {
        const auto& f = im.at->layer[l < L ? l : 0];
        pm.layer[l] = {im.d + f.wqkv, im.d + f.wo, im.d + f.w1, im.d + f.w2};
    }
    pm.win = im.d + im.at->win;
    pm.bin = m->d_raw + w.r_bin;
    pm.pe = m->d_pe;
    pm.bias = m->d_packed + w.p_bias;
    pm.wc = m->d_packed + w.p_wc;
    pm.bc = m->d_packed + w.p_bc;
    pm.L = L;
    return pm;
}

// T <= 32: the whole forward in one launch, a packed block of 32 / T sequences per wave or workgroup, in the variant the plan names
// (sched::single_bf16_variant, single_f32s_variant; fp32 has one).  wo.w == T: x is the predictor's feature matrix and sequence s its
// window at win_base + s.  The handle must be ready (ensure_ready).  Returns the launch's name for the profile.
const char* launch_single(savad_model* m, int family, int variant, hipStream_t st, const float* x, int B, int T, int F, float* out,
                          const WindowOffsets& wo, int win_base) {
    const int L = m->cfg.num_layers;
    const int G = 32 / T, nblk = (B + G - 1) / G;
    const float c = qscale();
    if (family == sched::BF16) {  // savad_packed_bf16.h
        const auto pm = packed_model<bf::PackedBf16Model>(m, m->bf16);
        const size_t bias_bytes = ((size_t)L * LBIAS + 2 * D + 4) * 4;   // every layer's biases + the classifier
        const size_t ring2 = (size_t)2 * bf::RING_BYTES, ring4 = (size_t)4 * bf::RING_BYTES;
        if (variant == 8)
            hipLaunchKernelGGL(bf::packed_forward_kernel_bf16_ns, dim3(nblk), dim3(256), bf::ns_lds_bytes(L), st, x, B, T, F, nblk, pm, c, out, wo, win_base,
                               m->d_sat);
        else if (variant == 5)
            hipLaunchKernelGGL((bf::packed_forward_kernel_bf16<8, 4, 0>), dim3((nblk + 7) / 8), dim3(512), ring4 + bias_bytes, st, x, B, T, F, nblk, pm, c, out,
                               wo, win_base, m->d_sat);
        else if (variant == 6)
            hipLaunchKernelGGL((bf::packed_forward_kernel_bf16<4, 4, 4>), dim3((nblk + 3) / 4), dim3(512), ring4 + bias_bytes, st, x, B, T, F, nblk, pm, c, out,
                               wo, win_base, m->d_sat);
        else
            hipLaunchKernelGGL((bf::packed_forward_kernel_bf16<4, 2, 0>), dim3((nblk + 3) / 4), dim3(256), ring2 + bias_bytes, st, x, B, T, F, nblk, pm, c, out,
                               wo, win_base, m->d_sat);
        return "packed_forward_bf16";
    }
    if (family == sched::F32S) {
        const auto pm = packed_model<fs::PackedF32sModel>(m, m->f32s);
        if (variant == sched::VARIANT_LATENCY)
            hipLaunchKernelGGL(fs::packed_forward_kernel_f32s_ns, dim3(nblk), dim3(256), fs::nsf_lds_bytes(L), st, x, B, T, F, nblk, pm, c, out, wo, win_base);
        else
            hipLaunchKernelGGL(fs::packed_forward_kernel_f32s, dim3((nblk + 3) / 4), dim3(256), fs::packed_f32s_lds_bytes(L), st, x, B, T, F, nblk, pm, c,
                               out, wo, win_base);
        return "packed_forward_f32s";
    }
    const weights::Layout& w = m->w;
    const float *R = m->d_raw, *P = m->d_packed;
    PackedModel pm;
    for (int l = 0; l < L; ++l) pm.layer[l] = PackedLayer{P + w.lp[l].frag};
    for (int l = L; l < PACKED_MAX_LAYERS; ++l) pm.layer[l] = pm.layer[0];
    pm.bias = P + w.p_bias;
    pm.win = win_fp32(m);
    pm.bin = R + w.r_bin;
    pm.pe = m->d_pe;
    pm.wc = P + w.p_wc;
    pm.bc = P + w.p_bc;
    pm.L = L;
    hipLaunchKernelGGL(packed_forward_kernel, dim3(nblk), dim3(256), 0, st, x, B * T, T, F, pm, c, out, G * T, wo, win_base);
    return "packed_forward";
}

// layer l's Q / K / V projection as a stage reads it from the image and the packed buffer; folded: the image Wq~ | Wo Wv' (four slots,
// the keys are the normalised rows) and its biases bq~ | Wo bv'
const char* qkv_frags(const FragImage& im, int l, bool folded) { return im.d + (folded ? im.at->layer[l].wq_vo : im.at->layer[l].wqkv); }
const float* qkv_bias(const savad_model* m, int l, bool folded) { return m->d_packed + (folded ? m->w.lp[l].bq_vo : m->w.lp[l].bqkv); }

// the row chain of layer l on the image `im`: its own matrices, then the next layer's Q / K / V projection into `nxt`, or the
// classifier into `out` after the last layer (bf::RowArgsBf16, which adds satcnt, and fs::RowArgs3)
template <typename Args, typename H>
Args row_args(const savad_model* m, const FragImage& im, bool folded, int l, int B, int T, int nblk, H* hb, char* const* nxt, float* out) {
    const weights::Layout& w = m->w;
    const float *R = m->d_raw, *P = m->d_packed;
    const auto& f = im.at->layer[l];
    const bool last = l + 1 == m->cfg.num_layers;
    Args A;
    A.B = B;
    A.T = T;
    A.nblk = nblk;
    A.hbuf = hb;
    A.wo_frag = im.d + f.wo;  // (not read by the folded launches)
    A.bo = R + w.lr[l].bo;
    A.w1_frag = im.d + f.w1;
    A.b1 = P + w.lp[l].b1;
    A.w2_frag = im.d + f.w2;
    A.b2 = R + w.lr[l].b2;
    A.wn_frag = last ? nullptr : qkv_frags(im, l + 1, folded);
    A.wc = last ? P + w.p_wc : nullptr;
    A.bn = last ? P + w.p_bc : qkv_bias(m, l + 1, folded);
    A.qf = nxt[0];
    A.kf = nxt[1];
    A.vtf = nxt[2];
    A.out = out;
    A.qscale = qscale();
    return A;
}

// bf16-operand forward, T > 32: input_qkv -> [attention -> row] x L on fragment-major buffers
void forward_bf16(savad_model* m, const sched::ForwardPlan& bp, const Features& in, int B, int T, float* out, char* W, hipStream_t st, Prof& prof) {
    bf::hres_t* hb = (bf::hres_t*)(W + bp.h);
    char *qf = W + bp.q, *kf = W + bp.k, *vtf = W + bp.v, *ctxf = W + bp.ctx;
    const int L = m->cfg.num_layers, F = in.F;
    const long xbs = in.xbs;
    const float c = qscale();
    const FragImage& im = m->bf16;
    const char* win = im.d + im.at->win;
    const float* bin = m->d_raw + m->w.r_bin;
    const bool fused = bp.form == sched::FUSED;
    auto run = [&](auto nw_tag) {
        constexpr int NW = decltype(nw_tag)::value;
        constexpr int ring = bf::Ring<NW>::NRING * bf::RING_BYTES;
        const int grid_rows = bp.nblk_pad / NW;
        const dim3 wg(64 * NW);
        if (bp.input_p) {  // the persistent weights-resident form of the stage
            auto go = [&](auto xt, auto ks_tag) {
                using XT = decltype(xt);
                constexpr int KSC = decltype(ks_tag)::value;
                hipLaunchKernelGGL((bf::input_qkv_kernel_bf16_p<XT, 8, KSC>), dim3(m->n_cu), dim3(512), bf::input_p_lds_bytes(F / 16), st,
                                   (const XT*)in.x, xbs, B, T, F, bp.nblk, bp.nblk_pad, win, bin, m->d_pe,
                                   qkv_frags(im, 0, false), qkv_bias(m, 0, false), hb, qf, kf, vtf, c, m->d_sat);
            };
            if (bp.KSC == 5) {
                if (in.is_bf16) go(__bf16{}, std::integral_constant<int, 5>{}); else go(float{}, std::integral_constant<int, 5>{});
            } else {
                if (in.is_bf16) go(__bf16{}, std::integral_constant<int, 0>{}); else go(float{}, std::integral_constant<int, 0>{});
            }
        } else if (in.is_bf16)
            hipLaunchKernelGGL((bf::input_qkv_kernel_bf16<__bf16, NW>), dim3(grid_rows), wg, ring + 3 * D * 4, st, (const __bf16*)in.x, xbs,
                               B, T, F, bp.nblk, win, bin, m->d_pe, qkv_frags(im, 0, false), qkv_bias(m, 0, false), hb,
                               qf, kf, vtf, c, m->d_sat);
        else
            hipLaunchKernelGGL((bf::input_qkv_kernel_bf16<float, NW>), dim3(grid_rows), wg, ring + 3 * D * 4, st, (const float*)in.x, xbs, B,
                               T, F, bp.nblk, win, bin, m->d_pe, qkv_frags(im, 0, false), qkv_bias(m, 0, false), hb, qf,
                               kf, vtf, c, m->d_sat);
        prof.mark("input_qkv_bf16");
        char* sets[2][3] = {{qf, kf, vtf}, {W + bp.q2, W + bp.k2, W + bp.v2}};
        for (int l = 0; l < L; ++l) {
            const bool last = l + 1 == L;
            char** cur = fused ? sets[l & 1] : sets[0];
            char** nxt = fused ? sets[(l + 1) & 1] : sets[0];
            bf::RowArgsBf16 A = row_args<bf::RowArgsBf16>(m, im, false, l, B, T, bp.nblk, hb, nxt, out);
            A.satcnt = m->d_sat;
            const dim3 grid_groups(8 * (((long)B * bp.NG + 7) / 8));  // a workgroup per query-block group, whole XCD rounds
            if (fused) {
                if (last)
                    hipLaunchKernelGGL((bf::attention_row_kernel_bf16<true, NW>), grid_groups, wg, ring + 9 * D * 4, st, cur[0], cur[1], cur[2], bp.NG, A);
                else
                    hipLaunchKernelGGL((bf::attention_row_kernel_bf16<false, NW>), grid_groups, wg, ring + 9 * D * 4, st, cur[0], cur[1], cur[2], bp.NG, A);
                prof.mark(last ? "attention_row_last_bf16" : "attention_row_bf16");
                continue;
            }
            if (bp.attn == sched::ATTN_PACKED)
                hipLaunchKernelGGL(bf::attention_packed_kernel_bf16, dim3((bp.nblk + 3) / 4), dim3(256), 0, st, qf, kf, vtf, ctxf,
                                   B, T, bp.nblk);
            else if (bp.attn == sched::ATTN_PW_NOSPLIT)  // persistent 4 x 64-row attention (savad_attn_pw_bf16.h)
                hipLaunchKernelGGL(bf::attention_pw_kernel_bf16_nosplit, dim3(bf::PW_GRID), dim3(256), bf::PW_LDS_BYTES, st, qf, kf, vtf, ctxf, B, T);
            else if (bp.attn == sched::ATTN_PW)
                hipLaunchKernelGGL(bf::attention_pw_kernel_bf16, dim3(bf::PW_GRID), dim3(256), bf::PW_LDS_BYTES, st, qf, kf, vtf, ctxf, B, T);
            else
                hipLaunchKernelGGL((bf::attention_kernel_bf16<NW>), grid_groups, wg, ring, st, qf, kf, vtf, ctxf, B, T, bp.NG);
            prof.mark("attention_bf16");
            if (last)
                hipLaunchKernelGGL((bf::row_kernel_bf16<true, NW>), dim3(grid_rows), wg, ring + 9 * D * 4, st, ctxf, A);
            else
                hipLaunchKernelGGL((bf::row_kernel_bf16<false, NW>), dim3(grid_rows), wg, ring + 9 * D * 4, st, ctxf, A);
            prof.mark(last ? "row_last_bf16" : "row_bf16");
        }
    };
    if (bp.wide)
        run(std::integral_constant<int, 8>{});
    else
        run(std::integral_constant<int, 4>{});
}

int prepare_f32s_launch(savad_model* m) {
    int rc;
    if (m->f32s.lds_attrs_set) return SAVAD_OK;
    if ((rc = allow_lds(fs::input_qkv_kernel_f32s_plain, fs::NRING3 * fs::SLOT_BYTES + 3 * D * 4))) return rc;
    if ((rc = allow_lds(fs::input_qkv_kernel_f32s, fs::NRING3 * fs::SLOT_BYTES + 3 * D * 4))) return rc;
    if ((rc = allow_lds(fs::attention_row_kernel_f32s<false, false>, fs::ROW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(fs::attention_row_kernel_f32s<true, false>, fs::ROW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(fs::attention_row_kernel_f32s<false, true>, fs::ROW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(fs::attention_row_kernel_f32s<true, true>, fs::ROW_LDS_BYTES))) return rc;
    if ((rc = allow_lds(fs::packed_forward_kernel_f32s, fs::packed_f32s_lds_bytes(fs::PACKED_F32S_MAX_LAYERS)))) return rc;
    if ((rc = allow_lds(fs::packed_forward_kernel_f32s_ns, fs::nsf_lds_bytes(fs::PACKED_F32S_MAX_LAYERS)))) return rc;
    m->f32s.lds_attrs_set = true;
    return SAVAD_OK;
}

// fp32s forward (precision 2), T > 32: input_qkv -> [attention + row chain] x L, every GEMM as six bf16 MFMA products of three-piece operands
void forward_f32s(savad_model* m, const sched::ForwardPlan& bp, const Features& in, int B, int T, float* out, char* W, hipStream_t st, Prof& prof) {
    float* hb = (float*)(W + bp.h);
    const int L = m->cfg.num_layers;
    const FragImage& im = m->f32s;
    char* sets[2][3] = {{W + bp.q, W + bp.k, W + bp.v}, {W + bp.q2, W + bp.k2, W + bp.v2}};
    const bool folded = bp.fold_v;  // otherwise the T <= 32 form of the launch: the plain Q/K/V images and its own out-projection
    const auto input_qkv = folded ? fs::input_qkv_kernel_f32s : fs::input_qkv_kernel_f32s_plain;
    hipLaunchKernelGGL(input_qkv, dim3(bp.nblk_pad / 4), dim3(256), fs::NRING3 * fs::SLOT_BYTES + 3 * D * 4, st, (const float*)in.x, in.xbs, B, T, in.F,
                       bp.nblk, im.d + im.at->win, m->d_raw + m->w.r_bin, m->d_pe, qkv_frags(im, 0, folded), qkv_bias(m, 0, folded), hb, sets[0][0],
                       sets[0][1], sets[0][2], qscale());
    prof.mark("input_qkv_f32s");
    const int NG = bp.NG;
    const dim3 grid(folded ? 8 * (((long)B * NG + 7) / 8) : bp.nblk_pad / 4);
    for (int l = 0; l < L; ++l) {
        const bool last = l + 1 == L;
        char** cur = sets[l & 1];
        const fs::RowArgs3 A = row_args<fs::RowArgs3>(m, im, folded, l, B, T, bp.nblk, hb, sets[(l + 1) & 1], out);
        if (!folded) {
            if (last) hipLaunchKernelGGL((fs::attention_row_kernel_f32s<true, true>), grid, dim3(256), fs::ROW_LDS_BYTES, st, cur[0], cur[1], cur[2], NG, A);
            else hipLaunchKernelGGL((fs::attention_row_kernel_f32s<false, true>), grid, dim3(256), fs::ROW_LDS_BYTES, st, cur[0], cur[1], cur[2], NG, A);
        } else {
            if (last) hipLaunchKernelGGL((fs::attention_row_kernel_f32s<true, false>), grid, dim3(256), fs::ROW_LDS_BYTES, st, cur[0], cur[1], cur[2], NG, A);
            else hipLaunchKernelGGL((fs::attention_row_kernel_f32s<false, false>), grid, dim3(256), fs::ROW_LDS_BYTES, st, cur[0], cur[1], cur[2], NG, A);
        }
        prof.mark(last ? "attention_row_last_f32s" : "attention_row_f32s");
    }
}

// exact-fp32 forward (precision 0, and the shapes precision 2 hands over), T > 32: input_qkv -> [attention -> row] x L on row-major fp32 buffers
void forward_f32(savad_model* m, const sched::ForwardPlan& ws, const Features& in, int B, int T, float* out, char* W, hipStream_t st, Prof& prof) {
    auto at = [W](size_t off) { return (float*)(W + off); };
    float *hb = at(ws.h), *q = at(ws.q), *k = at(ws.k), *v = at(ws.v), *op = at(ws.opart), *ml = at(ws.ml);
    const int L = m->cfg.num_layers, F = in.F;
    const float* x = (const float*)in.x;
    const long xbs = in.xbs;
    const int tiles = (int)(ws.rows_pad / TILE);
    const float c = qscale();
    const float* R = m->d_raw;
    const float* P = m->d_packed;
    const weights::Layout& w = m->w;
    const int tiles_m = (int)(ws.rows_pad / 128);
    const bool msplit = ws.msplit;
    if (msplit)
        hipLaunchKernelGGL(input_qkv_kernel_m, dim3(tiles_m), dim3(256), 0, st, x, xbs, (int)ws.rows, T, F, win_fp32(m),
                           R + w.r_bin, m->d_pe, P + w.lp[0].wqkv, P + w.lp[0].bqkv, hb, q, k, v);
    else
        hipLaunchKernelGGL(input_qkv_kernel, dim3(tiles), dim3(256), 0, st, x, xbs, (int)ws.rows, T, F, win_fp32(m),
                           R + w.r_bin, m->d_pe, P + w.lp[0].frag, P + w.lp[0].bqkv, hb, q, k, v);
    prof.mark("input_qkv");
    const int NG = ws.NG;
    if (ws.form == sched::FUSED) {
        float* qkv[2][3] = {{q, k, v}, {at(ws.q2), at(ws.k2), at(ws.v2)}};
        const int grid = (int)(8 * (((long)B * NG + 7) / 8));
        for (int l = 0; l < L; ++l) {
            const auto& r = w.lr[l];
            const auto& p = w.lp[l];
            float** cur = qkv[l & 1];
            float** nxt = qkv[(l + 1) & 1];
            if (l + 1 < L) {
                hipLaunchKernelGGL(attention_row_kernel<false>, dim3(grid), dim3(256), 0, st, cur[0], cur[1], cur[2], B, T, NG, c, hb,
                                   R + r.wo, R + r.bo, P + p.w1, P + p.b1, R + r.w2, R + r.b2, P + w.lp[l + 1].wqkv,
                                   P + w.lp[l + 1].bqkv, nxt[0], nxt[1], nxt[2], out);
                prof.mark("attention_row");
            } else {
                hipLaunchKernelGGL(attention_row_kernel<true>, dim3(grid), dim3(256), 0, st, cur[0], cur[1], cur[2], B, T, NG, c, hb,
                                   R + r.wo, R + r.bo, P + p.w1, P + p.b1, R + r.w2, R + r.b2, P + w.p_wc, P + w.p_bc, nxt[0],
                                   nxt[1], nxt[2], out);
                prof.mark("attention_row_last");
            }
        }
        return;
    }
    for (int l = 0; l < L; ++l) {
        if (ws.attn == sched::ATTN_PACKED) {
            hipLaunchKernelGGL(attention_packed_kernel, dim3(ws.nblk), dim3(64), 0, st, q, k, v, op, ml, B, T, (int)ws.rows, c);
        } else {
            const int grid = (int)(8 * (((long)B * NG * ws.S + 7) / 8));
            hipLaunchKernelGGL(attention_kernel, dim3(grid), dim3(256), 0, st, q, k, v, op, ml, B, T, (int)ws.rows_pad,
                               ws.S, NG, c);
        }
        prof.mark("attention");
        const auto& r = w.lr[l];
        const auto& p = w.lp[l];
#define SAVAD_ROW_ARGS(WN, BN) op, ml, ws.S, (int)ws.rows, (int)ws.rows_pad, c, hb, R + r.wo, R + r.bo, P + p.w1, P + p.b1, \
                               R + r.w2, R + r.b2, WN, BN, q, k, v, out
#define SAVAD_ROWN_ARGS(NFRAG, WN, BN) op, ml, ws.S, (int)ws.rows, (int)ws.rows_pad, c, hb, P + p.frag, R + r.bo, P + p.b1, R + r.b2, \
                                       NFRAG, WN, BN, q, k, v, out
        if (l + 1 < L) {
            if (msplit)
                hipLaunchKernelGGL(row_kernel_m<false>, dim3(tiles_m), dim3(256), 0, st,
                                   SAVAD_ROW_ARGS(P + w.lp[l + 1].wqkv, P + w.lp[l + 1].bqkv));
            else
                hipLaunchKernelGGL(row_kernel<false>, dim3(tiles), dim3(256), 0, st, SAVAD_ROWN_ARGS(P + w.lp[l + 1].frag, P, P + w.lp[l + 1].bqkv));
            prof.mark("row");
        } else {
            if (msplit)
                hipLaunchKernelGGL(row_kernel_m<true>, dim3(tiles_m), dim3(256), 0, st,
                                   SAVAD_ROW_ARGS(P + w.p_wc, P + w.p_bc));
            else
                hipLaunchKernelGGL(row_kernel<true>, dim3(tiles), dim3(256), 0, st, SAVAD_ROWN_ARGS(P + p.frag, P + w.p_wc, P + w.p_bc));
            prof.mark("row_last");
        }
#undef SAVAD_ROW_ARGS
#undef SAVAD_ROWN_ARGS
    }
}

// every forward entry point ends here: validate, plan once (savad_schedule.h), make the family's weights ready, launch what the plan
// names.  xbs_in: elements between consecutive sequences of x (savad_forward_strided), 0 = T * F
int forward_any(savad_handle m, const void* x, int x_dtype, int B, int T, long xbs_in, float* out, void* workspace, size_t workspace_bytes,
                void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    if (B < 0 || T < 0) return fail(SAVAD_E_INVALID, "negative shape B=%d T=%d", B, T);
    if (B == 0 || T == 0) return SAVAD_OK;
    if (!x || !out || !workspace) return fail(SAVAD_E_INVALID, "null tensor pointer");
    if ((double)B * T * D >= 2.0e9) return fail(SAVAD_E_UNSUPPORTED, "B*T too large");
    if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)workspace) & 15)
        return fail(SAVAD_E_INVALID, "x, out and workspace must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    const sched::ForwardPlan p = sched::plan_forward(knobs_of(m), B, T, x_dtype == 1, xbs_in);
    if (p.err) return fail(p.err, "%s", p.msg);
    if (workspace_bytes < p.total) return fail(SAVAD_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    int rc;
    if ((rc = ensure_ready(m, p.family, T, st))) return rc;
    char* W = (char*)workspace;
    const Features in = forward_input(m, p, x, p.family == sched::BF16 ? x_dtype : 0, B, T, xbs_in, W, st);
    Prof prof(m, st);
    if (p.form == sched::SINGLE) {
        WindowOffsets none;
        none.w = 0;
        prof.mark(launch_single(m, p.family, p.variant, st, (const float*)in.x, B, T, in.F, out, none, 0));
    } else {
        switch (p.family) {
            case sched::GENERIC: forward_generic(m, p, (const float*)x, B, T, out, workspace, st, prof); break;
            case sched::BF16: forward_bf16(m, p, in, B, T, out, W, st, prof); break;
            case sched::F32S: forward_f32s(m, p, in, B, T, out, W, st, prof); break;
            default: forward_f32(m, p, in, B, T, out, W, st, prof);
        }
    }
    prof.done();
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}
}  // namespace

// x_dtype: 0 = fp32 features, 1 = bf16 features (bf16 precision only)
SAVAD_EXPORT int savad_forward_ex(savad_handle m, const void* x, int x_dtype, int B, int T, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    if (x_dtype == 0 && m->precision != 1) return savad_forward(m, (const float*)x, B, T, out, workspace, workspace_bytes, stream);
    if (x_dtype < 0 || x_dtype > 1) return fail(SAVAD_E_INVALID, "x_dtype %d", x_dtype);
    if (m->w.generic) return fail(SAVAD_E_UNSUPPORTED, "bf16 features need the d_model=128 kernels (this handle: d_model=%d, fp32)", m->cfg.d_model);
    if (m->precision != 1) return fail(SAVAD_E_UNSUPPORTED, "bf16 features need savad_set_precision(h, 1)");
    return forward_any(m, x, x_dtype, B, T, 0, out, workspace, workspace_bytes, stream);
}

SAVAD_EXPORT int savad_forward_strided(savad_handle m, const void* x, int x_dtype, int B, int T, long x_batch_stride, float* out,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    if (m->w.generic) return fail(SAVAD_E_UNSUPPORTED, "strided input needs the d_model=128 kernels");
    if (T <= 32) return fail(SAVAD_E_UNSUPPORTED, "strided input is for sequences longer than 32 frames (windows of T <= 32 are read in place by savad_predict_probabilities)");
    if (m->w.FP != m->cfg.feature_size) return fail(SAVAD_E_UNSUPPORTED, "strided input needs feature_size %% 16 == 0 (no padding copy)");
    const long F = m->cfg.feature_size;
    if (x_batch_stride <= 0 || x_batch_stride % 4 || x_batch_stride % F)
        return fail(SAVAD_E_INVALID, "x_batch_stride=%ld (a positive multiple of feature_size and of 4 elements)", x_batch_stride);
    if (x_dtype < 0 || x_dtype > 1 || (x_dtype == 1 && m->precision != 1)) return fail(SAVAD_E_INVALID, "x_dtype %d (bf16 features need savad_set_precision(h, 1))", x_dtype);
    return forward_any(m, x, x_dtype, B, T, x_batch_stride, out, workspace, workspace_bytes, stream);
}

SAVAD_EXPORT int savad_forward(savad_handle m, const float* x, int B, int T, float* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
    return forward_any(m, x, 0, B, T, 0, out, workspace, workspace_bytes, stream);
}

SAVAD_EXPORT int savad_set_profiling(savad_handle m, int capacity) {
    if (!m || capacity < 0) return fail(SAVAD_E_INVALID, "bad argument");
    for (hipEvent_t e : m->events) hipEventDestroy(e);
    m->events.clear();
    m->prof_capacity = capacity;
    m->prof_used = 0;
    m->prof_nk = 0;
    m->prof_skip = 0;
    m->events.resize((size_t)capacity * MAX_EVENTS);
    for (auto& e : m->events) HIP_TRY(hipEventCreate(&e));
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_profiling_skip(savad_handle m, int forwards) {
    if (!m || forwards < 0) return fail(SAVAD_E_INVALID, "bad argument");
    m->prof_skip = forwards;
    return SAVAD_OK;
}

// Average duration (ms) of each launch position over the profiled forwards recorded since
// savad_set_profiling; the caller must have synchronised the stream.
SAVAD_EXPORT int savad_last_kernel_times(savad_handle m, const char** names, float* ms, int max) {
    if (!m || m->prof_used == 0) return 0;
    const int nk = m->prof_nk < max ? m->prof_nk : max;
    for (int i = 0; i < nk; ++i) {
        double acc = 0;
        for (int f = 0; f < m->prof_used; ++f) {
            hipEvent_t* ev = m->events.data() + (size_t)f * MAX_EVENTS;
            float t = 0;
            if (hipEventElapsedTime(&t, ev[i], ev[i + 1]) != hipSuccess) return fail(SAVAD_E_HIP, "hipEventElapsedTime failed");
            acc += t;
        }
        ms[i] = (float)(acc / m->prof_used);
        if (names) names[i] = m->knames[i];
    }
    m->prof_used = 0;
    return nk;
}

SAVAD_EXPORT int savad_window_offsets(int half, int jump, int32_t* offsets) {
    if (half < 0 || jump <= 0) return fail(SAVAD_E_INVALID, "half=%d jump=%d", half, jump);
    const long W = windows::offsets(half, jump, nullptr);   // (the caller's buffer holds every offset, however many)
    return (int)windows::offsets(half, jump, offsets, W);
}

namespace {
// the window geometry as the kernels take it; a window longer than WindowOffsets holds is refused
int window_offsets(int half, int jump, WindowOffsets* wo) {
    if (half < 0 || jump <= 0) return fail(SAVAD_E_INVALID, "half=%d jump=%d", half, jump);
    static_assert(std::is_same<decltype(wo->off[0]), int32_t&>::value && sizeof wo->off == sizeof(int32_t) * windows::MAX_FRAMES, "WindowOffsets::off");
    const long W = windows::offsets(half, jump, wo->off);
    if (W > windows::MAX_FRAMES) return fail(SAVAD_E_UNSUPPORTED, "%s", windows::TOO_LONG);
    wo->w = (int)W;
    return SAVAD_OK;
}

// The items [0, n_items) in `chunk` steps: gather(first, count) leaves a chunk's windows in `win`, one savad_forward turns them into
// the chunk's log-probs at logp + first * W * 2 (16-byte aligned: chunk is even).  The boost that follows reads all of logp.
template <class Gather>
int forward_chunks(savad_handle m, int n_items, int chunk, int W, float* win, float* logp, void* fwd, size_t fwd_bytes, void* stream,
                   Gather gather) {
    for (int first = 0; first < n_items; first += chunk) {
        const int count = n_items - first < chunk ? n_items - first : chunk;
        if (int rc = gather(first, count)) return rc;
        if (int rc = savad_forward(m, win, count, W, logp + (size_t)first * W * 2, fwd, fwd_bytes, stream)) return rc;
    }
    return SAVAD_OK;
}
}  // namespace

SAVAD_EXPORT int savad_gather_windows(const float* feature, int N, int F, int half, int jump, int first, int count,
                                      float* windows, int64_t* positions, void* stream) {
    if (count == 0) return SAVAD_OK;
    if (!feature || !windows || N <= 0 || F <= 0 || first < 0 || count < 0) return fail(SAVAD_E_INVALID, "bad argument");
    WindowOffsets wo;
    int rc = window_offsets(half, jump, &wo);
    if (rc) return rc;
    if ((long)half + first + count - 1 + wo.off[wo.w - 1] >= N || half + first + wo.off[0] < 0)
        return fail(SAVAD_E_INVALID, "window [%d,%d) reaches outside the %d feature frames", first, first + count, N);
    const int grid = grid_for((long)count * wo.w * (F % 4 ? F : F / 4), 2048);
    if (F % 4)
        hipLaunchKernelGGL(gather_windows_scalar_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, feature, F, half, first,
                           count, wo, windows, positions);
    else
        hipLaunchKernelGGL(gather_windows_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, feature, F, half, first,
                           count, wo, windows, positions);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_boost(const float* logp, const int64_t* positions, int count, int N, int W, float* boosted_ws,
                             float* probs, float* mean, void* stream) {
    if (N <= 0) return SAVAD_OK;
    if (!boosted_ws || !probs || W <= 0 || count < 0 || (count > 0 && (!logp || !positions)))
        return fail(SAVAD_E_INVALID, "bad argument");
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(boosted_ws, 0, sizeof(float) * (size_t)N * W * 2, st));
    if (count > 0) {
        const size_t cw = (size_t)count * W;
        hipLaunchKernelGGL(boost_scatter_kernel, dim3(grid_for((long)cw, 2048)), dim3(256), 0, st, logp, positions, cw, W, boosted_ws);
    }
    hipLaunchKernelGGL(boost_softmax_kernel, dim3(grid_for(N, 2048)), dim3(256), 0, st, boosted_ws, N, W, probs, mean);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- the whole of predict_probabilities (vad/predictor.py:159-262) in one call -------------------------------
namespace {
// validates the geometry and plans the call (savad_schedule.h: plan_predict)
int plan_predict(savad_model* m, int N, int half, int jump, int chunk, sched::PredictPlan* p) {
    if (N < 0 || half < 0 || jump <= 0 || chunk <= 0) return fail(SAVAD_E_INVALID, "N=%d half=%d jump=%d chunk=%d", N, half, jump, chunk);
    *p = sched::plan_predict(knobs_of(m), N, half, jump, chunk);
    if (p->err) return fail(p->err, "%s", p->msg);
    if (!p->windowed && (double)p->chunk * p->W * D >= 2.0e9)   // the chunk-sized forward's own limit (savad_workspace_bytes)
        return fail(SAVAD_E_UNSUPPORTED, "B*T=%ld rows exceed the 32-bit tile index range", (long)p->chunk * p->W);
    return SAVAD_OK;
}
}  // namespace

SAVAD_EXPORT int savad_predict_workspace_bytes(savad_handle m, int N, int half, int jump, int chunk, size_t* bytes) {
    if (!m || !bytes) return fail(SAVAD_E_INVALID, "null argument");
    sched::PredictPlan p;
    int rc = plan_predict(m, N, half, jump, chunk, &p);
    if (rc) return rc;
    *bytes = p.total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_predict_probabilities(savad_handle m, const float* feature, int N, int half, int jump, int chunk, float* probs,
                                             float* mean, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    if (N == 0) return SAVAD_OK;
    if (!feature || !probs || !workspace) return fail(SAVAD_E_INVALID, "null tensor pointer");
    if (((uintptr_t)feature | (uintptr_t)workspace) & 15) return fail(SAVAD_E_INVALID, "feature and workspace must be 16-byte aligned");
    sched::PredictPlan p;
    int rc = plan_predict(m, N, half, jump, chunk, &p);
    if (rc) return rc;
    if (workspace_bytes < p.total) return fail(SAVAD_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    const int F = m->cfg.feature_size, W = p.W;  // (F % 4 != 0: never windowed -- m->w.FP != F -- the windows go through savad_gather_windows)
    WindowOffsets wo;
    if ((rc = window_offsets(half, jump, &wo))) return rc;
    if (p.n_items > 0 && (half + wo.off[0] < 0 || (long)half + p.n_items - 1 + wo.off[W - 1] >= N))
        return fail(SAVAD_E_INVALID, "windows reach outside the %d feature frames", N);
    char* ws = (char*)workspace;
    float* logp = (float*)(ws + p.logp);
    if (p.windowed) {   // the single-launch forwards read their windows in place
        if (p.n_items > 0 && (rc = ensure_ready(m, p.family, W, st))) return rc;
        for (int first = 0; first < p.n_items; first += p.chunk) {
            const int count = p.n_items - first < p.chunk ? p.n_items - first : p.chunk;
            launch_single(m, p.family, count == p.chunk ? p.variant : p.variant_last, st, feature, count, W, F, logp + (size_t)first * W * 2, wo,
                          half + first);
        }
    } else {
        float* win = (float*)(ws + p.windows);
        rc = forward_chunks(m, p.n_items, p.chunk, W, win, logp, ws + p.fwd, p.fwd_bytes, stream, [&](int first, int count) {
            return savad_gather_windows(feature, N, F, half, jump, first, count, win, nullptr, stream);
        });
        if (rc) return rc;
    }
    hipLaunchKernelGGL(boost_gather_kernel, dim3(grid_for(N, 2048)), dim3(256), 0, st, logp, p.n_items, N, half, wo, probs, mean);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- many clips in one call (savad_batch_kernels.h; savad_schedule.h: plan_predict_batch) --------------------
namespace {
// the HOST table validated and counted; the refusal's message when it is not a clip table
int clip_table(const int32_t* clip_first_host, int C, int half, int jump, sched::ClipTotals* t) {
    *t = sched::clip_totals(clip_first_host, C, half, jump);
    return t->err ? fail(t->err, "%s", t->msg) : SAVAD_OK;
}

void launch_items_scan(const int32_t* clip_first, int C, int half, int32_t* items_first, hipStream_t st) {
    hipLaunchKernelGGL(clip_items_scan_kernel, dim3(1), dim3(BATCH_SCAN_THREADS), 0, st, clip_first, C, half, items_first);
}

// items [first, first + count) of a table whose items_first the device already holds
void launch_gather_batch(const float* feature, int F, const int32_t* clip_first, const int32_t* items_first, int C, int half, int first,
                         int count, const WindowOffsets& wo, float* windows, int64_t* positions, hipStream_t st) {
    const int tiles = (count + BATCH_GATHER_ITEMS - 1) / BATCH_GATHER_ITEMS;
    const dim3 grid(tiles < 4096 ? tiles : 4096);
    if (F % 4)
        hipLaunchKernelGGL(gather_windows_batch_kernel<false>, grid, dim3(256), 0, st, feature, F, clip_first, items_first, C, half, first,
                           count, wo, windows, positions);
    else
        hipLaunchKernelGGL(gather_windows_batch_kernel<true>, grid, dim3(256), 0, st, feature, F, clip_first, items_first, C, half, first,
                           count, wo, windows, positions);
}

int plan_predict_batch(savad_model* m, const int32_t* clip_first_host, int C, int half, int jump, int chunk, sched::PredictBatchPlan* p) {
    *p = sched::plan_predict_batch(knobs_of(m), clip_first_host, C, half, jump, chunk);
    if (p->err) return fail(p->err, "%s", p->msg);
    if ((double)p->chunk * p->W * D >= 2.0e9)   // the chunk-sized forward's own limit (savad_workspace_bytes)
        return fail(SAVAD_E_UNSUPPORTED, "B*T=%ld rows exceed the 32-bit tile index range", (long)p->chunk * p->W);
    return SAVAD_OK;
}
}  // namespace

SAVAD_EXPORT int savad_gather_windows_batch(const float* feature, const int32_t* clip_first_host, const int32_t* clip_first, int C, int F,
                                            int half, int jump, int first, int count, int32_t* items_first, float* windows,
                                            int64_t* positions, void* stream) {
    sched::ClipTotals t;
    int rc = clip_table(clip_first_host, C, half, jump, &t);
    if (rc) return rc;
    if (F <= 0 || first < 0 || count < 0) return fail(SAVAD_E_INVALID, "F=%d first=%d count=%d", F, first, count);
    if ((long)first + count > t.n_items)
        return fail(SAVAD_E_INVALID, "items [%d,%ld) reach outside the %d windows of the clips", first, (long)first + count, t.n_items);
    if (count == 0) return SAVAD_OK;
    if (!feature || !clip_first || !items_first || !windows) return fail(SAVAD_E_INVALID, "null pointer");
    if (F % 4 == 0 && (((uintptr_t)feature | (uintptr_t)windows) & 15))
        return fail(SAVAD_E_INVALID, "feature and windows must be 16-byte aligned when F is a multiple of 4");
    WindowOffsets wo;
    if ((rc = window_offsets(half, jump, &wo))) return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_items_scan(clip_first, C, half, items_first, st);
    launch_gather_batch(feature, F, clip_first, items_first, C, half, first, count, wo, windows, positions, st);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_boost_batch(const float* logp, const int32_t* clip_first_host, const int32_t* clip_first, int C, int half, int jump,
                                   int32_t* items_first, float* probs, float* mean, void* stream) {
    sched::ClipTotals t;
    int rc = clip_table(clip_first_host, C, half, jump, &t);
    if (rc) return rc;
    if (t.rows == 0) return SAVAD_OK;
    if (!clip_first || !items_first || !probs || (t.n_items > 0 && !logp)) return fail(SAVAD_E_INVALID, "null pointer");
    WindowOffsets wo;
    if ((rc = window_offsets(half, jump, &wo))) return rc;
    hipStream_t st = (hipStream_t)stream;
    launch_items_scan(clip_first, C, half, items_first, st);
    hipLaunchKernelGGL(boost_gather_batch_kernel, dim3(grid_for(t.rows, 2048)), dim3(256), 0, st, logp, clip_first, (const int32_t*)items_first,
                       C, t.rows, half, wo, probs, mean);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_predict_batch_workspace_bytes(savad_handle m, const int32_t* clip_first_host, int C, int half, int jump, int chunk,
                                                     size_t* bytes) {
    if (!m || !bytes) return fail(SAVAD_E_INVALID, "null argument");
    sched::PredictBatchPlan p;
    int rc = plan_predict_batch(m, clip_first_host, C, half, jump, chunk, &p);
    if (rc) return rc;
    *bytes = p.total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_predict_probabilities_batch(savad_handle m, const float* feature, const int32_t* clip_first_host,
                                                   const int32_t* clip_first, int C, int half, int jump, int chunk, float* probs, float* mean,
                                                   void* workspace, size_t workspace_bytes, void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    sched::PredictBatchPlan p;
    int rc = plan_predict_batch(m, clip_first_host, C, half, jump, chunk, &p);
    if (rc) return rc;
    if (p.rows == 0) return SAVAD_OK;
    if (!feature || !clip_first || !probs || !workspace) return fail(SAVAD_E_INVALID, "null tensor pointer");
    if (((uintptr_t)feature | (uintptr_t)workspace) & 15) return fail(SAVAD_E_INVALID, "feature and workspace must be 16-byte aligned");
    if (workspace_bytes < p.total) return fail(SAVAD_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, p.total);
    hipStream_t st = (hipStream_t)stream;
    const int F = m->cfg.feature_size, W = p.W;
    WindowOffsets wo;
    if ((rc = window_offsets(half, jump, &wo))) return rc;
    char* ws = (char*)workspace;
    int32_t* items_first = (int32_t*)(ws + p.items_first);
    float* logp = (float*)(ws + p.logp);
    float* win = (float*)(ws + p.windows);
    launch_items_scan(clip_first, C, half, items_first, st);
    rc = forward_chunks(m, p.n_items, p.chunk, W, win, logp, ws + p.fwd, p.fwd_bytes, stream, [&](int first, int count) {
        launch_gather_batch(feature, F, clip_first, items_first, C, half, first, count, wo, win, nullptr, st);
        HIP_TRY(hipGetLastError());
        return (int)SAVAD_OK;
    });
    if (rc) return rc;
    hipLaunchKernelGGL(boost_gather_batch_kernel, dim3(grid_for(p.rows, 2048)), dim3(256), 0, st, logp, clip_first, (const int32_t*)items_first, C,
                       p.rows, half, wo, probs, mean);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_stream_window_count(int N, int T, int hop) {
    if (N <= 0 || T <= 0 || hop <= 0) return fail(SAVAD_E_INVALID, "N=%d T=%d hop=%d", N, T, hop);
    return N <= T ? 1 : (N - T + hop - 1) / hop + 1;
}

SAVAD_EXPORT int savad_gather_strided(const float* feature, int N, int F, int T, int hop, int first, int count,
                                      float* windows, void* stream) {
    if (count == 0) return SAVAD_OK;
    if (!feature || !windows || N <= 0 || F <= 0 || F % 4 || T <= 0 || hop <= 0 || first < 0 || count < 0)
        return fail(SAVAD_E_INVALID, "bad argument (F must be a multiple of 4)");
    const int grid = grid_for((long)count * T * (F / 4));
    hipLaunchKernelGGL(gather_strided_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, feature, N, F, T, hop, first,
                       count, windows);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_overlap_merge(const float* logp, int W, int N, int T, int hop, float* probs, void* stream) {
    if (N <= 0) return SAVAD_OK;
    if (!logp || !probs || W <= 0 || T <= 0 || hop <= 0) return fail(SAVAD_E_INVALID, "bad argument");
    const int grid = grid_for(N, 2048);
    hipLaunchKernelGGL(overlap_merge_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, logp, W, N, T, hop, probs);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- device tables of the audio paths (host builders and layouts: savad_audio_host.h) -----------------------------------------
// A table is built on the host and uploaded on first use by the device that needs it -- synchronously, so never inside a
// graph capture: savad_frontend_prepare and savad_resample_prepare are the explicit steps before one -- and stays for the
// life of the process.  One mutex guards everything in this section.
namespace {

std::mutex g_audio_mutex;
std::vector<int> g_audio_n_cu;   // by device ordinal; 0 = the device is not set up yet

bool aligned16(const void* a, const void* b) { return (((uintptr_t)a | (uintptr_t)b) & 15) == 0; }
float* at(float* base, size_t bytes) { return reinterpret_cast<float*>(reinterpret_cast<char*>(base) + bytes); }

int audio_device(int dev, int* n_cu);   // (defined after the last entry point of the audio paths)

// tables with elements T... under a Key, per device
template <class Key, class... T>
struct DeviceTables {
    using Host = std::tuple<std::vector<T>...>;
    using Ptrs = std::tuple<T*...>;
    static inline std::map<std::pair<int, Key>, Ptrs> resident;

    // the key's tables on the current device; on a miss build(Host&) fills the host arrays (or returns its refusal).
    // The caller holds g_audio_mutex.
    template <class Build>
    static int get(const Key& key, Build&& build, Ptrs* out, int* n_cu) {
        int rc, dev = 0;
        HIP_TRY(hipGetDevice(&dev));
        if ((rc = audio_device(dev, n_cu))) return rc;
        auto it = resident.find({dev, key});
        if (it == resident.end()) {
            Host h;
            Ptrs p;
            if ((rc = build(h)) || (rc = upload(h, p, std::index_sequence_for<T...>{}))) return rc;
            it = resident.emplace(std::make_pair(dev, key), p).first;
        }
        *out = it->second;
        return SAVAD_OK;
    }

    // one allocation, every array starting 256-byte aligned; given back if a copy fails
    template <size_t... I>
    static int upload(const Host& h, Ptrs& p, std::index_sequence<I...>) {
        Arena a;
        const size_t off[] = {a.take(std::get<I>(h).size() * sizeof(T))...};
        char* base = nullptr;
        HIP_TRY(hipMalloc(&base, a.off));
        hipError_t e = hipSuccess;
        auto copy = [&](const auto& v, size_t at) { return v.empty() ? hipSuccess : hipMemcpy(base + at, v.data(), v.size() * sizeof(v[0]), hipMemcpyHostToDevice); };
        ((e = e != hipSuccess ? e : copy(std::get<I>(h), off[I])), ...);
        if (e != hipSuccess) {
            hipFree(base);
            return fail(SAVAD_E_HIP, "table upload: %s", hipGetErrorString(e));
        }
        ((std::get<I>(p) = reinterpret_cast<T*>(base + off[I])), ...);
        return SAVAD_OK;
    }
};

// ---- log-mel front-end (savad_logmel.h) ---------------------------------------------------------
int g_logmel_algorithm = 0;

int fft_tables_checked(std::vector<float>& t1, std::vector<float>& t3, std::vector<float>& tm) {
    return mel::fft_tables(t1, t3, tm) ? SAVAD_OK : fail(SAVAD_E_STATE, "log-mel tables: a filter weight falls outside the kernel's pair -> mel block pattern");
}

// DFT and mel fragments of the DFT-as-GEMM kernel (algorithm 1) | t1, t3, tm of the factored kernel (algorithm 0): 1.1 MB per device
using MelTables = DeviceTables<std::monostate, float, float, float, float, float>;
int mel_tables(MelTables::Ptrs* t, int* n_cu) {
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    return MelTables::get({}, [](MelTables::Host& h) {
        auto& [dft, melf, t1, t3, tm] = h;
        dft = mel::dft_fragments();
        melf = mel::mel_fragments();
        return fft_tables_checked(t1, t3, tm);
    }, t, n_cu);
}

}  // namespace

SAVAD_EXPORT int savad_logmel_frames(int n_samples) { return n_samples < 0 ? fail(SAVAD_E_INVALID, "n_samples") : 1 + n_samples / mel::HOP; }
SAVAD_EXPORT size_t savad_logmel_workspace_bytes(int n_samples) { return mel::workspace_whole(n_samples).total; }
SAVAD_EXPORT size_t savad_logmel_span_workspace_bytes(int frame_count) { return mel::workspace_span(frame_count).total; }
SAVAD_EXPORT int savad_logmel_set_algorithm(int algorithm) {
    if (algorithm < 0 || algorithm > 1) return fail(SAVAD_E_INVALID, "log-mel algorithm %d (0 = factored DFT, 1 = DFT as one GEMM)", algorithm);
    g_logmel_algorithm = algorithm;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_logmel_table_floats(int which) {
    return which == 0 ? mel::FFT_T1_FLOATS : which == 1 ? mel::FFT_T3_FLOATS : which == 2 ? mel::FFT_TM_FLOATS : fail(SAVAD_E_INVALID, "table %d", which);
}
SAVAD_EXPORT int savad_logmel_tables_host(float* t1, float* t3, float* tm) {
    if (!t1 || !t3 || !tm) return fail(SAVAD_E_INVALID, "null argument");
    std::vector<float> a, b, c;
    if (int rc = fft_tables_checked(a, b, c)) return rc;
    memcpy(t1, a.data(), a.size() * sizeof(float));
    memcpy(t3, b.data(), b.size() * sizeof(float));
    memcpy(tm, c.data(), c.size() * sizeof(float));
    return SAVAD_OK;
}
// 16-bit PCM -> float32 in [-1, 1): sample / 32768 (exact), what soundfile hands the reference for a PCM16 file
// (vad/data_models/audio_data.py:21-24,32).  The source format of an upload from the host: half the bytes of the float signal.
__global__ void pcm16_to_f32_kernel(const short* __restrict__ pcm, long n, float* __restrict__ out) {
    const long n4 = ((uintptr_t)pcm & 7) == 0 ? n / 4 : 0;   // 8-byte pieces when the slice starts on one
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const short4 v = reinterpret_cast<const short4*>(pcm)[i];
        st4(out + 4 * i, f32x4{v.x * (1.0f / 32768.0f), v.y * (1.0f / 32768.0f), v.z * (1.0f / 32768.0f), v.w * (1.0f / 32768.0f)});
    }
    for (long i = 4 * n4 + (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
        out[i] = pcm[i] * (1.0f / 32768.0f);
}
SAVAD_EXPORT int savad_pcm16_to_f32(const short* pcm, long n_samples, float* audio, void* stream) {
    if (n_samples == 0) return SAVAD_OK;
    if (!pcm || !audio || n_samples < 0) return fail(SAVAD_E_INVALID, "bad argument");
    if (((uintptr_t)pcm & 1) || ((uintptr_t)audio & 15)) return fail(SAVAD_E_INVALID, "pcm must be 2-byte, audio 16-byte aligned");
    const long work = (n_samples + 3) / 4;
    hipLaunchKernelGGL(pcm16_to_f32_kernel, dim3(grid_for(work)), dim3(256), 0, (hipStream_t)stream, pcm, n_samples, audio);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_logmel_span_samples(long n_samples, int frame_first, int frame_count, long* first, long* count) {
    if (!first || !count || n_samples < 1 || frame_first < 0 || frame_count < 1 || frame_first + (long)frame_count > 1 + n_samples / mel::HOP)
        return fail(SAVAD_E_INVALID, "bad frame span [%d, +%d) of %ld samples", frame_first, frame_count, n_samples);
    mel::span_samples(n_samples, frame_first, frame_count, first, count);
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_logmel_span(const float* audio, long audio_first, long audio_count, long n_samples, int frame_first,
                                   int frame_count, float* workspace, float* features, void* stream) {
    if (!audio || !workspace || !features || n_samples < 1 || n_samples > 2000000000L || audio_first < 0 || audio_count < 1 ||
        audio_first + audio_count > n_samples)
        return fail(SAVAD_E_INVALID, "bad argument");
    if (frame_first < 0 || frame_count < 1 || frame_first + (long)frame_count > 1 + n_samples / mel::HOP)
        return fail(SAVAD_E_INVALID, "frames [%d, +%d) outside the %ld frames of %ld samples", frame_first, frame_count, 1 + n_samples / mel::HOP, n_samples);
    if (!aligned16(workspace, features)) return fail(SAVAD_E_INVALID, "workspace and features must be 16-byte aligned");
    long need_first, need_count;
    mel::span_samples(n_samples, frame_first, frame_count, &need_first, &need_count);
    if (audio_first > need_first + 3 || audio_first + audio_count < need_first + need_count)  // (+3: need_first was rounded down)
        return fail(SAVAD_E_INVALID, "frames [%d, +%d) read samples [%ld, +%ld); the audio slice holds [%ld, +%ld)", frame_first, frame_count,
                    need_first, need_count, audio_first, audio_count);
    hipStream_t st = (hipStream_t)stream;
    int rc, n_cu;
    MelTables::Ptrs tb;
    if ((rc = mel_tables(&tb, &n_cu))) return rc;
    const float* y0 = audio - audio_first;  // y0[i] = sample i (only indices inside the slice are ever read)
    // the frames read padded indices [j_first, j_last + 4), in 16-byte chunks (savad_logmel.h: sample stage)
    const mel::PadRule rule = mel::pad_rule(n_samples, frame_first, frame_count);
    constexpr long NEVER = mel::PAD_NEVER;
    const mel::Workspace w = mel::workspace_span(frame_count);   // (the whole-signal workspace places its pieces the same)
    mel::FftSrc src{};
    mel::PadSeg A{at(workspace, w.pad_a), 0, 0}, B{at(workspace, w.pad_b), 0, 0};
    src.y0 = y0;
    src.jA_end = -NEVER;
    src.jB0 = NEVER;
    const bool direct = (((uintptr_t)audio - (uintptr_t)audio_first * 4u) & 15) == 0;
    if (direct) {  // the mirrored head and the run past the last sample, where the frames touch them
        if (rule.a_count) A.j0 = rule.a_j0, A.count = rule.a_count;
        if (rule.b_count) B.j0 = rule.b_j0, B.count = rule.b_count;
        src.jA_end = rule.a_end;
        src.jB0 = rule.b_j0;
    } else {  // unaligned audio: the whole span from a padded (and thereby aligned) copy
        A.j0 = rule.j_first;
        A.count = (int)(rule.j_last + 4 - rule.j_first);
        src.jA_end = NEVER;
    }
    src.padA = A.dst;
    src.jA0 = A.j0;
    src.padB = B.dst;
    if (A.count + B.count > 0) {
        const long total = (long)A.count + B.count;
        hipLaunchKernelGGL(mel::reflect_pad_segments_kernel, dim3(grid_for(total)), dim3(256), 0, st, y0, n_samples, A, B);
    }
    const auto [d_dft, d_mel, d_t1, d_t3, d_tm] = tb;
    const int tiles = (frame_count + 31) / 32;
    const int grid = tiles < n_cu ? tiles : n_cu;
    hipLaunchKernelGGL(mel::logmel_fft_kernel, dim3(grid), dim3(256), mel::FFT_LDS_BYTES, st, src, frame_first, frame_count, tiles, d_t1, d_t3, d_tm,
                       features);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_logmel(const float* audio, int n_samples, float* workspace, float* features, void* stream) {
    if (!audio || !workspace || !features || n_samples < 1) return fail(SAVAD_E_INVALID, "bad argument");
    if (g_logmel_algorithm == 0)
        return savad_logmel_span(audio, 0, n_samples, n_samples, 0, 1 + n_samples / mel::HOP, workspace, features, stream);
    if (!aligned16(workspace, features)) return fail(SAVAD_E_INVALID, "workspace and features must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int rc, n_cu;
    MelTables::Ptrs tb;
    if ((rc = mel_tables(&tb, &n_cu))) return rc;
    const int n_frames = 1 + n_samples / mel::HOP;
    const long total = (long)n_samples + mel::N_FFT;
    hipLaunchKernelGGL(mel::reflect_pad_kernel, dim3(grid_for(total)), dim3(256), 0, st, audio, n_samples, workspace);
    const int tiles = (n_frames + 31) / 32;
    hipLaunchKernelGGL(mel::logmel_kernel<4>, dim3(tiles), dim3(256), 0, st, workspace, n_frames, std::get<0>(tb), std::get<1>(tb), features);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- log-mel over a clip table (savad_logmel_batch_plan.h: the host plan; savad_logmel_batch.h: the kernels) ------------------
namespace {
static_assert(sizeof(savad_audio_clip) == sizeof(melbatch::Clip), "audio clip ABI struct");

// the HOST table validated and planned; the refusal's message when it is not an audio clip table
int logmel_batch_plan(const savad_audio_clip* clips_host, int n_clips, int64_t audio_count, melbatch::Plan* p) {
    *p = melbatch::plan(reinterpret_cast<const melbatch::Clip*>(clips_host), n_clips, audio_count);
    return p->err ? fail(p->err, "%s", p->msg) : SAVAD_OK;
}
}  // namespace

SAVAD_EXPORT int savad_logmel_batch_shape(const savad_audio_clip* clips_host, int n_clips, int64_t audio_count, int64_t* rows, int64_t* tiles) {
    melbatch::Plan p;
    if (int rc = logmel_batch_plan(clips_host, n_clips, audio_count, &p)) return rc;
    if (rows) *rows = p.rows;
    if (tiles) *tiles = p.tiles;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_logmel_batch_workspace_bytes(const savad_audio_clip* clips_host, int n_clips, int64_t audio_count, size_t* bytes) {
    melbatch::Plan p;
    if (int rc = logmel_batch_plan(clips_host, n_clips, audio_count, &p)) return rc;
    if (!bytes) return fail(SAVAD_E_INVALID, "null argument");
    *bytes = p.total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_logmel_batch(const float* audio, int64_t audio_count, const savad_audio_clip* clips_host, const savad_audio_clip* clips,
                                    int n_clips, void* workspace, float* features, int32_t* clip_first, void* stream) {
    melbatch::Plan p;
    int rc = logmel_batch_plan(clips_host, n_clips, audio_count, &p);
    if (rc) return rc;
    if (g_logmel_algorithm != 0) return fail(SAVAD_E_UNSUPPORTED, "the one-GEMM DFT (savad_logmel_set_algorithm(1)) has no batch form");
    if (!clips || !workspace || !clip_first || (p.rows > 0 && (!audio || !features))) return fail(SAVAD_E_INVALID, "null pointer");
    if (!aligned16(audio, workspace) || !aligned16(features, clip_first))
        return fail(SAVAD_E_INVALID, "audio, workspace, features and clip_first must be 16-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    int n_cu;
    MelTables::Ptrs tb;
    if ((rc = mel_tables(&tb, &n_cu))) return rc;
    char* ws = (char*)workspace;
    int32_t* tiles_first = (int32_t*)(ws + p.tiles_first);
    float *head = (float*)(ws + p.head), *tail = (float*)(ws + p.tail);
    const melbatch::Clip* table = reinterpret_cast<const melbatch::Clip*>(clips);
    hipLaunchKernelGGL(melbatch::clip_frames_scan_kernel, dim3(1), dim3(BATCH_SCAN_THREADS), 0, st, table, n_clips, clip_first, tiles_first);
    if (p.tiles > 0) {
        hipLaunchKernelGGL(melbatch::reflect_pad_clips_kernel, dim3(grid_for((long)n_clips * (melbatch::HEAD_SLOT + melbatch::TAIL_SLOT))), dim3(256), 0,
                           st, audio, table, n_clips, head, tail);
        const auto [d_dft, d_mel, d_t1, d_t3, d_tm] = tb;
        const int tiles = (int)p.tiles, grid = tiles < n_cu ? tiles : n_cu;
        hipLaunchKernelGGL(melbatch::logmel_fft_kernel_clips, dim3(grid), dim3(256), mel::FFT_LDS_BYTES, st, audio, table, (const int32_t*)clip_first,
                           (const int32_t*)tiles_first, n_clips, tiles, (const float*)head, (const float*)tail, d_t1, d_t3, d_tm, features);
    }
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- live sessions (savad_live_plan.h: the host plan; savad_live.h: the kernels) ----------------------------------
namespace {

static_assert(sizeof(savad_live_slot) == sizeof(live::Slot) && sizeof(savad_live_push) == sizeof(live::Push), "live ABI structs");

int live_geometry(const savad_live_config* c, live::Geometry* g) {
    if (!c) return fail(SAVAD_E_INVALID, "null config");
    *g = live::geometry(c->streams, c->max_push_samples, c->half, c->jump);
    if (g->err) return fail(g->err, "%s", g->msg);
    if (c->chunk < 1) return fail(SAVAD_E_INVALID, "chunk=%d", c->chunk);
    return SAVAD_OK;
}

WindowOffsets live_offsets(const live::Geometry& g) {
    WindowOffsets wo;
    wo.w = g.W;
    for (int i = 0; i < g.W; ++i) wo.off[i] = g.off[i];
    return wo;
}

// geometry + both copies of a tick's table
int live_tables(const savad_live_config* c, const void* table_host, const void* table_dev, live::Geometry* g, const live::Header** h) {
    int rc = live_geometry(c, g);
    if (rc) return rc;
    if (!table_host || !table_dev) return fail(SAVAD_E_INVALID, "null table");
    const live::PlanResult r = live::check_table(*g, table_host, nullptr);
    if (r.err) return fail(r.err, "%s", r.msg);
    if ((uintptr_t)table_dev & 15) return fail(SAVAD_E_INVALID, "the device table must be 16-byte aligned");
    *h = live::header(table_host);
    return SAVAD_OK;
}

template <class T>
const T* live_at(const void* table_dev, int32_t offset) { return reinterpret_cast<const T*>(reinterpret_cast<const char*>(table_dev) + offset); }

// the tick's chunk and its workspace (savad_windows.h: layout; no table)
struct LiveWorkspace {
    int chunk;
    size_t fwd_bytes;
    windows::Layout at;
};
int live_workspace(savad_handle m, const live::Geometry& g, int chunk, long max_items, LiveWorkspace* w) {
    const int unit = live::chunk_items(g, 1);
    max_items = (max_items + unit - 1) / unit * unit;
    w->chunk = live::chunk_items(g, chunk);
    if (w->chunk > max_items) w->chunk = (int)(max_items > unit ? max_items : unit);
    if (m->cfg.feature_size != g.F) return fail(SAVAD_E_UNSUPPORTED, "the live mode runs the shipped %d-mel front-end; the model takes %d features", g.F, m->cfg.feature_size);
    int rc = savad_workspace_bytes(m, w->chunk, g.W, &w->fwd_bytes);
    if (rc) return rc;
    w->at = windows::layout(0, max_items, w->chunk, g.W, g.F, w->fwd_bytes);
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT long savad_live_ready_frames(long n_samples) { return n_samples < 0 ? fail(SAVAD_E_INVALID, "n_samples") : live::ready_frames(n_samples); }
SAVAD_EXPORT long savad_live_final_rows(long n_samples, int half) {
    return n_samples < 0 || half < 0 ? fail(SAVAD_E_INVALID, "bad argument") : live::final_rows(live::ready_frames(n_samples), half);
}
SAVAD_EXPORT int savad_live_state_bytes(const savad_live_config* config, size_t* bytes) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!bytes) return fail(SAVAD_E_INVALID, "null argument");
    *bytes = g.state_bytes();
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_table_bytes(const savad_live_config* config, int max_pushes, size_t* bytes) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!bytes || max_pushes < 0 || max_pushes > g.streams) return fail(SAVAD_E_INVALID, "max_pushes=%d of %d streams", max_pushes, g.streams);
    *bytes = live::table_bytes(g, max_pushes);
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_max_rows(const savad_live_config* config, int* rows_per_stream) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!rows_per_stream) return fail(SAVAD_E_INVALID, "null argument");
    *rows_per_stream = g.max_rows;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_workspace_bytes(savad_handle m, const savad_live_config* config, int max_pushes, size_t* bytes) {
    if (!m || !bytes) return fail(SAVAD_E_INVALID, "null argument");
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (max_pushes < 0 || max_pushes > g.streams) return fail(SAVAD_E_INVALID, "max_pushes=%d of %d streams", max_pushes, g.streams);
    LiveWorkspace w;
    if (int rc = live_workspace(m, g, config->chunk, (long)max_pushes * g.max_items(), &w)) return rc;
    *bytes = w.at.total;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_open(const savad_live_config* config, savad_live_slot* slots, int slot) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!slots || slot < 0 || slot >= g.streams) return fail(SAVAD_E_INVALID, "slot %d of %d", slot, g.streams);
    if (slots[slot].open) return fail(SAVAD_E_INVALID, "slot %d is open", slot);
    slots[slot] = savad_live_slot{0, 0, 1, 0};
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_plan(const savad_live_config* config, const savad_live_slot* slots, const savad_live_push* pushes, int n_pushes,
                                 const void* state, void* table_host, size_t table_bytes, savad_live_counts* counts, int64_t* rows) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!slots || !table_host || !counts) return fail(SAVAD_E_INVALID, "null table, slots or counts");
    if ((uintptr_t)state & 15) return fail(SAVAD_E_INVALID, "the state must be 16-byte aligned");
    const live::PlanResult r = live::plan_tick(g, reinterpret_cast<const live::Slot*>(slots), reinterpret_cast<const live::Push*>(pushes), n_pushes,
                                               (uint64_t)(uintptr_t)state, table_host, table_bytes, rows);
    if (r.err) return fail(r.err, "%s", r.msg);
    const live::Header* h = live::header(table_host);
    *counts = savad_live_counts{h->n_entries, h->n_tiles, h->n_items, h->n_rows, h->total, g.W};
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_append(const savad_live_config* config, const void* table_host, const void* table_dev, void* stream) {
    live::Geometry g;
    const live::Header* h;
    if (int rc = live_tables(config, table_host, table_dev, &g, &h)) return rc;
    if (h->n_entries == 0) return SAVAD_OK;
    const int bx = (h->max_append + live::HEAD_FLOATS + live::TAIL_FLOATS + 255) / 256;
    hipLaunchKernelGGL(live::append_kernel, dim3(bx < 64 ? bx : 64, h->n_entries < 32768 ? h->n_entries : 32768), dim3(256), 0,
                       (hipStream_t)stream, live_at<live::Entry>(table_dev, h->o_entries), h->n_entries);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_logmel(const savad_live_config* config, const void* table_host, const void* table_dev, void* stream) {
    live::Geometry g;
    const live::Header* h;
    if (int rc = live_tables(config, table_host, table_dev, &g, &h)) return rc;
    if (h->n_tiles == 0) return SAVAD_OK;
    int rc, n_cu;
    MelTables::Ptrs tb;
    if ((rc = mel_tables(&tb, &n_cu))) return rc;
    const int grid = h->n_tiles < n_cu ? h->n_tiles : n_cu;
    hipLaunchKernelGGL(live::logmel_fft_kernel_table, dim3(grid), dim3(256), mel::FFT_LDS_BYTES, (hipStream_t)stream,
                       live_at<live::Tile>(table_dev, h->o_tiles), h->n_tiles, (const float*)std::get<2>(tb), (const float*)std::get<3>(tb),
                       (const float*)std::get<4>(tb));
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_gather(const savad_live_config* config, const void* table_host, const void* table_dev, int first, int count,
                                   float* windows, void* stream) {
    live::Geometry g;
    const live::Header* h;
    if (int rc = live_tables(config, table_host, table_dev, &g, &h)) return rc;
    if (first < 0 || count < 0 || (long)first + count > h->n_items)
        return fail(SAVAD_E_INVALID, "items [%d,%ld) reach outside the %d items of the tick", first, (long)first + count, h->n_items);
    if (count == 0) return SAVAD_OK;
    if (!windows || ((uintptr_t)windows & 15)) return fail(SAVAD_E_INVALID, "windows must be a 16-byte aligned pointer");
    hipLaunchKernelGGL(live::gather_items_kernel, dim3(grid_for((long)count * g.W * (g.F / 4), 2048)), dim3(256), 0, (hipStream_t)stream,
                       live_at<live::Entry>(table_dev, h->o_entries), live_at<live::Item>(table_dev, h->o_items), g.F, g.feat_cap, first, count,
                       live_offsets(g), windows);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_boost(const savad_live_config* config, const void* table_host, const void* table_dev, const float* logp,
                                  float* probs, float* mean, void* stream) {
    live::Geometry g;
    const live::Header* h;
    if (int rc = live_tables(config, table_host, table_dev, &g, &h)) return rc;
    if (h->n_rows == 0) return SAVAD_OK;
    if (!probs || (h->n_items > 0 && !logp)) return fail(SAVAD_E_INVALID, "null pointer");
    hipLaunchKernelGGL(live::boost_history_kernel, dim3(grid_for(h->n_rows, 2048)), dim3(256), 0, (hipStream_t)stream,
                       live_at<live::Entry>(table_dev, h->o_entries), live_at<int32_t>(table_dev, h->o_rows), h->n_entries, h->n_rows, logp, g.half,
                       g.logp_cap, live_offsets(g), probs, mean);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_commit(const savad_live_config* config, const void* table_host, savad_live_slot* slots) {
    live::Geometry g;
    if (int rc = live_geometry(config, &g)) return rc;
    if (!slots) return fail(SAVAD_E_INVALID, "null slots");
    const live::PlanResult r = live::check_table(g, table_host, reinterpret_cast<const live::Slot*>(slots));
    if (r.err) return fail(r.err, "%s", r.msg);
    live::commit(table_host, reinterpret_cast<live::Slot*>(slots));
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_step(savad_handle m, const savad_live_config* config, savad_live_slot* slots, const void* table_host,
                                 const void* table_dev, float* probs, float* mean, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m) return fail(SAVAD_E_INVALID, "null handle");
    live::Geometry g;
    const live::Header* h;
    if (int rc = live_tables(config, table_host, table_dev, &g, &h)) return rc;
    if (!slots) return fail(SAVAD_E_INVALID, "null slots");
    const live::PlanResult r = live::check_table(g, table_host, reinterpret_cast<const live::Slot*>(slots));
    if (r.err) return fail(r.err, "%s", r.msg);
    LiveWorkspace w{};
    if (h->n_items > 0) {
        if (int rc = live_workspace(m, g, config->chunk, h->n_items, &w)) return rc;
        if (!workspace || ((uintptr_t)workspace & 15)) return fail(SAVAD_E_INVALID, "workspace must be a 16-byte aligned pointer");
        if (workspace_bytes < w.at.total) return fail(SAVAD_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, w.at.total);
    }
    if (h->n_rows > 0 && !probs) return fail(SAVAD_E_INVALID, "null output");
    int rc;
    if ((rc = savad_live_append(config, table_host, table_dev, stream))) return rc;
    if ((rc = savad_live_logmel(config, table_host, table_dev, stream))) return rc;
    char* ws = (char*)workspace;
    float* logp = h->n_items > 0 ? (float*)(ws + w.at.logp) : nullptr;
    float* win = (float*)(ws + w.at.windows);
    rc = forward_chunks(m, h->n_items, w.chunk, g.W, win, logp, ws + w.at.fwd, w.fwd_bytes, stream, [&](int first, int count) {
        return savad_live_gather(config, table_host, table_dev, first, count, win, stream);
    });
    if (rc) return rc;
    if ((rc = savad_live_boost(config, table_host, table_dev, logp, probs, mean, stream))) return rc;
    live::commit(table_host, reinterpret_cast<live::Slot*>(slots));
    return SAVAD_OK;
}

// ---- live sessions: events as they become final (savad_live_post.h) -----------------------------------------------
namespace {

namespace lp = savad::livepost;

static_assert(sizeof(savad_live_event) == sizeof(lp::Event), "live event ABI");

int live_post_params(const savad_live_post_config* c, lp::Params* p) {
    if (!c) return fail(SAVAD_E_INVALID, "null post config");
    if (c->W < 1 || c->W > postdev::W_MAX) return fail(SAVAD_E_INVALID, "W = %d: the row mean has numpy's order for 1 .. %d", c->W, postdev::W_MAX);
    if (c->min_vally < 0 || c->min_hill < 0 || c->hang_before < 0 || c->hang_over < 0)
        return fail(SAVAD_E_INVALID, "negative trim parameter (%d, %d, %d, %d)", c->min_vally, c->min_hill, c->hang_before, c->hang_over);
    if (!(c->threshold == c->threshold)) return fail(SAVAD_E_INVALID, "threshold is NaN");
    *p = lp::Params{c->W, c->threshold, c->min_vally, c->min_hill, c->hang_before, c->hang_over};
    return SAVAD_OK;
}

// events [offsets entries + 1 | counts entries | events cap]; workspace [counts entries | raw entries x cap_max]
struct LivePostLayout {
    size_t ev_counts, ev_events, ev_total, ws_raw, ws_total;
    long events_cap;
    int cap_max;
};
int live_post_layout(const live::Geometry& g, const live::Header* h, const void* table_host, const lp::Params& p, LivePostLayout* L) {
    const live::Entry* e = live::entries(table_host);
    long total = 0;
    int cap_max = 0;
    for (int i = 0; i < h->n_entries; ++i) {
        if (e[i].row_count < 0 || e[i].row_out < 0 || (long)e[i].row_out + e[i].row_count > h->n_rows)
            return fail(SAVAD_E_INVALID, "entry %d names rows [%d, +%d) of %d", i, e[i].row_out, e[i].row_count, h->n_rows);
        if (e[i].slot < 0 || e[i].slot >= g.streams) return fail(SAVAD_E_INVALID, "entry %d names slot %d of %d", i, e[i].slot, g.streams);
        const int cap = lp::event_cap(e[i].row_count, p);
        total += cap;
        cap_max = cap > cap_max ? cap : cap_max;
    }
    const size_t n = (size_t)h->n_entries;
    L->ev_counts = sizeof(int32_t) * (n + 1);
    L->ev_events = live::up16(sizeof(int32_t) * (2 * n + 1));
    L->ev_total = L->ev_events + sizeof(lp::Event) * (size_t)total;
    L->ws_raw = live::up16(sizeof(int32_t) * n);
    L->ws_total = L->ws_raw + sizeof(lp::Event) * n * (size_t)cap_max;
    L->events_cap = total;
    L->cap_max = cap_max;
    return SAVAD_OK;
}

// config, post config and the host table -> geometry, parameters, layout
int live_post_plan(const savad_live_config* config, const savad_live_post_config* post, const void* table_host, live::Geometry* g,
                   const live::Header** h, lp::Params* p, LivePostLayout* L) {
    int rc;
    if ((rc = live_geometry(config, g))) return rc;
    if ((rc = live_post_params(post, p))) return rc;
    if (!table_host) return fail(SAVAD_E_INVALID, "null table");
    const live::PlanResult r = live::check_table(*g, table_host, nullptr);
    if (r.err) return fail(r.err, "%s", r.msg);
    *h = live::header(table_host);
    return live_post_layout(*g, *h, table_host, *p, L);
}

}  // namespace

SAVAD_EXPORT int savad_live_post_state_bytes(const savad_live_post_config* post, int streams, size_t* bytes) {
    lp::Params p;
    if (int rc = live_post_params(post, &p)) return rc;
    if (!bytes || streams < 1) return fail(SAVAD_E_INVALID, "streams = %d", streams);
    *bytes = sizeof(lp::State) * (size_t)streams;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_post_event_bytes(const savad_live_config* config, const savad_live_post_config* post, const void* table_host,
                                             size_t* bytes, size_t* events_offset) {
    live::Geometry g;
    const live::Header* h;
    lp::Params p;
    LivePostLayout L;
    if (int rc = live_post_plan(config, post, table_host, &g, &h, &p, &L)) return rc;
    if (!bytes) return fail(SAVAD_E_INVALID, "null argument");
    *bytes = L.ev_total;
    if (events_offset) *events_offset = L.ev_events;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_live_post_workspace_bytes(const savad_live_config* config, const savad_live_post_config* post, const void* table_host,
                                                 size_t* bytes) {
    live::Geometry g;
    const live::Header* h;
    lp::Params p;
    LivePostLayout L;
    if (int rc = live_post_plan(config, post, table_host, &g, &h, &p, &L)) return rc;
    if (!bytes) return fail(SAVAD_E_INVALID, "null argument");
    *bytes = L.ws_total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_post(const savad_live_config* config, const savad_live_post_config* post, const void* table_host,
                                 const void* table_dev, const float* probs, void* post_state, void* events, size_t events_bytes, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    live::Geometry g;
    const live::Header* h;
    lp::Params p;
    LivePostLayout L;
    if (int rc = live_post_plan(config, post, table_host, &g, &h, &p, &L)) return rc;
    if (p.W != g.W) return fail(SAVAD_E_INVALID, "the post config has W = %d, the window geometry %d", p.W, g.W);
    if (!table_dev || ((uintptr_t)table_dev & 15)) return fail(SAVAD_E_INVALID, "null table, or a device table that is not 16-byte aligned");
    if (!post_state || !events || !workspace || (h->n_rows > 0 && !probs)) return fail(SAVAD_E_INVALID, "null pointer");
    if (((uintptr_t)post_state & 15) || ((uintptr_t)events & 15) || ((uintptr_t)workspace & 15))
        return fail(SAVAD_E_INVALID, "post state, events and workspace must be 16-byte aligned");
    if (events_bytes < L.ev_total) return fail(SAVAD_E_INVALID, "event buffer too small for the tick: %zu < %zu bytes", events_bytes, L.ev_total);
    if (workspace_bytes < L.ws_total) return fail(SAVAD_E_INVALID, "workspace too small: %zu < %zu bytes", workspace_bytes, L.ws_total);
    char* ev = (char*)events;
    char* ws = (char*)workspace;
    int32_t* counts = (int32_t*)ws;
    lp::Event* raw = (lp::Event*)(ws + L.ws_raw);
    if (h->n_entries > 0) {
        hipLaunchKernelGGL(lp::post_kernel, dim3(h->n_entries < 65536 ? h->n_entries : 65536), dim3(64), 0, (hipStream_t)stream,
                           live_at<live::Entry>(table_dev, h->o_entries), h->n_entries, g.streams, probs, p, (lp::State*)post_state, raw, L.cap_max,
                           counts);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(lp::compact_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const lp::Event*)raw, L.cap_max, (const int32_t*)counts,
                       h->n_entries, (int32_t*)ev, (int32_t*)(ev + L.ev_counts), (lp::Event*)(ev + L.ev_events), L.events_cap);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_live_post_host(const savad_live_post_config* post, void* state, int slot, int64_t row_first, int row_count, int finish,
                                      const float* probs, savad_live_event* events, int cap, int* count) {
    lp::Params p;
    if (int rc = live_post_params(post, &p)) return rc;
    if (!state || !count || row_count < 0 || cap < 0) return fail(SAVAD_E_INVALID, "null state or count, or a negative count");
    if ((row_count > 0 && !probs) || (cap > 0 && !events)) return fail(SAVAD_E_INVALID, "null pointer");
    *count = lp::run_host((lp::State*)state, p, slot, row_first, row_count, finish, probs, (lp::Event*)events, cap);
    return SAVAD_OK;
}

// ---- feature front-end for any transform config (savad_frontend.h) ----------------------------------------------
namespace {

int fe_check(const savad_frontend_config* c) {
    if (!c) return fail(SAVAD_E_INVALID, "null config");
    if (c->transform < SAVAD_FE_SPECTROGRAM || c->transform > SAVAD_FE_MFCC) return fail(SAVAD_E_UNSUPPORTED, "unsupported transform %d", c->transform);
    if (c->win < 1 || c->hop < 1) return fail(SAVAD_E_INVALID, "window %d and hop %d must be >= 1", c->win, c->hop);
    if (c->n_fft < c->win || c->n_fft < 2 || c->n_fft > 2048) return fail(SAVAD_E_INVALID, "n_fft %d outside the limit win (%d) <= n_fft <= 2048", c->n_fft, c->win);
    if (c->transform != SAVAD_FE_SPECTROGRAM && (c->n_mels < 1 || c->n_mels > 256))
        return fail(SAVAD_E_INVALID, "n_mels %d outside the limit 1 <= n_mels <= 256", c->n_mels);
    if (c->transform == SAVAD_FE_MFCC && (c->n_mfcc < 1 || c->n_mfcc > c->n_mels))
        return fail(SAVAD_E_INVALID, "n_mfcc %d outside the limit 1 <= n_mfcc <= n_mels (%d)", c->n_mfcc, c->n_mels);
    if (c->deltas != 0 && c->deltas != 1) return fail(SAVAD_E_INVALID, "deltas must be 0 or 1");
    return SAVAD_OK;
}

// frames and features of a call (fe::shape); errors name the limit that was not met
int fe_shape(const savad_frontend_config* c, long n, int* frames, int* feats) {
    int rc;
    if ((rc = fe_check(c))) return rc;
    const fe::Shape s = fe::shape(*c, n);
    if (n < s.need || n > 2000000000L)
        return fail(SAVAD_E_INVALID, "%ld samples: the limit is n_samples >= %ld (%s)", n, s.need,
                    c->transform != SAVAD_FE_SPECTROGRAM ? "n_fft / 2 + 1, reflect padding" : "n_fft, center=False");
    if (c->deltas && s.frames < fe::DELTA_W)
        return fail(SAVAD_E_INVALID, "%ld frames: temporal differences need at least %d (librosa.feature.delta, width 9)", s.frames, fe::DELTA_W);
    *frames = (int)s.frames;
    *feats = s.feats;
    return SAVAD_OK;
}

// stft_kernel's A fragments | mel [n_mels][nb] | DCT [n_mfcc][n_mels] | Savitzky-Golay [2][9][9], under what of the config
// they depend on: (spectrogram or not, n_fft, win, n_mels, n_mfcc)
using FeTables = DeviceTables<std::tuple<int, int, int, int, int>, float, float, float, float>;
int fe_tables(const savad_frontend_config* c, FeTables::Ptrs* t) {
    const bool sp = c->transform == SAVAD_FE_SPECTROGRAM, mf = c->transform == SAVAD_FE_MFCC;
    int n_cu;
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    return FeTables::get({sp ? 0 : 1, c->n_fft, c->win, sp ? 0 : c->n_mels, mf ? c->n_mfcc : 0}, [c](FeTables::Host& h) {
        auto& [dft, melw, dct, sg] = h;
        dft = fe::dft_fragments(fe::geometry(*c), fe::host_table(*c, 0));
        melw = fe::host_table(*c, 1);
        dct = fe::host_table(*c, 2);
        sg = fe::host_table(*c, 3);
        return (int)SAVAD_OK;
    }, t, &n_cu);
}

}  // namespace

SAVAD_EXPORT int savad_frontend_shape(const savad_frontend_config* config, long n_samples, int* n_frames, int* n_features) {
    if (!n_frames || !n_features) return fail(SAVAD_E_INVALID, "null argument");
    return fe_shape(config, n_samples, n_frames, n_features);
}
SAVAD_EXPORT int savad_frontend_workspace_bytes(const savad_frontend_config* config, long n_samples, size_t* bytes) {
    int N, F, rc;
    if (!bytes) return fail(SAVAD_E_INVALID, "null argument");
    if ((rc = fe_shape(config, n_samples, &N, &F))) return rc;
    *bytes = fe::workspace(*config, n_samples, N).total;
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_frontend_prepare(const savad_frontend_config* config) {
    int rc;
    FeTables::Ptrs t;
    if ((rc = fe_check(config))) return rc;
    return fe_tables(config, &t);
}
SAVAD_EXPORT int savad_frontend_table_floats(const savad_frontend_config* config, int which) {
    int rc;
    if ((rc = fe_check(config))) return rc;
    if (which < 0 || which > 3) return fail(SAVAD_E_INVALID, "table %d (0 = DFT, 1 = mel, 2 = DCT, 3 = Savitzky-Golay)", which);
    return (int)fe::host_table(*config, which).size();
}
SAVAD_EXPORT int savad_frontend_tables_host(const savad_frontend_config* config, int which, float* out) {
    int rc;
    if ((rc = fe_check(config))) return rc;
    if (!out || which < 0 || which > 3) return fail(SAVAD_E_INVALID, "table %d / null output", which);
    const std::vector<float> t = fe::host_table(*config, which);
    if (!t.empty()) memcpy(out, t.data(), t.size() * sizeof(float));
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_frontend(const savad_frontend_config* config, const float* audio, long n_samples, float* workspace, float* features,
                                void* stream) {
    using namespace savad::fe;
    int N, Fo, rc;
    if ((rc = fe_shape(config, n_samples, &N, &Fo))) return rc;
    if (!audio || !workspace || !features) return fail(SAVAD_E_INVALID, "null argument");
    if (!aligned16(workspace, features)) return fail(SAVAD_E_INVALID, "workspace and features must be 16-byte aligned");
    FeTables::Ptrs tb;
    if ((rc = fe_tables(config, &tb))) return rc;
    const auto [d_dft, d_mel, d_dct, d_sg] = tb;
    hipStream_t st = (hipStream_t)stream;
    const savad_frontend_config& c = *config;
    const Geo g = geometry(c);
    const fe::Workspace w = fe::workspace(c, n_samples, N);
    const bool sp = c.transform == SAVAD_FE_SPECTROGRAM, mf = c.transform == SAVAD_FE_MFCC;
    const int F = c.deltas ? Fo / 3 : Fo;
    int* gmax = reinterpret_cast<int*>(at(workspace, w.gmax));
    float *sig = at(workspace, w.sig), *spec = at(workspace, w.spec), *db = at(workspace, w.db);
    const float* src;
    if (!sp) {  // centred: the reflect-padded signal, always materialised (aligned whatever the audio pointer)
        const long total = n_samples + c.n_fft + SLACK;
        hipLaunchKernelGGL(fe_reflect_pad_kernel, dim3(grid_for(total)), dim3(256), 0, st, audio, n_samples, c.n_fft / 2, total, sig);
        src = sig;
    } else {  // straight from the audio when every 16-byte read lands inside it; otherwise from an aligned copy (same values)
        const bool aligned = ((uintptr_t)audio & 15) == 0 || (g.hop & 3);
        if (aligned && (long)g.hop * (N - 1) + g.k0 + g.kr <= n_samples) {
            src = audio;
        } else {
            const long total = n_samples + SLACK;
            hipLaunchKernelGGL(fe_copy_kernel, dim3(grid_for(total)), dim3(256), 0, st, audio, n_samples, total, sig);
            src = sig;
        }
    }
    const StftArgs a{src + g.k0, d_dft, sp ? features : spec, mf ? gmax : nullptr, N, g.hop, g.kg, g.rblocks, g.nb, g.n_fft, sp ? Fo : g.nbs, sp};
    const int wgs = (N + 32 * FT - 1) / (32 * FT);
    hipLaunchKernelGGL((g.hop % 4 == 0 ? stft_kernel<true> : stft_kernel<false>), dim3(wgs), dim3(256), 0, st, a);
    if (!sp) {
        FeGemm m{spec, (long)g.nbs, d_mel, mf ? db : features, mf ? (long)c.n_mels : (long)Fo, N, c.n_mels, g.nb, gmax};
        const dim3 gm((c.n_mels + GT - 1) / GT, (N + GT - 1) / GT);
        if (c.transform == SAVAD_FE_MEL)
            hipLaunchKernelGGL((fe_gemm_kernel<EPI_NONE, false>), gm, dim3(256), 0, st, m);
        else if (c.transform == SAVAD_FE_LOGMEL)
            hipLaunchKernelGGL((fe_gemm_kernel<EPI_LOG, false>), gm, dim3(256), 0, st, m);
        else {
            hipLaunchKernelGGL((fe_gemm_kernel<EPI_DB, false>), gm, dim3(256), 0, st, m);
            FeGemm d{db, (long)c.n_mels, d_dct, features, (long)Fo, N, c.n_mfcc, c.n_mels, gmax};
            hipLaunchKernelGGL((fe_gemm_kernel<EPI_NONE, true>), dim3((c.n_mfcc + GT - 1) / GT, (N + GT - 1) / GT), dim3(256), 0, st, d);
        }
    }
    if (c.deltas) hipLaunchKernelGGL(delta_kernel, dim3(grid_for((long)N * F)), dim3(256), 0, st, features, N, F, (long)Fo, d_sg);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// ---- audio ingest: channel average and resampling to 16 kHz on the device (savad_ingest.h) ----------------------------------
namespace {

struct RsHost {   // per source rate, host side: the plan and the time segments
    ingest::Plan plan;
    std::vector<ingest::Seg> segs;
    long long k_end = 0;
};
std::vector<double> g_rs_window;            // the caller's "kaiser_fast" half window (savad_resample_set_window)
std::map<int, RsHost> g_rs_host;            // rate -> host tables; process lifetime
int g_rs_table_mode = 0;                    // 0 = table in LDS, 1 = through the cache
using RsTables = DeviceTables<int, double2, ingest::Seg>;   // rate -> (win, delta) pairs | time segments

int rs_check_rate(int rate) {
    if (rate < ingest::RATE_MIN || rate > ingest::RATE_MAX)
        return fail(SAVAD_E_UNSUPPORTED, "source rate %d Hz outside the limit %d <= rate <= %d", rate, ingest::RATE_MIN, ingest::RATE_MAX);
    return SAVAD_OK;
}

// A rate's plan and time segments need no window: the host-only helpers (length, span samples, segments) work without one.
// The caller holds g_audio_mutex.
int rs_host(int rate, const RsHost** out) {
    namespace in = savad::ingest;
    int rc;
    if ((rc = rs_check_rate(rate))) return rc;
    auto it = g_rs_host.find(rate);
    if (it == g_rs_host.end()) {
        RsHost h;
        h.plan = in::plan_for(rate);
        h.segs = in::time_segments(h.plan.inc, &h.k_end);
        if (h.segs.empty()) return fail(SAVAD_E_UNSUPPORTED, "source rate %d Hz: its time register needs more than %d segments", rate, in::MAX_SEGS);
        if (in::lds_bytes(h.plan, true) > (size_t)in::LDS_BYTES_MAX)
            return fail(SAVAD_E_UNSUPPORTED, "source rate %d Hz: a block's input span does not fit the LDS next to the table", rate);
        it = g_rs_host.emplace(rate, std::move(h)).first;
    }
    *out = &it->second;
    return SAVAD_OK;
}

// the caller's window as the rate's kernel reads it (ingest::scaled_window), while g_audio_mutex is held
int rs_window(const RsHost& h, std::vector<double>& win, std::vector<double>& delta) {
    if (g_rs_window.empty()) return fail(SAVAD_E_STATE, "the kaiser_fast half window was never set (savad_resample_set_window)");
    ingest::scaled_window(h.plan, g_rs_window, win, delta);
    return SAVAD_OK;
}

// the rate's tables on the current device (the caller holds g_audio_mutex)
int rs_tables(int rate, const RsHost& h, RsTables::Ptrs* t, int* n_cu) {
    return RsTables::get(rate, [&h](RsTables::Host& up) {
        auto& [tab, segs] = up;
        std::vector<double> win, delta;
        if (int rc = rs_window(h, win, delta)) return rc;
        for (int i = 0; i < ingest::NWIN; ++i) tab.push_back(double2{win[i], delta[i]});
        segs = h.segs;
        return (int)SAVAD_OK;
    }, t, n_cu);
}

long rs_n_out(const savad::ingest::Plan& p, long n) { return (long)((double)n * p.ratio); }          // int(n * ratio)
long rs_n_fix(const savad::ingest::Plan& p, long n) { return (long)ceil((double)n * p.ratio); }     // ceil(n * ratio)

// savad_resample_span_samples for a rate other than 16 kHz
int rs_span_samples(const RsHost& h, long n_samples, long out_first, long out_count, long* first, long* count) {
    const long n_fix = rs_n_fix(h.plan, n_samples), n_out = rs_n_out(h.plan, n_samples);
    if (out_first + out_count > n_fix) return fail(SAVAD_E_INVALID, "output span [%ld, +%ld) of %ld", out_first, out_count, n_fix);
    if (n_out > h.k_end) return fail(SAVAD_E_UNSUPPORTED, "%ld samples: beyond the time-register table", n_samples);
    const long o1 = out_first + out_count < n_out ? out_first + out_count : n_out;
    long long a = 0, c = 0;   // nothing but fix_length's zeros (or an empty span): no input is read
    if (o1 > out_first) savad::ingest::span_inputs(h.plan, h.segs, n_samples, out_first, o1, &a, &c);
    *first = (long)a;
    *count = (long)c;
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT long savad_resample_length(long n_samples, int rate) {
    if (n_samples < 0) return fail(SAVAD_E_INVALID, "n_samples %ld", n_samples);
    if (rate == savad::ingest::TARGET) return n_samples;
    int rc;
    if ((rc = rs_check_rate(rate))) return rc;
    return rs_n_fix(savad::ingest::plan_for(rate), n_samples);
}

SAVAD_EXPORT int savad_resample_set_window(const double* half_window) {
    if (!half_window) return fail(SAVAD_E_INVALID, "null window");
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    if (!g_rs_window.empty()) {
        if (memcmp(g_rs_window.data(), half_window, sizeof(double) * savad::ingest::NWIN) == 0) return SAVAD_OK;
        return fail(SAVAD_E_STATE, "a different half window is already set (tables built from it may be on a device)");
    }
    g_rs_window.assign(half_window, half_window + savad::ingest::NWIN);
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_resample_prepare(int rate) {
    if (rate == savad::ingest::TARGET) return SAVAD_OK;
    const RsHost* h;
    RsTables::Ptrs t;
    int rc, n_cu;
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    if ((rc = rs_host(rate, &h))) return rc;
    return rs_tables(rate, *h, &t, &n_cu);
}

SAVAD_EXPORT int savad_resample_set_table_mode(int mode) {
    if (mode < 0 || mode > 1) return fail(SAVAD_E_INVALID, "table mode %d (0 = LDS, 1 = through the cache)", mode);
    g_rs_table_mode = mode;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_resample_table_host(int rate, double* window, double* delta) {
    const RsHost* h;
    std::vector<double> win, dlt;
    int rc;
    if (!window) return fail(SAVAD_E_INVALID, "null output");
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    if ((rc = rs_host(rate, &h)) || (rc = rs_window(*h, win, dlt))) return rc;
    memcpy(window, win.data(), sizeof(double) * savad::ingest::NWIN);
    if (delta) memcpy(delta, dlt.data(), sizeof(double) * savad::ingest::NWIN);
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_resample_segments_host(int rate, int max, long* first, double* time, double* step, long* covered) {
    const RsHost* h;
    int rc;
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    if ((rc = rs_host(rate, &h))) return rc;
    const int n = (int)h->segs.size();
    if (covered) *covered = (long)h->k_end;
    if (max > 0 && (!first || !time || !step)) return fail(SAVAD_E_INVALID, "null output");
    for (int i = 0; i < n && i < max; ++i) {
        first[i] = (long)h->segs[i].k0;
        time[i] = h->segs[i].t0;
        step[i] = h->segs[i].s;
    }
    return n;
}

SAVAD_EXPORT int savad_resample_span_samples(long n_samples, int rate, long out_first, long out_count, long* first, long* count) {
    if (!first || !count || n_samples < 0 || out_first < 0 || out_count < 0) return fail(SAVAD_E_INVALID, "bad argument");
    if (rate == savad::ingest::TARGET) {
        if (out_first + out_count > n_samples) return fail(SAVAD_E_INVALID, "output span [%ld, +%ld) of %ld", out_first, out_count, n_samples);
        *first = out_first / 4 * 4;
        *count = out_first + out_count - *first;
        return SAVAD_OK;
    }
    const RsHost* h;
    int rc;
    std::lock_guard<std::mutex> lock(g_audio_mutex);
    if ((rc = rs_host(rate, &h))) return rc;
    return rs_span_samples(*h, n_samples, out_first, out_count, first, count);
}

SAVAD_EXPORT int savad_resample_span(const float* audio, long audio_first, long audio_count, long n_samples, int rate, long out_first,
                                     long out_count, float* out, void* stream) {
    namespace in = savad::ingest;
    hipStream_t st = (hipStream_t)stream;
    if (n_samples < 0 || audio_first < 0 || audio_count < 0 || audio_first + audio_count > n_samples || out_first < 0 || out_count < 0)
        return fail(SAVAD_E_INVALID, "bad argument");
    if (out_count == 0) return SAVAD_OK;
    if (!out || (audio_count > 0 && !audio)) return fail(SAVAD_E_INVALID, "null pointer");
    long need_first, need_count;
    int rc, n_cu;
    if (rate == in::TARGET) {   // a 16 kHz source is a plain copy
        if ((rc = savad_resample_span_samples(n_samples, rate, out_first, out_count, &need_first, &need_count))) return rc;
        if (out_first < audio_first || out_first + out_count > audio_first + audio_count)
            return fail(SAVAD_E_INVALID, "the slice [%ld, +%ld) does not hold samples [%ld, +%ld)", audio_first, audio_count, out_first, out_count);
        HIP_TRY(hipMemcpyAsync(out, audio + (out_first - audio_first), sizeof(float) * (size_t)out_count, hipMemcpyDeviceToDevice, st));
        return SAVAD_OK;
    }
    const RsHost* h;
    RsTables::Ptrs tb;
    {
        std::lock_guard<std::mutex> lock(g_audio_mutex);
        if ((rc = rs_host(rate, &h)) || (rc = rs_span_samples(*h, n_samples, out_first, out_count, &need_first, &need_count))) return rc;
        if (need_count > 0) {   // (the slice may start after the aligned *first, as long as it holds every sample that is read)
            long lo = (long)in::time_at(h->segs, out_first) - h->plan.taps + 1;
            if (lo < 0) lo = 0;
            if (audio_first > lo || audio_first + audio_count < need_first + need_count)
                return fail(SAVAD_E_INVALID, "the slice [%ld, +%ld) does not hold the samples outputs [%ld, +%ld) read: [%ld, +%ld) (savad_resample_span_samples)",
                            audio_first, audio_count, out_first, out_count, need_first, need_count);
        }
        if ((rc = rs_tables(rate, *h, &tb, &n_cu))) return rc;
    }
    const auto [d_tab, d_segs] = tb;
    const bool in_lds = g_rs_table_mode == 0;
    const long blocks = (out_count + in::BLOCK - 1) / in::BLOCK;
    const long cap = in_lds ? n_cu : 2L * n_cu;   // resident workgroups: one per CU around the table, two without it
    const int grid = (int)(blocks < cap ? blocks : cap);
    const size_t lds = in::lds_bytes(h->plan, in_lds);
    const long long n_out = rs_n_out(h->plan, n_samples);
    hipLaunchKernelGGL((in_lds ? in::resample_kernel<true> : in::resample_kernel<false>), dim3(grid), dim3(in::BLOCK), lds, st, audio,
                       (long long)audio_first, (long long)audio_count, (long long)n_samples, (long long)out_first, (long long)out_count, n_out,
                       d_tab, d_segs, (int)h->segs.size(), h->plan.scale, h->plan.step, h->plan.taps, h->plan.span, out);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_resample(const float* audio, long n_samples, int rate, float* out, void* stream) {
    const long n = savad_resample_length(n_samples, rate);
    if (n < 0) return (int)n;
    return savad_resample_span(audio, 0, n_samples, n_samples, rate, 0, n, out, stream);
}

SAVAD_EXPORT int savad_ingest_downmix(const void* raw, int dtype, int channels, long n_frames, float* mono, void* stream) {
    namespace in = savad::ingest;
    hipStream_t st = (hipStream_t)stream;
    if (dtype != SAVAD_PCM_INT16 && dtype != SAVAD_PCM_FLOAT32) return fail(SAVAD_E_INVALID, "dtype %d (0 = int16, 1 = float32)", dtype);
    if (channels < 1 || n_frames < 0) return fail(SAVAD_E_INVALID, "channels %d, frames %ld", channels, n_frames);
    if (dtype == SAVAD_PCM_INT16 && channels > 256)
        return fail(SAVAD_E_UNSUPPORTED, "%d channels of int16: the limit is 256 (partial sums stay exact in float32)", channels);
    if (dtype == SAVAD_PCM_FLOAT32 && channels > 7)
        return fail(SAVAD_E_UNSUPPORTED, "%d channels of float32: the limit is 7 (numpy's mean sums rows of 8 or more in another order)", channels);
    if (n_frames == 0) return SAVAD_OK;
    if (!raw || !mono) return fail(SAVAD_E_INVALID, "null pointer");
    if (((uintptr_t)raw & (dtype == SAVAD_PCM_INT16 ? 1 : 3)) || ((uintptr_t)mono & 3)) return fail(SAVAD_E_INVALID, "misaligned pointer");
    if (channels == 1 && dtype == SAVAD_PCM_INT16 && ((uintptr_t)mono & 15) == 0) return savad_pcm16_to_f32((const short*)raw, n_frames, mono, stream);
    if (channels == 1 && dtype == SAVAD_PCM_FLOAT32) {
        if (raw != (const void*)mono) HIP_TRY(hipMemcpyAsync(mono, raw, sizeof(float) * (size_t)n_frames, hipMemcpyDeviceToDevice, st));
        return SAVAD_OK;
    }
    const int grid = grid_for(n_frames);
    if (dtype == SAVAD_PCM_INT16)
        hipLaunchKernelGGL(in::downmix_kernel<short>, dim3(grid), dim3(256), 0, st, (const short*)raw, channels, (long long)n_frames, mono);
    else
        hipLaunchKernelGGL(in::downmix_kernel<float>, dim3(grid), dim3(256), 0, st, (const float*)raw, channels, (long long)n_frames, mono);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// What depends on the device alone, once per device: its compute units, and each LDS limit at its kernel's maximum.  (Down here: a
// kernel template's place in the code object follows its first mention in this file, and the launches above keep the kernels' order.)
namespace {
int audio_device(int dev, int* n_cu) {
    if ((size_t)dev >= g_audio_n_cu.size()) g_audio_n_cu.resize(dev + 1, 0);
    if (!g_audio_n_cu[dev]) {
        int rc, n = 0;
        HIP_TRY(hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev));
        if ((rc = allow_lds(mel::logmel_fft_kernel, mel::FFT_LDS_BYTES))) return rc;
        if ((rc = allow_lds(ingest::resample_kernel<true>, ingest::LDS_BYTES_MAX))) return rc;   // rs_host refuses a rate that needs more
        if ((rc = allow_lds(ingest::resample_kernel<false>, ingest::LDS_BYTES_MAX - ingest::NWIN * 16))) return rc;
        if ((rc = allow_lds(live::logmel_fft_kernel_table, mel::FFT_LDS_BYTES))) return rc;
        if ((rc = allow_lds(melbatch::logmel_fft_kernel_clips, mel::FFT_LDS_BYTES))) return rc;
        g_audio_n_cu[dev] = n;
    }
    *n_cu = g_audio_n_cu[dev];
    return SAVAD_OK;
}
}  // namespace

// ---- post-processing (host arrays; savad_post.h) ------------------------------------------------
SAVAD_EXPORT int savad_trim_voice_activity(const uint8_t* pred, int n, int min_vally, int min_hill, int hang_before,
                                           int hang_over, uint8_t* out) {
    if (n < 0 || (n > 0 && (!pred || !out))) return fail(SAVAD_E_INVALID, "bad argument");
    savad::post::trim_voice_activity(pred, n, min_vally, min_hill, hang_before, hang_over, out);
    return SAVAD_OK;
}
SAVAD_EXPORT long savad_frames_to_samples(const double* frames, int n, int sample_rate, double hop_ms, double window_ms,
                                          double* out) {
    if (n < 0 || (n > 0 && !frames)) return fail(SAVAD_E_INVALID, "bad argument");
    return savad::post::frames_to_samples(frames, n, sample_rate, hop_ms, window_ms, out);
}
SAVAD_EXPORT int savad_samples_to_segments(const double* samples, long n, long* starts, long* ends, int cap) {
    if (n < 0 || (n > 0 && !samples) || cap < 0) return fail(SAVAD_E_INVALID, "bad argument");
    return savad::post::samples_to_segments(samples, n, starts, ends, cap);
}
SAVAD_EXPORT int savad_optimal_split(const double* pred, const double* probs, long n, long max_samples, double* out) {
    if (n < 0 || (n > 0 && (!pred || !probs || !out)) || max_samples <= 1) return fail(SAVAD_E_INVALID, "bad argument");
    savad::post::optimal_split(pred, probs, n, max_samples, out);
    return SAVAD_OK;
}

// ---- post-processing on the device (savad_post_device.h) -----------------------------------------------------------------
namespace {

namespace pd = savad::postdev;

int g_post_block = 0;   // savad_post_set_block: elements per workgroup block of the scans (0 = the default)

int post_block() { return g_post_block ? g_post_block : pd::SCAN_BLOCK_DEFAULT; }

struct PostLayout {   // byte offsets into the caller's workspace
    size_t last, next, sums_f, frames_end;                                  // savad_post_frames: a function of n_frames alone
    size_t cls, state, sums_s, seg_starts, seg_ends, totals, partial, result, total;   // savad_post_segments
    long seg_cap;                                                           // slots of the segment (and break) buffers
};

PostLayout post_layout(int N, const pd::Geometry& g) {
    PostLayout L;
    Arena a;
    L.last = a.take(sizeof(int) * (size_t)N);
    L.next = a.take(sizeof(int) * (size_t)N);
    L.sums_f = a.take(sizeof(int) * (size_t)pd::scan_sums_elems(N));
    L.frames_end = a.off;
    L.seg_cap = (long)N + 2;   // without a split a segment needs a frame of its own
    L.cls = a.take((size_t)g.num);
    L.state = a.take((size_t)g.num);
    L.sums_s = a.take(sizeof(pd::Long2) * (size_t)pd::scan_sums_elems(g.num + 1));
    L.seg_starts = a.take(sizeof(long) * (size_t)L.seg_cap);
    L.seg_ends = a.take(sizeof(long) * (size_t)L.seg_cap);
    L.totals = a.take(sizeof(long) * 2);
    L.partial = a.take(sizeof(pd::MinKey) * pd::ARGMIN_GRID);
    L.result = a.take(sizeof(pd::MinKey));
    L.total = a.off;
    return L;
}

int post_check_trim(int min_vally, int min_hill, int hang_before, int hang_over) {
    if (min_vally < 0 || min_hill < 0 || hang_before < 0 || hang_over < 0)
        return fail(SAVAD_E_INVALID, "negative trim parameter (%d, %d, %d, %d)", min_vally, min_hill, hang_before, hang_over);
    return SAVAD_OK;
}

int post_check_geometry(int sample_rate, double hop_ms, double window_ms, int n_frames) {
    if (!pd::geometry_supported(sample_rate, hop_ms, window_ms, n_frames))
        return fail(SAVAD_E_UNSUPPORTED, "geometry (%d Hz, hop %g ms, window %g ms, %d frames): the device post-processing needs a hop of a whole "
                    "number of samples >= 1 and (n-1)*hop + window < 2^52", sample_rate, hop_ms, window_ms, n_frames);
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT int savad_post_supported(int W, int sample_rate, double hop_ms, double window_ms, int n_frames) {
    return W >= 1 && W <= pd::W_MAX && pd::geometry_supported(sample_rate, hop_ms, window_ms, n_frames) ? 1 : 0;
}

SAVAD_EXPORT int savad_post_set_block(int elems) {
    if (elems != 0 && (elems < pd::SCAN_BLOCK_MIN || elems > pd::SCAN_BLOCK_DEFAULT || (elems & (elems - 1))))
        return fail(SAVAD_E_INVALID, "scan block %d (0 = default, or a power of two from %d to %d)", elems, pd::SCAN_BLOCK_MIN, pd::SCAN_BLOCK_DEFAULT);
    g_post_block = elems;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_workspace_bytes(int n_frames, int W, int sample_rate, double hop_ms, double window_ms, size_t* bytes) {
    if (!bytes || n_frames < 0 || W < 1) return fail(SAVAD_E_INVALID, "bad argument");
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    int rc;
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n_frames))) return rc;
    *bytes = post_layout(n_frames, pd::make_geometry(n_frames, sample_rate, hop_ms, window_ms)).total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_frames(const float* probs, int N, int W, float threshold, int min_vally, int min_hill, int hang_before, int hang_over,
                                   float* boosted, uint8_t* trimmed, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (N < 0 || W < 1) return fail(SAVAD_E_INVALID, "N = %d, W = %d", N, W);
    if ((rc = post_check_trim(min_vally, min_hill, hang_before, hang_over))) return rc;
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    if (N == 0) return SAVAD_OK;
    if (!probs || !boosted || !trimmed || !ws) return fail(SAVAD_E_INVALID, "null pointer");
    pd::Geometry none = pd::make_geometry(0, 1, 1000.0, 1000.0);
    const PostLayout L = post_layout(N, none);
    if (ws_bytes < L.frames_end) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, L.frames_end);
    int* last = (int*)((char*)ws + L.last);
    int* next = (int*)((char*)ws + L.next);
    int* sums = (int*)((char*)ws + L.sums_f);
    const int block = post_block();
    hipLaunchKernelGGL(pd::frames_kernel, dim3(grid_for(N)), dim3(256), 0, st, probs, N, W, threshold, boosted, trimmed);
    for (int pass = 0; pass < 3; ++pass) {
        if ((pass == 0 && min_vally <= 0) || (pass == 1 && min_hill <= 0) || (pass == 2 && hang_before <= 0)) continue;
        const int k_last = pass == 1 ? 0 : 1, k_next = pass == 1 ? 1 : 0;
        pd::scan_run<pd::OpMax>(st, N, block, pd::EdgeLoad{trimmed, N, k_last, 0}, pd::EdgeStore{last, N, 0}, sums);
        pd::scan_run<pd::OpMin>(st, N, block, pd::EdgeLoad{trimmed, N, k_next, 1}, pd::EdgeStore{next, N, 1}, sums);
        hipLaunchKernelGGL(pd::trim_apply_kernel, dim3(grid_for(N)), dim3(256), 0, st, trimmed, N, pass, (const int*)last, (const int*)next, min_vally,
                           min_hill, hang_before, hang_over);
    }
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_segments(const uint8_t* trimmed, const float* boosted, int N, int sample_rate, double hop_ms, double window_ms,
                                     long max_samples, long* starts, long* ends, int cap, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if (N < 0 || cap < 0 || max_samples < 0 || max_samples == 1) return fail(SAVAD_E_INVALID, "N = %d, cap = %d, max_samples = %ld", N, cap, max_samples);
    if (cap > 0 && (!starts || !ends)) return fail(SAVAD_E_INVALID, "null output");
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, N))) return rc;
    if (N == 0) return 0;
    if (!trimmed || (max_samples > 0 && !boosted) || !ws) return fail(SAVAD_E_INVALID, "null pointer");
    const pd::Geometry g = pd::make_geometry(N, sample_rate, hop_ms, window_ms);
    const PostLayout L = post_layout(N, g);
    if (ws_bytes < L.total) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    if (g.num == 0) return 0;
    char* base = (char*)ws;
    uint8_t* cls = (uint8_t*)(base + L.cls);
    uint8_t* state = (uint8_t*)(base + L.state);
    pd::Long2* sums = (pd::Long2*)(base + L.sums_s);
    long* d_starts = (long*)(base + L.seg_starts);
    long* d_ends = (long*)(base + L.seg_ends);
    long* d_totals = (long*)(base + L.totals);
    pd::MinKey* d_partial = (pd::MinKey*)(base + L.partial);
    pd::MinKey* d_result = (pd::MinKey*)(base + L.result);
    const int block = post_block();
    long tot[2] = {0, 0};
    long have_first = -1;   // the window of segments the buffers hold

    // the segments of the classes as they stand: state scan (when the classes changed), flags, prefix sums, scatter of the
    // window [first, first + seg_cap), totals to the host.  Synchronises.
    auto segments_pass = [&](bool classes_changed, long first) -> int {
        if (classes_changed) pd::scan_run<pd::OpLast>(st, g.num, block, pd::ClassLoad{cls}, pd::ClassStore{state}, (int*)sums);
        const pd::FlagLoad flags{cls, state, g.num};
        pd::scan_run<pd::OpSum2>(st, g.num + 1, block, flags, pd::SegmentStore{flags, d_starts, d_ends, first, L.seg_cap, d_totals}, sums);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(tot, d_totals, sizeof(tot), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        have_first = first;
        if (tot[0] != tot[1]) return fail(SAVAD_E_STATE, "%ld starts and %ld ends", tot[0], tot[1]);
        if (tot[0] > INT_MAX) return fail(SAVAD_E_UNSUPPORTED, "%ld segments", tot[0]);
        return SAVAD_OK;
    };
    // copies segments [first, first + count) to the host; count <= seg_cap
    auto fetch = [&](long first, long count, long* hs, long* he) -> int {
        if (have_first != first) {
            int r = segments_pass(false, first);
            if (r) return r;
        }
        HIP_TRY(hipMemcpyAsync(hs, d_starts, sizeof(long) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(he, d_ends, sizeof(long) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        return SAVAD_OK;
    };

    hipLaunchKernelGGL(pd::sample_class_kernel, dim3(grid_for(g.num)), dim3(256), 0, st, trimmed, g, cls);
    if ((rc = segments_pass(true, 0))) return rc;

    if (max_samples > 0 && tot[0] > 0) {
        // vad/postprocessing/split.py:26-109: the recursion of savad_post.h's split_long_block on the host, its argmin as range queries
        // to the device (one stream synchronisation per query; a long segment needs on the order of len / max_samples of them)
        const long half = max_samples / 2;
        auto query = [&](long a, long b, long* best) -> int {
            const long work = (b - a + 255) / 256;
            const int grid = (int)(work < pd::ARGMIN_GRID ? work : pd::ARGMIN_GRID);
            pd::MinKey r;
            hipLaunchKernelGGL(pd::argmin_stage1_kernel, dim3(grid), dim3(256), 0, st, boosted, g, a, b, d_partial);
            hipLaunchKernelGGL(pd::argmin_stage2_kernel, dim3(1), dim3(256), 0, st, (const pd::MinKey*)d_partial, grid, d_result);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(&r, d_result, sizeof(r), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (r.index < a || r.index >= b) return fail(SAVAD_E_STATE, "argmin over [%ld, %ld) answered %ld", a, b, r.index);
            *best = r.index;
            return SAVAD_OK;
        };
        std::vector<long> breaks;
        // break points of the long block [s, s + len) (len > max_samples); the right-hand remainder is walked in a loop
        std::function<int(long, long)> split = [&](long s, long len) -> int {
            for (;;) {
                long best;
                int r = query(s + half, s + len - half, &best);
                if (r) return r;
                const long bp = best - s;
                if (bp > max_samples && (r = split(s, bp))) return r;
                breaks.push_back(s + bp);
                const long rlen = len - bp - 1;
                if (rlen <= max_samples) return SAVAD_OK;
                s += bp + 1;
                len = rlen;
            }
        };
        const long count = tot[0];
        std::vector<long> hs((size_t)(count < L.seg_cap ? count : L.seg_cap)), he(hs.size());
        for (long first = 0; first < count; first += L.seg_cap) {
            const long c = count - first < L.seg_cap ? count - first : L.seg_cap;
            if ((rc = fetch(first, c, hs.data(), he.data()))) return rc;
            for (long k = 0; k < c; ++k)
                if (he[k] + 1 - hs[k] > max_samples && (rc = split(hs[k], he[k] + 1 - hs[k]))) return rc;
        }
        if (!breaks.empty()) {   // (sorted: the recursion emits them in order.)  Uploaded through the segment buffer, a chunk at a time
            for (size_t at = 0; at < breaks.size(); at += (size_t)L.seg_cap) {
                const size_t c = breaks.size() - at < (size_t)L.seg_cap ? breaks.size() - at : (size_t)L.seg_cap;
                HIP_TRY(hipMemcpyAsync(d_starts, breaks.data() + at, sizeof(long) * c, hipMemcpyHostToDevice, st));
                hipLaunchKernelGGL(pd::breaks_kernel, dim3((unsigned)((c + 255) / 256)), dim3(256), 0, st, (const long*)d_starts, (int)c, g.num, cls);
                HIP_TRY(hipStreamSynchronize(st));   // (the chunk's source and the buffer are free again)
            }
            if ((rc = segments_pass(true, 0))) return rc;
        }
    }
    const long count = tot[0], want = count < cap ? count : cap;
    for (long first = 0; first < want; first += L.seg_cap) {
        const long c = want - first < L.seg_cap ? want - first : L.seg_cap;
        if ((rc = fetch(first, c, starts + first, ends + first))) return rc;
    }
    return (int)count;
}

SAVAD_EXPORT int savad_post_sample_probs(const float* boosted, int N, int sample_rate, double hop_ms, double window_ms, double* out, void* stream) {
    int rc;
    if (N < 0) return fail(SAVAD_E_INVALID, "N = %d", N);
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, N))) return rc;
    const pd::Geometry g = pd::make_geometry(N, sample_rate, hop_ms, window_ms);
    if (g.num == 0) return SAVAD_OK;
    if ((N > 0 && !boosted) || !out) return fail(SAVAD_E_INVALID, "null pointer");
    hipLaunchKernelGGL(pd::sample_probs_kernel, dim3(grid_for(g.num)), dim3(256), 0, (hipStream_t)stream, boosted, g, out);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_frames_host(const float* probs, int N, int W, float threshold, int min_vally, int min_hill, int hang_before, int hang_over,
                                        float* boosted, uint8_t* trimmed) {
    int rc;
    if (N < 0 || W < 1) return fail(SAVAD_E_INVALID, "N = %d, W = %d", N, W);
    if ((rc = post_check_trim(min_vally, min_hill, hang_before, hang_over))) return rc;
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    if (N == 0) return SAVAD_OK;
    if (!probs || !boosted || !trimmed) return fail(SAVAD_E_INVALID, "null pointer");
    for (int i = 0; i < N; ++i) {
        boosted[i] = pd::row_mean(probs + (size_t)i * W, W);
        trimmed[i] = pd::above(boosted[i], threshold);
    }
    std::vector<int> last((size_t)N), next((size_t)N);
    pd::trim_host(trimmed, N, min_vally, min_hill, hang_before, hang_over, last.data(), next.data());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_sample_class_host(const uint8_t* frames, int n, int sample_rate, double hop_ms, double window_ms, long first, long count,
                                              uint8_t* cls) {
    int rc;
    if (n < 0 || first < 0 || count < 0) return fail(SAVAD_E_INVALID, "n = %d, samples [%ld, +%ld)", n, first, count);
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n))) return rc;
    const pd::Geometry g = pd::make_geometry(n, sample_rate, hop_ms, window_ms);
    if (first + count > g.num) return fail(SAVAD_E_INVALID, "samples [%ld, +%ld) of %ld", first, count, g.num);
    if (count == 0) return SAVAD_OK;
    if ((n > 0 && !frames) || !cls) return fail(SAVAD_E_INVALID, "null pointer");
    for (long i = 0; i < count; ++i) cls[i] = pd::sample_class(frames, g, first + i);
    return SAVAD_OK;
}

// ---- post-processing of every clip of a batch (savad_post_batch.h) ----------------------------------------------------------
namespace {

struct PostBatchLayout {   // byte offsets into the caller's workspace: host arithmetic from the table
    size_t row_lo, row_hi, last, next, sums_f, frames_end;                                       // savad_post_batch_frames
    size_t slot_first, sums_c, cls, state, sums_s, seg_starts, seg_ends, seg_clip, result, single, total;   // savad_post_batch_segments
    size_t result_bytes, single_bytes;   // result: totals [2] long | clip_total [C] long | flags [C] bytes, fetched in one copy
    long slots, seg_cap;                 // slots of all clips; room of the segment buffers (without a split a segment needs a frame of its own)
    int rows, n_max;                     // rows of the table; frames of its longest clip
};

// the HOST table validated (as the batched prediction does) and measured
int post_batch_table(const int32_t* clip_first_host, int C, int* rows, int* n_max) {
    if (!clip_first_host || C < 1) return fail(SAVAD_E_INVALID, "clip table: at least one clip");
    if (clip_first_host[0] != 0) return fail(SAVAD_E_INVALID, "clip table: clip_first[0] must be 0");
    int longest = 0;
    for (int c = 0; c < C; ++c) {
        const long n = (long)clip_first_host[c + 1] - clip_first_host[c];
        if (n < 0) return fail(SAVAD_E_INVALID, "clip table: clip_first must not decrease");
        if (n > longest) longest = (int)n;
    }
    *rows = clip_first_host[C];
    *n_max = longest;
    return SAVAD_OK;
}

// geometry: only the frame stage's share is laid out when sample_rate == 0
PostBatchLayout post_batch_layout(const int32_t* clip_first_host, int C, int rows, int n_max, int sample_rate, double hop_ms, double window_ms) {
    PostBatchLayout L{};
    Arena a;
    const size_t N = (size_t)rows;
    L.rows = rows, L.n_max = n_max;
    L.row_lo = a.take(sizeof(int) * N);
    L.row_hi = a.take(sizeof(int) * N);
    L.last = a.take(sizeof(int) * N);
    L.next = a.take(sizeof(int) * N);
    L.sums_f = a.take(sizeof(int) * (size_t)pd::scan_sums_elems(rows));
    L.frames_end = a.off;
    if (sample_rate == 0) return L;
    for (int c = 0; c < C; ++c) L.slots += pd::clip_slots(clip_first_host[c + 1] - clip_first_host[c], sample_rate, hop_ms, window_ms);
    L.seg_cap = (long)rows + 2 * (long)C;
    L.slot_first = a.take(sizeof(long) * ((size_t)C + 1));
    L.sums_c = a.take(sizeof(long) * (size_t)pd::scan_sums_elems(C));
    L.cls = a.take((size_t)L.slots);
    L.state = a.take((size_t)L.slots);
    L.sums_s = a.take(sizeof(pd::Long2) * (size_t)pd::scan_sums_elems(L.slots));
    L.seg_starts = a.take(sizeof(long) * (size_t)L.seg_cap);
    L.seg_ends = a.take(sizeof(long) * (size_t)L.seg_cap);
    L.seg_clip = a.take(sizeof(int) * (size_t)L.seg_cap);
    L.result_bytes = sizeof(long) * (2 + (size_t)C) + (size_t)C;
    L.result = a.take(L.result_bytes);
    L.single_bytes = post_layout(n_max, pd::make_geometry(n_max, sample_rate, hop_ms, window_ms)).total;   // a flagged clip's savad_post_segments
    L.single = a.take(L.single_bytes);
    L.total = a.off;
    return L;
}

int post_batch_check_w(int W) {
    if (W < 1) return fail(SAVAD_E_INVALID, "W = %d", W);
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT int savad_post_batch_supported(const int32_t* clip_first_host, int C, int W, int sample_rate, double hop_ms, double window_ms) {
    if (!clip_first_host || C < 1 || clip_first_host[0] != 0) return 0;
    for (int c = 0; c < C; ++c) {
        const long n = (long)clip_first_host[c + 1] - clip_first_host[c];
        if (n < 0 || !savad_post_supported(W, sample_rate, hop_ms, window_ms, (int)n)) return 0;
    }
    return 1;
}

SAVAD_EXPORT int savad_post_batch_slot_table(const int32_t* clip_first_host, int C, int sample_rate, double hop_ms, double window_ms, long* slot_first) {
    int rc, rows, n_max;
    if ((rc = post_batch_table(clip_first_host, C, &rows, &n_max))) return rc;
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n_max))) return rc;   // (the longest clip's span bounds every other)
    if (!slot_first) return fail(SAVAD_E_INVALID, "null pointer");
    pd::slot_table_host(clip_first_host, C, sample_rate, hop_ms, window_ms, slot_first);
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_batch_workspace_bytes(const int32_t* clip_first_host, int C, int W, int sample_rate, double hop_ms, double window_ms,
                                                  size_t* bytes) {
    int rc, rows, n_max;
    if (!bytes) return fail(SAVAD_E_INVALID, "null pointer");
    if ((rc = post_batch_table(clip_first_host, C, &rows, &n_max))) return rc;
    if ((rc = post_batch_check_w(W))) return rc;
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n_max))) return rc;
    *bytes = post_batch_layout(clip_first_host, C, rows, n_max, sample_rate, hop_ms, window_ms).total;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_batch_frames(const float* probs, const int32_t* clip_first_host, const int32_t* clip_first, int C, int W, float threshold,
                                         int min_vally, int min_hill, int hang_before, int hang_over, float* boosted, uint8_t* trimmed, void* ws,
                                         size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc, N, n_max;
    if ((rc = post_batch_table(clip_first_host, C, &N, &n_max))) return rc;
    if ((rc = post_batch_check_w(W))) return rc;
    if ((rc = post_check_trim(min_vally, min_hill, hang_before, hang_over))) return rc;
    if (N == 0) return SAVAD_OK;
    if (!probs || !clip_first || !boosted || !trimmed || !ws) return fail(SAVAD_E_INVALID, "null pointer");
    if ((uintptr_t)ws & 7) return fail(SAVAD_E_INVALID, "workspace must be 8-byte aligned");
    const PostBatchLayout L = post_batch_layout(clip_first_host, C, N, n_max, 0, 0.0, 0.0);
    if (ws_bytes < L.frames_end) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, L.frames_end);
    char* base = (char*)ws;
    int* row_lo = (int*)(base + L.row_lo);
    int* row_hi = (int*)(base + L.row_hi);
    int* last = (int*)(base + L.last);
    int* next = (int*)(base + L.next);
    int* sums = (int*)(base + L.sums_f);
    const int block = post_block();
    hipLaunchKernelGGL(pd::frames_batch_kernel, dim3(grid_for(N)), dim3(256), 0, st, probs, clip_first, C, N, W, threshold, boosted, trimmed, row_lo,
                       row_hi);
    for (int pass = 0; pass < 3; ++pass) {
        if ((pass == 0 && min_vally <= 0) || (pass == 1 && min_hill <= 0) || (pass == 2 && hang_before <= 0)) continue;
        const int k_last = pass == 1 ? 0 : 1, k_next = pass == 1 ? 1 : 0;
        pd::scan_run<pd::OpMax>(st, N, block, pd::EdgeLoadBatch{trimmed, row_lo, N, k_last, 0}, pd::EdgeStore{last, N, 0}, sums);
        pd::scan_run<pd::OpMin>(st, N, block, pd::EdgeLoadBatch{trimmed, row_lo, N, k_next, 1}, pd::EdgeStore{next, N, 1}, sums);
        hipLaunchKernelGGL(pd::trim_apply_batch_kernel, dim3(grid_for(N)), dim3(256), 0, st, trimmed, N, pass, (const int*)last, (const int*)next,
                           (const int*)row_lo, (const int*)row_hi, min_vally, min_hill, hang_before, hang_over);
    }
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

// Launches and synchronisations of a batch in which no clip is flagged: one scan of C elements, one launch over the slots, two
// scans of them, (with max_samples) one memset and one launch over the segments, two synchronisations -- the scans' levels grow
// with log(slots), nothing with the number of clips.  A flagged clip adds its own savad_post_segments.
SAVAD_EXPORT int savad_post_batch_segments(const uint8_t* trimmed, const float* boosted, const int32_t* clip_first_host, const int32_t* clip_first,
                                           int C, int sample_rate, double hop_ms, double window_ms, long max_samples, long* seg_first_host,
                                           uint8_t* long_host, long* starts, long* ends, int cap, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc, N, n_max;
    if ((rc = post_batch_table(clip_first_host, C, &N, &n_max))) return rc;
    if (cap < 0 || max_samples < 0 || max_samples == 1) return fail(SAVAD_E_INVALID, "cap = %d, max_samples = %ld", cap, max_samples);
    if (!seg_first_host || !long_host || (cap > 0 && (!starts || !ends))) return fail(SAVAD_E_INVALID, "null output");
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n_max))) return rc;
    if (N > 0 && (!trimmed || !clip_first || (max_samples > 0 && !boosted) || !ws)) return fail(SAVAD_E_INVALID, "null pointer");
    if ((uintptr_t)ws & 7) return fail(SAVAD_E_INVALID, "workspace must be 8-byte aligned");
    const PostBatchLayout L = post_batch_layout(clip_first_host, C, N, n_max, sample_rate, hop_ms, window_ms);
    if (N > 0 && ws_bytes < L.total) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, L.total);
    for (int c = 0; c <= C; ++c) seg_first_host[c] = 0;
    for (int c = 0; c < C; ++c) long_host[c] = 0;
    if (N == 0) return 0;
    char* base = (char*)ws;
    long* slot_first = (long*)(base + L.slot_first);
    uint8_t* cls = (uint8_t*)(base + L.cls);
    uint8_t* state = (uint8_t*)(base + L.state);
    pd::Long2* sums = (pd::Long2*)(base + L.sums_s);
    long* d_starts = (long*)(base + L.seg_starts);
    long* d_ends = (long*)(base + L.seg_ends);
    int* d_seg_clip = (int*)(base + L.seg_clip);
    long* d_totals = (long*)(base + L.result);
    long* d_clip_total = d_totals + 2;
    uint8_t* d_flags = (uint8_t*)(d_clip_total + C);
    const int block = post_block();

    pd::scan_run<pd::OpSumL>(st, C, block, pd::SlotCountLoad{clip_first, sample_rate, hop_ms, window_ms}, pd::SlotFirstStore{slot_first},
                             (long*)(base + L.sums_c));
    hipLaunchKernelGGL(pd::slot_class_kernel, dim3(grid_for(L.slots)), dim3(256), 0, st, trimmed, clip_first, (const long*)slot_first, C, L.slots,
                       sample_rate, hop_ms, window_ms, cls);
    pd::scan_run<pd::OpLast>(st, L.slots, block, pd::ClassLoadBatch{cls}, pd::ClassStore{state}, (int*)sums);
    const pd::FlagLoadBatch flags{cls, state};
    pd::scan_run<pd::OpSum2>(st, L.slots, block, flags,
                             pd::SegmentStoreBatch{flags, slot_first, C, L.slots, d_starts, d_ends, d_seg_clip, L.seg_cap, d_clip_total, d_totals}, sums);
    if (max_samples > 0) {
        HIP_TRY(hipMemsetAsync(d_flags, 0, (size_t)C, st));
        hipLaunchKernelGGL(pd::long_flag_kernel, dim3(grid_for(L.seg_cap)), dim3(256), 0, st, (const long*)d_starts, (const long*)d_ends,
                           (const int*)d_seg_clip, (const long*)d_totals, L.seg_cap, max_samples, d_flags);
    }
    HIP_TRY(hipGetLastError());
    std::vector<char> result(L.result_bytes);
    HIP_TRY(hipMemcpyAsync(result.data(), d_totals, max_samples > 0 ? L.result_bytes : L.result_bytes - (size_t)C, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));   // the first of two
    long tot[2];
    memcpy(tot, result.data(), sizeof(tot));
    if (tot[0] != tot[1]) return fail(SAVAD_E_STATE, "%ld starts and %ld ends", tot[0], tot[1]);
    if (tot[0] > L.seg_cap) return fail(SAVAD_E_STATE, "%ld segments in %d frames of %d clips", tot[0], N, C);
    if (tot[0] > INT_MAX) return fail(SAVAD_E_UNSUPPORTED, "%ld segments", tot[0]);
    bool any_long = false;
    for (int c = 0; c < C; ++c) {   // a clip without rows has no closing slot: it ends where the clip before it ends
        long upto = seg_first_host[c];
        if (clip_first_host[c + 1] > clip_first_host[c]) memcpy(&upto, result.data() + sizeof(long) * (2 + (size_t)c), sizeof(long));
        seg_first_host[c + 1] = upto;
        if (max_samples > 0) long_host[c] = (uint8_t)result[sizeof(long) * (2 + (size_t)C) + (size_t)c];
        any_long = any_long || long_host[c];
    }
    const long count = tot[0];
    if (!any_long) {
        const size_t want = (size_t)(count < cap ? count : cap);
        if (want) {
            HIP_TRY(hipMemcpyAsync(starts, d_starts, sizeof(long) * want, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(ends, d_ends, sizeof(long) * want, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));   // the second
        }
        return (int)count;
    }
    // some clip holds an over-long segment: the optimal split stays the single-clip routine, run on that clip's slice; every
    // other clip keeps the pairs of the batch
    std::vector<long> bs((size_t)count), be((size_t)count), os, oe, one_s, one_e;
    if (count) {
        HIP_TRY(hipMemcpyAsync(bs.data(), d_starts, sizeof(long) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(be.data(), d_ends, sizeof(long) * (size_t)count, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    long before = 0;   // seg_first_host[c] of the batch pass, before the entry is rewritten
    for (int c = 0; c < C; ++c) {
        const long upto = seg_first_host[c + 1];
        if (!long_host[c]) {
            os.insert(os.end(), bs.begin() + before, bs.begin() + upto);
            oe.insert(oe.end(), be.begin() + before, be.begin() + upto);
        } else {
            const int lo = clip_first_host[c], n = clip_first_host[c + 1] - lo;
            int one_cap = n + 2;
            for (;;) {
                one_s.resize((size_t)one_cap), one_e.resize((size_t)one_cap);
                const int got = savad_post_segments(trimmed + lo, boosted + lo, n, sample_rate, hop_ms, window_ms, max_samples, one_s.data(),
                                                    one_e.data(), one_cap, base + L.single, L.single_bytes, stream);
                if (got < 0) return got;
                if (got <= one_cap) {
                    one_cap = got;
                    break;
                }
                one_cap = got;   // (a split into more pieces than frames)
            }
            os.insert(os.end(), one_s.begin(), one_s.begin() + one_cap);
            oe.insert(oe.end(), one_e.begin(), one_e.begin() + one_cap);
        }
        before = upto;
        if (os.size() > (size_t)INT_MAX) return fail(SAVAD_E_UNSUPPORTED, "%zu segments", os.size());
        seg_first_host[c + 1] = (long)os.size();
    }
    const size_t want = os.size() < (size_t)cap ? os.size() : (size_t)cap;
    if (want) {
        memcpy(starts, os.data(), sizeof(long) * want);
        memcpy(ends, oe.data(), sizeof(long) * want);
    }
    return (int)os.size();
}

SAVAD_EXPORT int savad_post_batch_frames_host(const float* probs, const int32_t* clip_first_host, int C, int W, float threshold, int min_vally,
                                              int min_hill, int hang_before, int hang_over, float* boosted, uint8_t* trimmed) {
    int rc, N, n_max;
    if ((rc = post_batch_table(clip_first_host, C, &N, &n_max))) return rc;
    if ((rc = post_batch_check_w(W))) return rc;
    if ((rc = post_check_trim(min_vally, min_hill, hang_before, hang_over))) return rc;
    if (N == 0) return SAVAD_OK;
    if (!probs || !boosted || !trimmed) return fail(SAVAD_E_INVALID, "null pointer");
    for (int i = 0; i < N; ++i) {
        boosted[i] = pd::row_mean(probs + (size_t)i * W, W);
        trimmed[i] = pd::above(boosted[i], threshold);
    }
    std::vector<int> row_lo((size_t)N), row_hi((size_t)N), last((size_t)N), next((size_t)N);
    pd::clip_bounds_host(clip_first_host, C, N, row_lo.data(), row_hi.data());
    pd::trim_batch_host(trimmed, N, row_lo.data(), row_hi.data(), min_vally, min_hill, hang_before, hang_over, last.data(), next.data());
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_post_batch_slot_class_host(const uint8_t* frames, const int32_t* clip_first_host, int C, int sample_rate, double hop_ms,
                                                  double window_ms, uint8_t* cls) {
    int rc, N, n_max;
    if ((rc = post_batch_table(clip_first_host, C, &N, &n_max))) return rc;
    if ((rc = post_check_geometry(sample_rate, hop_ms, window_ms, n_max))) return rc;
    if (N == 0) return SAVAD_OK;
    if (!frames || !cls) return fail(SAVAD_E_INVALID, "null pointer");
    std::vector<long> slot_first((size_t)C + 1);
    pd::slot_table_host(clip_first_host, C, sample_rate, hop_ms, window_ms, slot_first.data());
    for (long j = 0; j < slot_first[(size_t)C]; ++j) {
        const int c = pd::clip_of(slot_first.data(), C, j);
        const int lo = clip_first_host[c];
        cls[j] = pd::slot_class(frames + lo, clip_first_host[c + 1] - lo, j - slot_first[(size_t)c], sample_rate, hop_ms, window_ms);
    }
    return SAVAD_OK;
}

// ---- evaluate's metrics on the device (savad_eval_device.h) --------------------------------------------------------------------
namespace {

namespace ed = savad::evaldev;

int g_eval_block = 0;   // savad_eval_set_block: elements per workgroup block of the sort and of its scans (0 = the default)

int eval_block() { return g_eval_block ? g_eval_block : ed::SORT_BLOCK_DEFAULT; }

struct EvalLayout {   // byte offsets into the caller's workspace: a function of the frame count alone
    size_t keys_a, keys_b, y, labels_a, labels_b, spred, bpred, table, sums, scan, seg, counters, total;
    long seg_cap;     // records of the boundary buffer: a true segment needs a frame of its own and a gap
};

EvalLayout eval_layout(long N) {
    EvalLayout L;
    Arena a;
    const size_t n = (size_t)N;
    L.keys_a = a.take(sizeof(uint32_t) * n);
    L.keys_b = a.take(sizeof(uint32_t) * n);
    L.y = a.take(n);
    L.labels_a = a.take(n);
    L.labels_b = a.take(n);
    L.spred = a.take(n);
    L.bpred = a.take(n);
    L.table = a.take(sizeof(unsigned) * (size_t)ed::sort_table_elems(N));
    const size_t sums_sort = sizeof(unsigned) * (size_t)pd::scan_sums_elems(ed::sort_table_elems(N));
    const size_t sums_frames = sizeof(pd::Long2) * (size_t)pd::scan_sums_elems(N);   // (Long2 is the larger of the two frame scans' types)
    L.sums = a.take(sums_sort > sums_frames ? sums_sort : sums_frames);
    L.scan = a.take(sizeof(ed::HeadNeg) * n);
    L.seg_cap = (N + 1) / 2;
    L.seg = a.take((size_t)ed::SEG_BYTES * (size_t)L.seg_cap);
    L.counters = a.take(sizeof(long) * ed::COUNTERS);
    L.total = a.off;
    return L;
}

long eval_frames(long n_frames, long n_labels) { return n_frames < n_labels ? n_frames : n_labels; }

int eval_check(int W, long n_frames, long n_labels, int L) {
    if (n_frames < 0 || n_labels < 0 || W < 1) return fail(SAVAD_E_INVALID, "N = %ld, labels = %ld, W = %d", n_frames, n_labels, W);
    if (L < 1 || L > ed::L_MAX) return fail(SAVAD_E_INVALID, "L = %d (1 .. %d)", L, ed::L_MAX);
    if (!savad_eval_supported(W, n_frames, n_labels))
        return fail(SAVAD_E_UNSUPPORTED, "W = %d, %ld frames, %ld labels: the device metrics take 1 <= W <= %d and 1 <= min(frames, labels) < 2^31", W,
                    n_frames, n_labels, pd::W_MAX);
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT int savad_eval_supported(int W, long n_frames, long n_labels) {
    const long n = eval_frames(n_frames, n_labels);
    return W >= 1 && W <= pd::W_MAX && n >= 1 && n < 2147483648L ? 1 : 0;
}

SAVAD_EXPORT int savad_eval_set_block(int elems) {
    if (elems != 0 && (elems < pd::SCAN_BLOCK_MIN || elems > ed::SORT_BLOCK_DEFAULT || (elems & (elems - 1))))
        return fail(SAVAD_E_INVALID, "sort block %d (0 = default, or a power of two from %d to %d)", elems, pd::SCAN_BLOCK_MIN, ed::SORT_BLOCK_DEFAULT);
    g_eval_block = elems;
    return SAVAD_OK;
}

SAVAD_EXPORT int savad_eval_workspace_bytes(int n_frames, int W, size_t* bytes) {
    if (!bytes || n_frames < 0 || W < 1) return fail(SAVAD_E_INVALID, "bad argument");
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    *bytes = eval_layout(n_frames).total;
    return SAVAD_OK;
}

SAVAD_EXPORT long savad_eval_counts(const float* probs, int N, int W, const uint8_t* labels, long n_labels, float threshold, int L, long* counters,
                                    uint8_t* seg, long seg_cap, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    if ((rc = eval_check(W, N, n_labels, L))) return rc;
    if (!probs || !labels || !counters || !ws || seg_cap < 0 || (seg_cap > 0 && !seg)) return fail(SAVAD_E_INVALID, "null pointer");
    const int n = (int)eval_frames(N, n_labels);
    const EvalLayout Y = eval_layout(N);
    if (ws_bytes < Y.total) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, Y.total);
    char* base = (char*)ws;
    uint32_t* keys_a = (uint32_t*)(base + Y.keys_a);
    uint32_t* keys_b = (uint32_t*)(base + Y.keys_b);
    uint8_t* y = (uint8_t*)(base + Y.y);
    uint8_t* labels_a = (uint8_t*)(base + Y.labels_a);
    uint8_t* labels_b = (uint8_t*)(base + Y.labels_b);
    uint8_t* spred = (uint8_t*)(base + Y.spred);
    uint8_t* bpred = (uint8_t*)(base + Y.bpred);
    unsigned* table = (unsigned*)(base + Y.table);
    void* sums = base + Y.sums;
    ed::HeadNeg* scan = (ed::HeadNeg*)(base + Y.scan);
    uint8_t* d_seg = (uint8_t*)(base + Y.seg);
    long* d_counters = (long*)(base + Y.counters);
    const int block = eval_block();

    HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(long) * ed::COUNTERS, st));
    hipLaunchKernelGGL(ed::frames_kernel, dim3(grid_for(n)), dim3(256), 0, st, probs, W, labels, n, threshold, keys_a, y, spred, bpred, d_counters);
    hipLaunchKernelGGL(ed::counts_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const uint8_t*)y, (const uint8_t*)spred, (const uint8_t*)bpred, n, d_counters);
    const ed::BoundaryLoad flags{y, n};
    pd::scan_run<pd::OpSum2>(st, n, block, flags, ed::BoundaryStore{flags, spred, bpred, L, d_seg, Y.seg_cap}, (pd::Long2*)sums);
    ed::sort_run(st, n, block, keys_a, keys_b, y, labels_a, labels_b, table, (unsigned*)sums);
    pd::scan_run<ed::OpHeadNeg>(st, n, block, ed::HeadNegLoad{keys_a, labels_a}, pd::PtrStore<ed::HeadNeg>{scan}, (ed::HeadNeg*)sums);
    hipLaunchKernelGGL(ed::u2_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const uint32_t*)keys_a, (const uint8_t*)labels_a, (const ed::HeadNeg*)scan, n,
                       d_counters);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(long) * ed::COUNTERS, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    counters[ed::C_N] = n;
    const long n_true = counters[ed::C_TRUE];
    if (n_true < 0 || n_true > Y.seg_cap) return fail(SAVAD_E_STATE, "%ld true segments in %d frames", n_true, n);
    if (n_true > seg_cap) return fail(SAVAD_E_INVALID, "%ld true segments, room for %ld", n_true, seg_cap);
    if (n_true > 0) {
        HIP_TRY(hipMemcpyAsync(seg, d_seg, (size_t)ed::SEG_BYTES * (size_t)n_true, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    return n_true;
}

SAVAD_EXPORT int savad_eval_sort(const float* keys, const uint8_t* labels, long n, float* sorted_keys, uint8_t* sorted_labels, void* ws, size_t ws_bytes,
                                 void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n < 0 || n >= 2147483648L) return fail(SAVAD_E_INVALID, "n = %ld", n);
    if (n == 0) return SAVAD_OK;
    if (!keys || !labels || !sorted_keys || !sorted_labels || !ws) return fail(SAVAD_E_INVALID, "null pointer");
    const EvalLayout Y = eval_layout(n);
    if (ws_bytes < Y.total) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, Y.total);
    char* base = (char*)ws;
    uint32_t* keys_a = (uint32_t*)(base + Y.keys_a);
    uint8_t* labels_a = (uint8_t*)(base + Y.labels_a);
    hipLaunchKernelGGL(ed::keys_kernel, dim3(grid_for(n)), dim3(256), 0, st, keys, n, keys_a);
    ed::sort_run(st, n, eval_block(), keys_a, (uint32_t*)(base + Y.keys_b), labels, labels_a, (uint8_t*)(base + Y.labels_b), (unsigned*)(base + Y.table),
                 (unsigned*)(base + Y.sums));
    hipLaunchKernelGGL(ed::values_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const uint32_t*)keys_a, (const uint8_t*)labels_a, n, sorted_keys, sorted_labels);
    HIP_TRY(hipGetLastError());
    return SAVAD_OK;
}

SAVAD_EXPORT long savad_eval_counts_host(const float* probs, int N, int W, const uint8_t* labels, long n_labels, float threshold, int L, long* counters,
                                         uint8_t* seg, long seg_cap) {
    int rc;
    if ((rc = eval_check(W, N, n_labels, L))) return rc;
    if (!probs || !labels || !counters || seg_cap < 0 || (seg_cap > 0 && !seg)) return fail(SAVAD_E_INVALID, "null pointer");
    const int n = (int)eval_frames(N, n_labels);
    const long n_true = ed::counts_host(probs, W, labels, n, threshold, L, counters, seg, seg_cap);
    if (n_true > seg_cap) return fail(SAVAD_E_INVALID, "%ld true segments, room for %ld", n_true, seg_cap);
    return n_true;
}

// ---- evaluate's metrics for every clip of a batch (savad_eval_batch.h) ---------------------------------------------------------
namespace {

namespace eb = savad::evalbatch;

struct EvalBatchLayout {   // byte offsets into the caller's workspace: host arithmetic from the two tables
    size_t elem_first, block_first, sums_c, elem_clip, keys_a, keys_b, y, labels_a, labels_b, spred, bpred, table, sums, scan, seg, counters, total;
    long E, seg_cap;       // frames of all clips; records of the boundary buffer (a true segment needs a frame of its own and a gap, per clip)
};

// both HOST tables validated: the refusal's message, or null.  *E = the frames of all clips
const char* eval_batch_tables(const int32_t* clip_first_host, const int32_t* label_first_host, int C, long* E) {
    if (!clip_first_host || !label_first_host) return "null table";
    if (C < 1) return "at least one clip";
    if (clip_first_host[0] != 0 || label_first_host[0] != 0) return "clip_first[0] and label_first[0] must be 0";
    long total = 0;
    for (int c = 0; c < C; ++c) {
        if (clip_first_host[c + 1] < clip_first_host[c] || label_first_host[c + 1] < label_first_host[c]) return "a table must not decrease";
        total += eb::clip_frames(clip_first_host, label_first_host, c);
    }
    if (total >= 2147483648L) return "2^31 frames or more";
    *E = total;
    return nullptr;
}

EvalBatchLayout eval_batch_layout(const int32_t* clip_first_host, const int32_t* label_first_host, int C, long E) {
    EvalBatchLayout L;
    Arena a;
    const size_t n = (size_t)E;
    L.E = E;
    L.elem_first = a.take(sizeof(long) * ((size_t)C + 1));
    L.block_first = a.take(sizeof(long) * ((size_t)C + 1));
    L.sums_c = a.take(sizeof(pd::Long2) * (size_t)pd::scan_sums_elems(C));
    L.elem_clip = a.take(sizeof(int) * n);
    L.keys_a = a.take(sizeof(uint32_t) * n);
    L.keys_b = a.take(sizeof(uint32_t) * n);
    L.y = a.take(n);
    L.labels_a = a.take(n);
    L.labels_b = a.take(n);
    L.spred = a.take(n);
    L.bpred = a.take(n);
    const long table = eb::sort_table_elems(clip_first_host, label_first_host, C);
    L.table = a.take(sizeof(unsigned) * (size_t)table);
    const size_t sums_sort = sizeof(unsigned) * (size_t)pd::scan_sums_elems(table);
    const size_t sums_frames = sizeof(pd::Long2) * (size_t)pd::scan_sums_elems(E);   // (Long2 is the larger of the two frame scans' types)
    L.sums = a.take(sums_sort > sums_frames ? sums_sort : sums_frames);
    L.scan = a.take(sizeof(ed::HeadNeg) * n);
    L.seg_cap = 0;
    for (int c = 0; c < C; ++c) L.seg_cap += (eb::clip_frames(clip_first_host, label_first_host, c) + 1) / 2;
    L.seg = a.take((size_t)ed::SEG_BYTES * (size_t)L.seg_cap);
    L.counters = a.take(sizeof(long) * ed::COUNTERS * (size_t)C);
    L.total = a.off;
    return L;
}

// the arguments both forms of the call share
int eval_batch_check(const int32_t* clip_first_host, const int32_t* label_first_host, int C, int W, int L, long* E) {
    if (const char* why = eval_batch_tables(clip_first_host, label_first_host, C, E)) return fail(SAVAD_E_INVALID, "clip tables: %s", why);
    if (W < 1) return fail(SAVAD_E_INVALID, "W = %d", W);
    if (W > pd::W_MAX) return fail(SAVAD_E_UNSUPPORTED, "W = %d: the device row mean has numpy's order up to %d", W, pd::W_MAX);
    if (L < 1 || L > ed::L_MAX) return fail(SAVAD_E_INVALID, "L = %d (1 .. %d)", L, ed::L_MAX);
    return SAVAD_OK;
}

}  // namespace

SAVAD_EXPORT int savad_eval_batch_supported(const int32_t* clip_first_host, const int32_t* label_first_host, int C, int W) {
    long E;
    return !eval_batch_tables(clip_first_host, label_first_host, C, &E) && W >= 1 && W <= pd::W_MAX ? 1 : 0;
}

SAVAD_EXPORT int savad_eval_batch_workspace_bytes(const int32_t* clip_first_host, const int32_t* label_first_host, int C, int W, size_t* bytes) {
    int rc;
    long E;
    if (!bytes) return fail(SAVAD_E_INVALID, "null pointer");
    if ((rc = eval_batch_check(clip_first_host, label_first_host, C, W, 1, &E))) return rc;
    *bytes = eval_batch_layout(clip_first_host, label_first_host, C, E).total;
    return SAVAD_OK;
}

// Launches and synchronisations: one memset, one scan of C elements, two launches over the frames, two scans of them, four sort
// passes (histogram, scan of the digit table, scatter), one launch for the rank sum, two synchronisations -- the scans' levels
// grow with the logarithm of their lengths, nothing with the number of clips.
SAVAD_EXPORT long savad_eval_batch_counts(const float* probs, const int32_t* clip_first_host, const int32_t* clip_first, const uint8_t* labels,
                                          const int32_t* label_first_host, const int32_t* label_first, int C, int W, float threshold, int L,
                                          long* counters, uint8_t* seg, long seg_cap, long* seg_first_host, void* ws, size_t ws_bytes, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    int rc;
    long E;
    if ((rc = eval_batch_check(clip_first_host, label_first_host, C, W, L, &E))) return rc;
    if (!probs || !clip_first || !labels || !label_first || !counters || !seg_first_host || !ws || seg_cap < 0 || (seg_cap > 0 && !seg))
        return fail(SAVAD_E_INVALID, "null pointer");
    if ((uintptr_t)ws & 7) return fail(SAVAD_E_INVALID, "workspace must be 8-byte aligned");
    const EvalBatchLayout Y = eval_batch_layout(clip_first_host, label_first_host, C, E);
    if (ws_bytes < Y.total) return fail(SAVAD_E_INVALID, "workspace of %zu bytes, %zu needed", ws_bytes, Y.total);
    char* base = (char*)ws;
    long* elem_first = (long*)(base + Y.elem_first);
    long* block_first = (long*)(base + Y.block_first);
    int* elem_clip = (int*)(base + Y.elem_clip);
    uint32_t* keys_a = (uint32_t*)(base + Y.keys_a);
    uint32_t* keys_b = (uint32_t*)(base + Y.keys_b);
    uint8_t* y = (uint8_t*)(base + Y.y);
    uint8_t* labels_a = (uint8_t*)(base + Y.labels_a);
    uint8_t* labels_b = (uint8_t*)(base + Y.labels_b);
    uint8_t* spred = (uint8_t*)(base + Y.spred);
    uint8_t* bpred = (uint8_t*)(base + Y.bpred);
    unsigned* table = (unsigned*)(base + Y.table);
    void* sums = base + Y.sums;
    ed::HeadNeg* scan = (ed::HeadNeg*)(base + Y.scan);
    uint8_t* d_seg = (uint8_t*)(base + Y.seg);
    long* d_counters = (long*)(base + Y.counters);
    const int block = eval_block();
    long blocks = 0;
    for (int c = 0; c < C; ++c) blocks += eb::blocks_of(eb::clip_frames(clip_first_host, label_first_host, c), block);

    if (E > 0) {
        HIP_TRY(hipMemsetAsync(d_counters, 0, sizeof(long) * ed::COUNTERS * (size_t)C, st));
        pd::scan_run<pd::OpSum2>(st, C, block, eb::ClipCountLoad{clip_first, label_first, block}, eb::ClipFirstStore{elem_first, block_first},
                                 (pd::Long2*)(base + Y.sums_c));
        hipLaunchKernelGGL(eb::frames_kernel, dim3(grid_for(E)), dim3(256), 0, st, probs, clip_first, labels, label_first, (const long*)elem_first, C, E, W,
                           threshold, elem_clip, keys_a, y, spred, bpred, d_counters);
        hipLaunchKernelGGL(eb::counts_kernel, dim3(grid_for(E)), dim3(256), 0, st, (const uint8_t*)y, (const uint8_t*)spred, (const uint8_t*)bpred,
                           (const int*)elem_clip, (const long*)elem_first, E, d_counters);
        const eb::BoundaryLoad flags{y, elem_clip, elem_first};
        pd::scan_run<pd::OpSum2>(st, E, block, flags, eb::BoundaryStore{flags, spred, bpred, L, d_seg, Y.seg_cap}, (pd::Long2*)sums);
        eb::sort_run(st, blocks, block, elem_first, block_first, C, keys_a, keys_b, y, labels_a, labels_b, table, (unsigned*)sums);
        pd::scan_run<ed::OpHeadNeg>(st, E, block, eb::HeadNegLoad{keys_a, labels_a, elem_clip}, pd::PtrStore<ed::HeadNeg>{scan}, (ed::HeadNeg*)sums);
        hipLaunchKernelGGL(eb::u2_kernel, dim3(grid_for(E)), dim3(256), 0, st, (const uint32_t*)keys_a, (const uint8_t*)labels_a, (const ed::HeadNeg*)scan,
                           (const int*)elem_clip, (const long*)elem_first, E, d_counters);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(counters, d_counters, sizeof(long) * ed::COUNTERS * (size_t)C, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // the first of two
    } else {
        for (long k = 0; k < (long)ed::COUNTERS * C; ++k) counters[k] = 0;
    }
    long n_true = 0;
    seg_first_host[0] = 0;
    for (int c = 0; c < C; ++c) {
        long* mine = counters + (size_t)c * ed::COUNTERS;
        const long n = eb::clip_frames(clip_first_host, label_first_host, c);
        mine[ed::C_N] = n;
        if (mine[ed::C_TRUE] < 0 || mine[ed::C_TRUE] > (n + 1) / 2) return fail(SAVAD_E_STATE, "%ld true segments in the %ld frames of clip %d", mine[ed::C_TRUE], n, c);
        n_true += mine[ed::C_TRUE];
        seg_first_host[c + 1] = n_true;
    }
    if (n_true > seg_cap) return fail(SAVAD_E_INVALID, "%ld true segments, room for %ld", n_true, seg_cap);
    if (n_true > 0) {
        HIP_TRY(hipMemcpyAsync(seg, d_seg, (size_t)ed::SEG_BYTES * (size_t)n_true, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));   // the second
    }
    return n_true;
}

SAVAD_EXPORT long savad_eval_batch_counts_host(const float* probs, const int32_t* clip_first_host, const uint8_t* labels, const int32_t* label_first_host,
                                               int C, int W, float threshold, int L, long* counters, uint8_t* seg, long seg_cap, long* seg_first_host) {
    int rc;
    long E;
    if ((rc = eval_batch_check(clip_first_host, label_first_host, C, W, L, &E))) return rc;
    if (!probs || !labels || !counters || !seg_first_host || seg_cap < 0 || (seg_cap > 0 && !seg)) return fail(SAVAD_E_INVALID, "null pointer");
    const long n_true = eb::counts_host_batch(probs, clip_first_host, labels, label_first_host, C, W, threshold, L, counters, seg, seg_cap, seg_first_host);
    if (n_true > seg_cap) return fail(SAVAD_E_INVALID, "%ld true segments, room for %ld", n_true, seg_cap);
    return n_true;
}

#ifdef SAVAD_TIMING
// experiments only: read the phase stamps of the last row_kernel_m launch
SAVAD_EXPORT int savad_debug_wg_stamps(long long* out, int n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(savad::g_savad_wg), sizeof(long long) * n));
    return SAVAD_OK;
}
SAVAD_EXPORT int savad_debug_stamps(long long* out, int n) {
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out, HIP_SYMBOL(savad::g_savad_dbg), sizeof(long long) * n));
    return SAVAD_OK;
}
#endif
