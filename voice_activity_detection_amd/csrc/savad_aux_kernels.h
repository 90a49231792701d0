// savad_aux_kernels.h -- the kernels around the forward pass: weight preparation (fragment order, LayerNorm folding), the
// predictor's window gather / boosting / overlap merge, and the zero-padding of feature rows.
#pragma once
#include "savad_device.h"

namespace savad {

// ---------------------------------------------------------------------------------------------
// Weight preparation: fold a LayerNorm's affine parameters into the Linear that consumes it:
//   LN(x) W^T + b = xhat (W diag(gamma))^T + (b + W beta)
// One block per output row; beta term accumulated in fp64.
// ---------------------------------------------------------------------------------------------
// fp32 weights in fragment order (PackedLayer::frag).  mode 0: `count` row blocks of W [32 count][128] (register i =
// k-chunk G: W[32 b + n][8 G + 4 h + e]); mode 1: `count` column blocks of W2 [128][512] (register i = 4 nb + g:
// W2[32 nb + n][32 b + 8 g + 4 h + e]).
__global__ void pack_frag32_kernel(const float* __restrict__ W, int mode, int count, float* __restrict__ out) {
    const size_t total = (size_t)count * FRAG_BLOCK;
    for (size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
        const int b = (int)(idx / FRAG_BLOCK), r = (int)(idx % FRAG_BLOCK);
        const int i = r >> 8, lane = (r >> 2) & 63, e = r & 3, n = lane & 31, h = lane >> 5;
        out[idx] = mode == 0 ? W[(size_t)(32 * b + n) * D + 8 * i + 4 * h + e]
                             : W[(size_t)(32 * (i >> 2) + n) * DFF + 32 * b + 8 * (i & 3) + 4 * h + e];
    }
}

__global__ void fold_ln_kernel(const float* __restrict__ W, const float* __restrict__ b, const float* __restrict__ gamma,
                               const float* __restrict__ beta, float* __restrict__ Wout, float* __restrict__ bout,
                               int K) {
    __shared__ double red[256];
    const int nrow = blockIdx.x;
    double acc = 0.0;
    for (int kk = threadIdx.x; kk < K; kk += blockDim.x) {
        const float wv = W[(size_t)nrow * K + kk];
        Wout[(size_t)nrow * K + kk] = wv * gamma[kk];
        acc += (double)wv * (double)beta[kk];
    }
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int st = blockDim.x / 2; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) red[threadIdx.x] += red[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) bout[nrow] = (float)((double)b[nrow] + red[0]);
}

// ---------------------------------------------------------------------------------------------
// a13: window gather (vad/predictor.py:180-220).  One thread per output float4.
// ---------------------------------------------------------------------------------------------
// one piece of a window row, 16 bytes (VEC) or one float, from `from` to `to`: what every window gather moves (DUMMIES: a null
// `from` gives zeros)
template <bool VEC, bool DUMMIES = false>
__device__ __forceinline__ void move_piece(const float* __restrict__ from, float* __restrict__ to) {
    if (VEC)
        st4(to, !DUMMIES || from ? ld4(from) : f32x4{0.0f, 0.0f, 0.0f, 0.0f});
    else
        *to = !DUMMIES || from ? *from : 0.0f;
}
__global__ void gather_windows_kernel(const float* __restrict__ feature, int F, int half, int first, int count,
                                      WindowOffsets wo, float* __restrict__ windows, int64_t* __restrict__ positions) {
    const int f4 = F / 4;
    const size_t total = (size_t)count * wo.w * f4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % f4);
        const size_t iw = i / f4;
        const int wi = (int)(iw % wo.w);
        const size_t item = iw / wo.w;
        const size_t pos = (size_t)half + first + item + wo.off[wi];
        move_piece<true>(feature + pos * F + 4 * c, windows + iw * F + 4 * c);
        if (c == 0 && positions) positions[iw] = (int64_t)pos;
    }
}

// the same for a feature size that is not a multiple of 4 (the MFCC / spectrogram front-ends: 13, 39, 161 ...): one float per thread
__global__ void gather_windows_scalar_kernel(const float* __restrict__ feature, int F, int half, int first, int count,
                                             WindowOffsets wo, float* __restrict__ windows, int64_t* __restrict__ positions) {
    const size_t total = (size_t)count * wo.w * F;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % F);
        const size_t iw = i / F;
        const int wi = (int)(iw % wo.w);
        const size_t item = iw / wo.w;
        const size_t pos = (size_t)half + first + item + wo.off[wi];
        move_piece<false>(feature + pos * F + c, windows + i);
        if (c == 0 && positions) positions[iw] = (int64_t)pos;
    }
}

// ---------------------------------------------------------------------------------------------
// a14: boosted prediction (vad/predictor.py:238-258, :95): scatter, then softmax[...,1] and mean.
// ---------------------------------------------------------------------------------------------
__global__ void boost_scatter_kernel(const float* __restrict__ logp, const int64_t* __restrict__ positions,
                                     size_t count_w, int W, float* __restrict__ boosted) {
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count_w; i += (size_t)gridDim.x * blockDim.x) {
        const int wi = (int)(i % W);
        const size_t p = (size_t)positions[i];
        *reinterpret_cast<f32x2*>(boosted + (p * W + wi) * 2) = *reinterpret_cast<const f32x2*>(logp + i * 2);
    }
}
__global__ void boost_softmax_kernel(const float* __restrict__ boosted, int N, int W, float* __restrict__ probs,
                                     float* __restrict__ mean) {
    for (int nrow = blockIdx.x * blockDim.x + threadIdx.x; nrow < N; nrow += gridDim.x * blockDim.x) {
        float acc = 0.0f;
        for (int wi = 0; wi < W; ++wi) {
            const f32x2 z = *reinterpret_cast<const f32x2*>(boosted + ((size_t)nrow * W + wi) * 2);
            const float mx = fmaxf(z[0], z[1]);
            const float e0 = expf(z[0] - mx), e1 = expf(z[1] - mx);
            const float p = e1 / (e0 + e1);
            probs[(size_t)nrow * W + wi] = p;
            acc += p;
        }
        if (mean) mean[nrow] = acc / (float)W;
    }
}

// softmax(z)[1] of one slot's (log p0, log p1): the arithmetic every boost kernel that reads slots as a gather shares
__device__ __forceinline__ float boost_slot(f32x2 z) {
    const float mx = fmaxf(z[0], z[1]);
    const float e0 = expf(z[0] - mx), e1 = expf(z[1] - mx);
    return e1 / (e0 + e1);
}

// One output row of every such kernel: slot(w) names the (log p0, log p1) of slot w, or the (0, 0) placeholder -> exactly 0.5;
// the row's W probabilities are stored and summed in slot order, the mean is the sum over W.  The kernels differ only in `slot`.
template <class Slot>
__device__ __forceinline__ void boost_row(int row, int W, Slot slot, float* __restrict__ probs, float* __restrict__ mean) {
    float acc = 0.0f;
    for (int wi = 0; wi < W; ++wi) {
        const float p = boost_slot(slot(wi));
        probs[(size_t)row * W + wi] = p;
        acc += p;
    }
    if (mean) mean[row] = acc / (float)W;
}

// The same result as scatter + softmax, read the other way round: slot (n, w) of the boosted array was written by
// window b = n - half - off[w] if that window exists, else it still holds (0, 0) -> 0.5.  Same arithmetic on the same
// values, no memset, no scatter launch, no positions array.
__global__ void boost_gather_kernel(const float* __restrict__ logp, int n_items, int N, int half, WindowOffsets wo,
                                    float* __restrict__ probs, float* __restrict__ mean) {
    const int W = wo.w;
    for (int nrow = blockIdx.x * blockDim.x + threadIdx.x; nrow < N; nrow += gridDim.x * blockDim.x) {
        boost_row(nrow, W, [&](int wi) {
            const int b = nrow - half - wo.off[wi];
            f32x2 z = f32x2{0.0f, 0.0f};
            if (b >= 0 && b < n_items) z = *reinterpret_cast<const f32x2*>(logp + ((size_t)b * W + wi) * 2);
            return z;
        }, probs, mean);
    }
}

// ---------------------------------------------------------------------------------------------
// Streaming long-form mode (BASELINE configs[4]; not a reference mode -- the reference would cut
// 7-frame windows): window w covers frames [hop*w, hop*w + T) of feature[N][F], zero-padded past N.
// ---------------------------------------------------------------------------------------------
__global__ void gather_strided_kernel(const float* __restrict__ feature, int N, int F, int T, int hop, int first,
                                      int count, float* __restrict__ windows) {
    const int f4 = F / 4;
    const size_t total = (size_t)count * T * f4;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % f4);
        const size_t wt = i / f4;
        const int t = (int)(wt % T);
        const size_t wi = wt / T;
        const long frame = (long)hop * (long)(first + wi) + t;
        f32x4 val = f32x4{0.f, 0.f, 0.f, 0.f};
        if (frame < N) val = ld4(feature + (size_t)frame * F + 4 * c);
        st4(windows + wt * F + 4 * c, val);
    }
}
// probs[n] = mean over the windows w covering frame n (hop*w <= n < hop*w + T, 0 <= w < W) of
// softmax(logp[w][n - hop*w])[1]
__global__ void overlap_merge_kernel(const float* __restrict__ logp, int W, int N, int T, int hop,
                                     float* __restrict__ probs) {
    for (int nrow = blockIdx.x * blockDim.x + threadIdx.x; nrow < N; nrow += gridDim.x * blockDim.x) {
        int w_hi = nrow / hop;
        if (w_hi > W - 1) w_hi = W - 1;
        float acc = 0.0f;
        int cnt = 0;
        for (int wi = w_hi; wi >= 0 && nrow - hop * wi < T; --wi) {
            const f32x2 z = *reinterpret_cast<const f32x2*>(logp + ((size_t)wi * T + (nrow - hop * wi)) * 2);
            const float mx = fmaxf(z[0], z[1]);
            const float e0 = expf(z[0] - mx), e1 = expf(z[1] - mx);
            acc += e1 / (e0 + e1);
            ++cnt;
        }
        probs[nrow] = cnt ? acc / (float)cnt : 0.5f;
    }
}

// ---------------------------------------------------------------------------------------------
// Arbitrary feature sizes (the reference's transforms give 80 mels, 257 spectrogram bins, n_mfcc ...):
// the MFMA kernels read K in groups of 8 (fp32) / 16 (bf16) with 16-byte loads, so rows are zero-padded
// to FP = round_up(F, 16) when F is not a multiple of 16: the input weight once (prepare_weights), the
// features once per forward.
// ---------------------------------------------------------------------------------------------
template <typename T>
__global__ void pad_rows_kernel(const T* __restrict__ src, size_t rows, int F, int FP, float* __restrict__ dst) {
    const size_t total = rows * (size_t)FP;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % FP);
        const size_t r = i / FP;
        dst[i] = c < F ? (float)src[r * F + c] : 0.0f;
    }
}

}  // namespace savad
