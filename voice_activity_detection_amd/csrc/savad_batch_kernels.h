// savad_batch_kernels.h -- many clips in one prediction: the predictor's window gather and boosted prediction over a CLIP TABLE.
// clip_first[C + 1] (int32, non-decreasing, clip_first[0] = 0): clip c owns rows [clip_first[c], clip_first[c + 1]) of one
// concatenated feature matrix; it has n_c = max(0, rows - 2 half) windows (vad/predictor.py:169), none of which crosses into a
// neighbour.  items_first[C + 1] = the exclusive prefix sum of n_c: global item g belongs to the clip c with
// items_first[c] <= g < items_first[c + 1] (an empty clip, or one too short for a window, owns no g and is never found).
#pragma once
#include "savad_aux_kernels.h"   // boost_row
#include "savad_device.h"
#include "savad_windows.h"   // the item rule

namespace savad {

constexpr int BATCH_SCAN_THREADS = 256;
constexpr int BATCH_GATHER_ITEMS = 32;  // items per tile of the gather: their clips are searched once, by the tile's first lanes

// index of the last entry <= v (upper_bound - 1) of a non-decreasing table[0 .. n] with table[0] <= v < table[n]
__device__ __forceinline__ int last_not_above(const int32_t* __restrict__ table, int n, int v) {
    int lo = 0, hi = n;  // table[lo] <= v < table[hi]
    while (hi - lo > 1) {
        const int mid = lo + ((hi - lo) >> 1);
        if (table[mid] <= v)
            lo = mid;
        else
            hi = mid;
    }
    return lo;
}

// ---------------------------------------------------------------------------------------------
// clip_first -> items_first.  ONE workgroup: tiles of 256 clips, an inclusive scan of a tile in LDS, the running total carried on.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BATCH_SCAN_THREADS) void clip_items_scan_kernel(const int32_t* __restrict__ clip_first, int C, int half,
                                                                             int32_t* __restrict__ items_first) {
    __shared__ int part[BATCH_SCAN_THREADS];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < C; base += BATCH_SCAN_THREADS) {
        const int c = base + t;
        int n = 0;
        if (c < C) n = (int)windows::items(clip_first[c + 1] - clip_first[c], half);
        part[t] = n;
        __syncthreads();
        for (int d = 1; d < BATCH_SCAN_THREADS; d <<= 1) {
            const int add = t >= d ? part[t - d] : 0;
            __syncthreads();
            part[t] += add;
            __syncthreads();
        }
        if (c < C) items_first[c] = carry + part[t] - n;
        carry += part[BATCH_SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) items_first[C] = carry;
}

// ---------------------------------------------------------------------------------------------
// Window gather (vad/predictor.py:180-220) of the global items [first, first + count): windows[g - first][w][:] =
// feature[clip_first[c] + half + (g - items_first[c]) + off[w]][:], positions = that (global) row.  A workgroup takes tiles of
// BATCH_GATHER_ITEMS items: the tile's first lanes find each item's clip (one search per item) and leave the row of its centre in
// LDS, then all lanes move the tile's pieces -- VEC: 16 bytes each (F a multiple of 4), else one float.
// ---------------------------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void gather_windows_batch_kernel(const float* __restrict__ feature, int F,
                                                                   const int32_t* __restrict__ clip_first,
                                                                   const int32_t* __restrict__ items_first, int C, int half, int first,
                                                                   int count, WindowOffsets wo, float* __restrict__ windows,
                                                                   int64_t* __restrict__ positions) {
    __shared__ int centre[BATCH_GATHER_ITEMS];
    const int pieces = VEC ? F / 4 : F, W = wo.w;
    const int per_item = W * pieces;
    const int tiles = (count + BATCH_GATHER_ITEMS - 1) / BATCH_GATHER_ITEMS;
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int i0 = tile * BATCH_GATHER_ITEMS;
        const int ni = count - i0 < BATCH_GATHER_ITEMS ? count - i0 : BATCH_GATHER_ITEMS;
        if ((int)threadIdx.x < ni) {
            const int g = first + i0 + (int)threadIdx.x;
            const int c = last_not_above(items_first, C, g);
            centre[threadIdx.x] = clip_first[c] + half + (g - items_first[c]);
        }
        __syncthreads();
        const int total = ni * per_item;
        for (int i = threadIdx.x; i < total; i += blockDim.x) {
            const int it = i / per_item, r = i - it * per_item;
            const int wi = r / pieces, p = r - wi * pieces;
            const size_t row = (size_t)(centre[it] + wo.off[wi]);
            const size_t iw = (size_t)(i0 + it) * W + wi;
            move_piece<VEC>(feature + row * F + (VEC ? 4 : 1) * p, windows + iw * F + (VEC ? 4 : 1) * p);
            if (p == 0 && positions) positions[iw] = (int64_t)row;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------
// Boosted prediction (vad/predictor.py:238-258, :95) read as a gather, per clip: row n of clip c (local = n - clip_first[c]) takes
// slot w from the clip's window b = local - half - off[w] when it exists, else (0, 0) -> exactly 0.5.  The arithmetic is
// boost_gather_kernel's (savad_aux_kernels.h: boost_row): a one-clip table gives its bits.
// ---------------------------------------------------------------------------------------------
__global__ void boost_gather_batch_kernel(const float* __restrict__ logp, const int32_t* __restrict__ clip_first,
                                          const int32_t* __restrict__ items_first, int C, int N, int half, WindowOffsets wo,
                                          float* __restrict__ probs, float* __restrict__ mean) {
    const int W = wo.w;
    for (int nrow = blockIdx.x * blockDim.x + threadIdx.x; nrow < N; nrow += gridDim.x * blockDim.x) {
        const int c = last_not_above(clip_first, C, nrow);
        const int local = nrow - clip_first[c], item0 = items_first[c], n_items = items_first[c + 1] - item0;
        boost_row(nrow, W, [&](int wi) {
            const int b = local - half - wo.off[wi];
            f32x2 z = f32x2{0.0f, 0.0f};
            if (b >= 0 && b < n_items) z = *reinterpret_cast<const f32x2*>(logp + ((size_t)(item0 + b) * W + wi) * 2);
            return z;
        }, probs, mean);
    }
}

}  // namespace savad
