// savad_live.h -- the kernels of the live mode: one tick for S streams is a fixed number of launches, each reading the tables the
// host plan (savad_live_plan.h) built for the tick: append -> log-mel over the tile table -> window gather over the item table ->
// savad_forward -> log-prob history and boost.  Entries, tiles and items are read-only here; the state they point into is the caller's.
#pragma once
#include "savad_aux_kernels.h"     // boost_row, move_piece
#include "savad_batch_kernels.h"   // last_not_above
#include "savad_live_plan.h"
#include "savad_logmel.h"

namespace savad {
namespace live {

// sample i of an entry's stream as the tick finds it: still in the old buffer, or in the push (PCM16 as savad_pcm16_to_f32 converts it)
__device__ __forceinline__ float sample_at(const Entry& e, long i) {
    if (i < e.n_before) return reinterpret_cast<const float*>(e.buf_old)[i - e.base_before];
    const long k = i - e.n_before;
    return e.dtype ? reinterpret_cast<const float*>(e.src)[k] : reinterpret_cast<const short*>(e.src)[k] * (1.0f / 32768.0f);
}

// ---------------------------------------------------------------------------------------------
// Append: blockIdx.y = entry.  The kept tail moves to the front of the other sample buffer, the push goes behind it (position ==
// index mod 4: base_after is a multiple of 16), and the mirrored stretches of the padded signal are written when the tick needs
// them: [48, 256) with the stream's first frames, the stretch past the last sample at finish (reflect_pad_segments_kernel's rule).
// Everything is read from the old buffer and the push, which nobody writes in this launch.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void append_kernel(const Entry* __restrict__ entries, int n_entries) {
  for (int ei = blockIdx.y; ei < n_entries; ei += gridDim.y) {
    const Entry e = entries[ei];
    float* dst = reinterpret_cast<float*>(e.buf_new);
    const int n_head = e.head_write ? HEAD_FLOATS : 0;
    const int total = e.keep_count + e.push + n_head + e.tail_count;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < total; t += gridDim.x * blockDim.x) {
        if (t < e.keep_count + e.push) {
            dst[t] = sample_at(e, e.base_after + t);
        } else if (t < e.keep_count + e.push + n_head) {
            const int k = t - e.keep_count - e.push;
            reinterpret_cast<float*>(e.head)[k] = sample_at(e, mel::N_FFT / 2 - (HEAD_J0 + k));   // i = j - 256 < 0 -> -i
        } else {
            const int k = t - e.keep_count - e.push - n_head;
            const long n = e.n_after;
            long i = e.tail_j0 + k - mel::N_FFT / 2;
            if (i < 0) i = -i;
            if (i >= n) i = 2L * (n - 1) - i;
            if (i < 0) i = 0;
            if (i >= n) i = n - 1;
            reinterpret_cast<float*>(e.tail)[k] = sample_at(e, i);
        }
    }
  }
}

// ---------------------------------------------------------------------------------------------
// Log-mel over the tile table: the tile loop of logmel_fft_kernel (savad_logmel.h), a tile's place read from the table.
// ---------------------------------------------------------------------------------------------
struct TableTiles {
    const Tile* tab;
    __device__ __forceinline__ mel::FftWhere where(int tile) const {
        const Tile& t = tab[tile];
        return mel::FftWhere{(uintptr_t)t.srcA, (uintptr_t)t.srcB, (uintptr_t)t.srcY, (long)t.J0, (long)t.j_last, (long)t.jA_end, (long)t.jB0};
    }
    __device__ __forceinline__ int room(int tile, int n_tiles) const { return tile < n_tiles ? tab[tile].count - 1 : 0; }
    __device__ __forceinline__ float* rows(int tile) const { return reinterpret_cast<float*>(tab[tile].out); }
};

__global__ __launch_bounds__(256, 1) void logmel_fft_kernel_table(const Tile* __restrict__ tab, int n_tiles, const float* __restrict__ t1,
                                                                  const float* __restrict__ t3, const float* __restrict__ tm) {
    mel::logmel_fft_tiles(TableTiles{tab}, n_tiles, t1, t3, tm);
}

// ---------------------------------------------------------------------------------------------
// Window gather of the items [first, first + count): windows[i - first][w][:] = the row off[w] from the item's centre in its
// stream's feature ring; a dummy item gives zeros.  16-byte pieces (F a multiple of 4).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void gather_items_kernel(const Entry* __restrict__ entries, const Item* __restrict__ items, int F, int cap,
                                                           int first, int count, WindowOffsets wo, float* __restrict__ windows) {
    const int pieces = F / 4, W = wo.w;
    const long total = (long)count * W * pieces;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int p = (int)(i % pieces);
        const long iw = i / pieces;
        const int wi = (int)(iw % W);
        const Item it = items[first + iw / W];
        const float* from = nullptr;
        if (it.entry >= 0) {
            const int row = (it.centre + wo.off[wi] + cap) % cap;
            from = reinterpret_cast<const float*>(entries[it.entry].feat) + (size_t)row * F + 4 * p;
        }
        move_piece<true, true>(from, windows + (size_t)iw * F + 4 * p);
    }
}

// ---------------------------------------------------------------------------------------------
// Log-prob history and boost: output row t (compact, stream order) is row r = t - row_out of its entry, row row_first + r of the
// recording.  Slot w takes window r - half - off[w] counted from the entry's first new window: >= 0 is an item of this tick (when it
// exists), below 0 a window the ring kept (when the recording has it), anything else the (0, 0) placeholder -> exactly 0.5
// (boost_gather_kernel's arithmetic: boost_row).  Row r < n_windows also files window r's log-probs in the ring -- at positions
// no row of this launch reads.
// ---------------------------------------------------------------------------------------------
__global__ void boost_history_kernel(const Entry* __restrict__ entries, const int32_t* __restrict__ row_out, int n_entries, int n_rows,
                                     const float* __restrict__ logp, int half, int cap, WindowOffsets wo, float* __restrict__ probs,
                                     float* __restrict__ mean) {
    const int W = wo.w;
    for (int t = blockIdx.x * blockDim.x + threadIdx.x; t < n_rows; t += gridDim.x * blockDim.x) {
        const int c = last_not_above(row_out, n_entries, t);
        const Entry& e = entries[c];
        const int r = t - e.row_out;
        float* ring = reinterpret_cast<float*>(e.logp);
        boost_row(t, W, [&](int wi) {
            const int b = r - half - wo.off[wi];
            f32x2 z = f32x2{0.0f, 0.0f};
            if (b >= 0) {
                if (b < e.n_windows) z = *reinterpret_cast<const f32x2*>(logp + ((size_t)(e.item0 + b) * W + wi) * 2);
            } else if (b >= -e.win_kept) {
                z = *reinterpret_cast<const f32x2*>(ring + ((size_t)((e.win_first_mod + b + cap) % cap) * W + wi) * 2);
            }
            return z;
        }, probs, mean);
        if (r < e.n_windows)
            for (int wi = 0; wi < W; ++wi)
                *reinterpret_cast<f32x2*>(ring + ((size_t)((e.win_first_mod + r) % cap) * W + wi) * 2) =
                    *reinterpret_cast<const f32x2*>(logp + ((size_t)(e.item0 + r) * W + wi) * 2);
    }
}

}  // namespace live
}  // namespace savad
