// savad_logmel_batch.h -- the log-mel front-end over a CLIP TABLE: the features of every clip of a batch in three launches,
// whatever the number of clips (host plan and workspace layout: savad_logmel_batch_plan.h).
//   clip_frames_scan_kernel    the device copy of the table -> clip_first [C + 1] (rows; the table the batched prediction takes) and
//                              tiles_first [C + 1]
//   reflect_pad_clips_kernel   every clip's mirrored head and its run past the last sample into the clip's two slots: the stretches
//                              reflect_pad_segments_kernel writes on the direct path of savad_logmel_span (mel::pad_rule, mel::pad_source)
//   logmel_fft_kernel_clips    the tile loop of logmel_fft_kernel (savad_logmel.h) with a provider that finds a tile's clip in
//                              tiles_first: a frame's bits depend on nothing but its own 400 samples, so a clip's rows are those of
//                              savad_logmel on the clip alone
// The only ordering between workgroups is the boundary between the launches.
#pragma once
#include "savad_batch_kernels.h"   // last_not_above, BATCH_SCAN_THREADS
#include "savad_logmel.h"
#include "savad_logmel_batch_plan.h"

namespace savad {
namespace melbatch {

// ---------------------------------------------------------------------------------------------
// clips -> clip_first, tiles_first.  ONE workgroup, the pattern of clip_items_scan_kernel: tiles of 256 clips, an inclusive scan of
// a tile in LDS (rows and tiles side by side), the running totals carried on.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BATCH_SCAN_THREADS) void clip_frames_scan_kernel(const Clip* __restrict__ clips, int C,
                                                                              int32_t* __restrict__ clip_first,
                                                                              int32_t* __restrict__ tiles_first) {
    __shared__ int rows[BATCH_SCAN_THREADS], tiles[BATCH_SCAN_THREADS];
    const int t = threadIdx.x;
    int carry_rows = 0, carry_tiles = 0;
    for (int base = 0; base < C; base += BATCH_SCAN_THREADS) {
        const int c = base + t;
        int nr = 0, nt = 0;
        if (c < C) {
            nr = (int)frames_of(clips[c].count);
            nt = (int)tiles_of(nr);
        }
        rows[t] = nr;
        tiles[t] = nt;
        __syncthreads();
        for (int d = 1; d < BATCH_SCAN_THREADS; d <<= 1) {
            const int add_r = t >= d ? rows[t - d] : 0, add_t = t >= d ? tiles[t - d] : 0;
            __syncthreads();
            rows[t] += add_r;
            tiles[t] += add_t;
            __syncthreads();
        }
        if (c < C) {
            clip_first[c] = carry_rows + rows[t] - nr;
            tiles_first[c] = carry_tiles + tiles[t] - nt;
        }
        carry_rows += rows[BATCH_SCAN_THREADS - 1];
        carry_tiles += tiles[BATCH_SCAN_THREADS - 1];
        __syncthreads();
    }
    if (t == 0) {
        clip_first[C] = carry_rows;
        tiles_first[C] = carry_tiles;
    }
}

// ---------------------------------------------------------------------------------------------
// The two stretches of every clip: element e of clip c's HEAD_SLOT + TAIL_SLOT floats is padded index a_j0 + e of the head, or
// b_j0 + (e - HEAD_SLOT) of the tail, where the clip's frames read it; nothing else is written.  A clip without frames has neither.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reflect_pad_clips_kernel(const float* __restrict__ audio, const Clip* __restrict__ clips, int C,
                                                                float* __restrict__ head, float* __restrict__ tail) {
    constexpr int PER_CLIP = HEAD_SLOT + TAIL_SLOT;
    const long total = (long)C * PER_CLIP;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (long)gridDim.x * blockDim.x) {
        const int c = (int)(t / PER_CLIP), e = (int)(t - (long)c * PER_CLIP);
        const long n = clips[c].count;
        if (n < 1) continue;
        const mel::PadRule r = mel::pad_rule(n, 0, frames_of(n));
        const float* y0 = audio + clips[c].first;
        if (e < HEAD_SLOT) {
            if (e < r.a_count) head[(size_t)c * HEAD_SLOT + e] = y0[mel::pad_source(r.a_j0 + e, n)];
        } else if (e - HEAD_SLOT < r.b_count) {
            tail[(size_t)c * TAIL_SLOT + (e - HEAD_SLOT)] = y0[mel::pad_source(r.b_j0 + (e - HEAD_SLOT), n)];
        }
    }
}

// ---------------------------------------------------------------------------------------------
// The tiles of a clip table: tile t is the t_local-th of the clip c with tiles_first[c] <= t < tiles_first[c + 1] (a clip without
// frames owns no tile and is never found); everything wave-uniform.  where, room and rows each search tiles_first on their own: four
// or five searches of log2(C) dependent loads per tile and wave, beside the tile's ~900 MFMAs.  Their cost has NOT been measured on
// its own (it is inside the end-to-end figures of DESIGN section 4o); it weighs most where tiles hold one or two frames.
// ---------------------------------------------------------------------------------------------
struct ClipTiles {
    const float* audio;
    const Clip* clips;
    const int32_t* clip_first;
    const int32_t* tiles_first;
    int C;
    const float* head;
    const float* tail;
    float* features;
    __device__ __forceinline__ mel::FftWhere where(int tile) const {
        const int c = last_not_above(tiles_first, C, tile), t_local = tile - tiles_first[c];
        const long n = clips[c].count;
        const mel::PadRule r = mel::pad_rule(n, 0, frames_of(n));   // the whole clip's: its head is A, its tail B
        return mel::FftWhere{(uintptr_t)(head + (size_t)c * HEAD_SLOT) - 4 * (uintptr_t)r.a_j0, (uintptr_t)(tail + (size_t)c * TAIL_SLOT) - 4 * (uintptr_t)r.b_j0,
                             (uintptr_t)(audio + clips[c].first) - 4 * (uintptr_t)(mel::N_FFT / 2), (long)mel::HOP * TILE_FRAMES * t_local + 48,
                             r.j_last, r.a_end, r.b_j0};
    }
    // frames of the tile - 1: what is left of its clip (not clamped above); 0 past the last tile
    __device__ __forceinline__ int room(int tile, int n_tiles) const {
        if (tile >= n_tiles) return 0;
        const int c = last_not_above(tiles_first, C, tile);
        return (int)frames_of(clips[c].count) - 1 - TILE_FRAMES * (tile - tiles_first[c]);
    }
    __device__ __forceinline__ float* rows(int tile) const {
        const int c = last_not_above(tiles_first, C, tile);
        return features + ((size_t)clip_first[c] + (size_t)TILE_FRAMES * (tile - tiles_first[c])) * mel::N_MELS;
    }
};

__global__ __launch_bounds__(256, 1) void logmel_fft_kernel_clips(const float* __restrict__ audio, const Clip* __restrict__ clips,
                                                                  const int32_t* __restrict__ clip_first, const int32_t* __restrict__ tiles_first,
                                                                  int C, int n_tiles, const float* __restrict__ head, const float* __restrict__ tail,
                                                                  const float* __restrict__ t1, const float* __restrict__ t3,
                                                                  const float* __restrict__ tm, float* __restrict__ features) {
    mel::logmel_fft_tiles(ClipTiles{audio, clips, clip_first, tiles_first, C, head, tail, features}, n_tiles, t1, t3, tm);
}

}  // namespace melbatch
}  // namespace savad
