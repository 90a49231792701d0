// savad_logmel_batch_plan.h -- the host plan of the log-mel front-end over a CLIP TABLE (one launch sequence for the audio of many
// clips), free of HIP: the table's validation, every count, and the workspace layout the kernels of savad_logmel_batch.h read.
// Plain integer arithmetic; savad.hip launches from it and never reads a count back from the device; tests/logmel_batch_dump.cpp
// includes this header alone.
//
// clips[C] = {first, count}: clip c is samples [first, first + count) of one float32 buffer of audio_count samples.  first is a
// multiple of 4 (the tile DMA reads 16-byte chunks straight from the clip; there is no aligned-copy fall-back here); clips may
// overlap or repeat (they are only read).  count = 0 is a clip without frames, count >= 1 gives 1 + count / 160 frames
// (savad_logmel_frames).  A tile is 32 frames of ONE clip: clip c owns tiles [tiles_first[c], tiles_first[c + 1]) and rows
// [clip_first[c], clip_first[c + 1]) of the feature matrix -- clip_first is the table savad_predict_probabilities_batch takes.
//
// Workspace: tiles_first [C + 1] int32 | head slots [C][HEAD_SLOT] | tail slots [C][TAIL_SLOT] (floats): a clip's mirrored head
// (padded indices [48, 256)) and its run past the last sample (mel::pad_rule), every piece 16-byte aligned.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "savad_audio_host.h"   // HOP, pad_rule and the stretch sizes

namespace savad {
namespace melbatch {

struct Clip {   // savad_audio_clip
    int64_t first, count;
};

constexpr int TILE_FRAMES = 32;
constexpr int HEAD_SLOT = (mel::PAD_A_MAX + 3) & ~3, TAIL_SLOT = (mel::PAD_B_MAX + 3) & ~3;   // floats
constexpr int64_t COUNT_LIMIT = 2000000000, INDEX_LIMIT = 2147483647;                         // savad_logmel_span's; int32 tables

constexpr int64_t frames_of(int64_t count) { return count > 0 ? 1 + count / mel::HOP : 0; }
constexpr int64_t tiles_of(int64_t frames) { return (frames + TILE_FRAMES - 1) / TILE_FRAMES; }
inline size_t up16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Plan {
    int err = 0;           // 0, -1 (SAVAD_E_INVALID) or -2 (SAVAD_E_UNSUPPORTED)
    char msg[160] = {0};
    int C = 0;
    int64_t rows = 0, tiles = 0;
    size_t tiles_first = 0, head = 0, tail = 0, total = 0;   // byte offsets into the workspace
    size_t head_at(int c) const { return head + sizeof(float) * HEAD_SLOT * (size_t)c; }
    size_t tail_at(int c) const { return tail + sizeof(float) * TAIL_SLOT * (size_t)c; }
};

inline Plan refuse(int err, const char* fmt, long long a = 0, long long b = 0, long long c = 0) {
    Plan p;
    p.err = err;
    snprintf(p.msg, sizeof p.msg, fmt, a, b, c);
    return p;
}

// The plan of a table, or its refusal.  clip_first / tiles_first (C + 1 entries each), when given, receive the two prefix sums.
inline Plan plan(const Clip* clips, int C, int64_t audio_count, int32_t* clip_first = nullptr, int32_t* tiles_first = nullptr) {
    if (C < 1 || !clips) return refuse(-1, "an audio clip table needs at least one clip");
    if (audio_count < 0) return refuse(-1, "audio_count = %lld", audio_count);
    Plan p;
    p.C = C;
    for (int c = 0; c < C; ++c) {
        const int64_t first = clips[c].first, count = clips[c].count;
        if (first < 0 || count < 0) return refuse(-1, "clip %lld: first %lld, count %lld", c, first, count);
        if (first > audio_count || count > audio_count - first)
            return refuse(-1, "clip %lld: first %lld + count %lld reaches past the audio", c, first, count);   // (no sum: it may overflow)
        if (first % 4) return refuse(-1, "clip %lld starts at sample %lld: not a multiple of 4 (16-byte reads)", c, first);
        if (count > COUNT_LIMIT) return refuse(-2, "clip %lld holds %lld samples, more than %lld", c, count, COUNT_LIMIT);
        if (clip_first) clip_first[c] = (int32_t)p.rows;
        if (tiles_first) tiles_first[c] = (int32_t)p.tiles;
        p.rows += frames_of(count);
        p.tiles += tiles_of(frames_of(count));
        if (p.rows > INDEX_LIMIT || p.tiles > INDEX_LIMIT)   // (a clip has no more tiles than rows: the first bound is the one met)
            return refuse(-2, "more than 2^31 - 1 feature rows or tiles (at clip %lld)", c);
    }
    if (clip_first) clip_first[C] = (int32_t)p.rows;
    if (tiles_first) tiles_first[C] = (int32_t)p.tiles;
    size_t o = 0;
    p.tiles_first = o, o += up16(sizeof(int32_t) * ((size_t)C + 1));
    p.head = o, o += sizeof(float) * HEAD_SLOT * (size_t)C;
    p.tail = o, o += sizeof(float) * TAIL_SLOT * (size_t)C;
    p.total = o;
    return p;
}

}  // namespace melbatch
}  // namespace savad
