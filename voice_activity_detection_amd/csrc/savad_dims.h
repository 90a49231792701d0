// savad_dims.h -- the sizes that the kernels, the launch schedule (savad_schedule.h) and the weight layout (savad_weights.h) agree on,
// each stated once.  Plain C++17: no HIP, no device code.
#pragma once

#include <stddef.h>

namespace savad {

constexpr int D = 128;        // d_model (= d_head, n_heads = 1: vad/models/self_attention.py:18)
constexpr int DFF = 4 * D;    // vad/models/self_attention.py:10
constexpr int TILE = 32;      // data rows per MFMA tile / per workgroup of the row kernels

// ---- fp32 family (savad_kernels.h)
constexpr int LBIAS = DFF + D + 3 * D + D;                      // a layer's biases, contiguous: b1 | b2 | bqkv | bo
constexpr int FRAG_BLOCK = 4096, FRAG_LAYER = 48 * FRAG_BLOCK;  // floats: a 16 KB weight block in fragment order, a layer's 48 of them
constexpr int PACKED_MAX_LAYERS = 8;  // packed_forward_kernel stages every layer's biases in LDS: 8 x 4.5 KiB behind 87 KiB of exchange buffers

namespace bf {  // bf16 family (savad_kernels_bf16.h, savad_attn_pw_bf16.h, savad_packed_bf16.h)
constexpr int FRAG_BYTES = 1024;             // one K-step fragment of 32 rows: 64 lanes x 16 B
constexpr int BLK_BYTES = 8 * FRAG_BYTES;    // 32 rows x 128 features in bf16
constexpr int HBLK_FLOATS = 32 * D;          // elements of one residual block
constexpr int HRES_BYTES = 2;                // sizeof(hres_t): the residual stream is fp16 between kernels
constexpr int PW_GRID = 256;                 // the persistent attention kernel: one workgroup per CU; must be a multiple of 8 (XCDs)
constexpr int PACKED_BF16_MAX_LAYERS = 6;    // ring (NW = 8: 128 KiB) + 6 x 4.5 KiB of biases fit the 160 KiB of LDS
}  // namespace bf

namespace fs {  // fp32s family (savad_kernels_f32s.h)
constexpr int TFRAG_BYTES = 3 * bf::FRAG_BYTES;  // one triple
constexpr int BLK3_BYTES = 8 * TFRAG_BYTES;      // 32 rows x 128 features as triples: 24 KiB
constexpr int HBLK_BYTES = 32 * D * 4;           // a residual block (fp32)
constexpr int PACKED_F32S_MAX_LAYERS = 3;        // ring (144 KiB) + 3 x 4.5 KiB of biases + the classifier fit the 160 KiB of LDS
}  // namespace fs

namespace gen {  // any d_model (savad_generic.h)
constexpr size_t SCORE_CAP = (size_t)32 << 20;   // floats: 128 MiB of scores per attention pass
}  // namespace gen

}  // namespace savad
