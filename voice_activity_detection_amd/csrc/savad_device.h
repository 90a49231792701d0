// savad_device.h -- the device layer every kernel family is written in: vector types and 16-byte accesses, the exchange between a
// row's two half-lanes, row-layout blocks (bias, residual, LayerNorm), bias staging, the workgroup -> XCD map, the experiment
// switches (SAVAD_TIMING / SAVAD_STAMP, SAVAD_ABLATE, SAVAD_FAULT_INJECT) and the row-chain steps that every family ends or masks
// with (acc_row, packed_key_ok, classify_rows).  The row layout itself is described at the top of savad_kernels.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "savad_dims.h"

namespace savad {

constexpr int XLD = D + 4;    // LDS row stride (floats) of the 32x128 exchange buffer: conflict-free b128
constexpr float LN_EPS = 1e-5f;
constexpr float NEG_BIG = -1.0e30f;
constexpr float RESCALE_LOG2 = 16.0f;  // online softmax: the reference maximum moves only when a row's maximum grew by more than 2^16 (online_softmax)

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define SAVAD_MFMA(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)

__device__ __forceinline__ f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ __forceinline__ void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
// A data row lives in lanes m and m+32: one v_permlane32_swap hands every lane both halves' values
// (no LDS round trip as with ds_bpermute), in the same order on both lanes (bit-identical results).
// NB: copy the two results into scalars before __builtin_bit_cast -- bit_cast applied directly to a
// vector-element lvalue (r[1]) reads element 0 (clang quirk; it cost a parity failure to find).
__device__ __forceinline__ void both_halves(float v, float& lo, float& hi) {
    const unsigned u = __builtin_bit_cast(unsigned, v);
    const auto r = __builtin_amdgcn_permlane32_swap(u, u, false, false);  // r[0] = low half's value, r[1] = high half's
    const unsigned a = r[0], b = r[1];
    lo = __builtin_bit_cast(float, a);
    hi = __builtin_bit_cast(float, b);
}
__device__ __forceinline__ float half_sum(float v) {
    float lo, hi;
    both_halves(v, lo, hi);
    return lo + hi;
}
__device__ __forceinline__ float half_max(float v) {
    float lo, hi;
    both_halves(v, lo, hi);
    return fmaxf(lo, hi);
}

__device__ __forceinline__ f32x16 zero16() {
    f32x16 z;
#pragma unroll
    for (int i = 0; i < 16; ++i) z[i] = 0.0f;
    return z;
}

// bias for the wave's feature block in row layout: b[n0 + 8g + 4h + s]
__device__ __forceinline__ void add_bias(f32x16& acc, const float* __restrict__ b, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = ld4(b + 8 * g + 4 * h);
#pragma unroll
        for (int s = 0; s < 4; ++s) acc[4 * g + s] += b4[s];
    }
}

// element offset of flat row r = b T + t of the features: sequences xbs elements apart (xbs = T F: the contiguous [B,T,F]
// tensor; smaller: overlapping windows read in place out of a feature matrix -- the streaming mode, savad_forward_strided)
__device__ __forceinline__ size_t x_row_offset(size_t r, int T, int F, long xbs) {
    return xbs == (long)T * F ? r * (size_t)F : (r / (size_t)T) * (size_t)xbs + (r % (size_t)T) * (size_t)F;
}

// row-layout 32-feature block <-> memory row (global or LDS): 4 x 16-byte pieces at 8g + 4h
__device__ __forceinline__ void store_block(float* rowp /* &X[row][n0] */, const f32x16& v, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        f32x4 t;
#pragma unroll
        for (int s = 0; s < 4; ++s) t[s] = v[4 * g + s];
        st4(rowp + 8 * g + 4 * h, t);
    }
}
__device__ __forceinline__ void add_block(f32x16& v, const float* rowp, int h) {
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 t = ld4(rowp + 8 * g + 4 * h);
#pragma unroll
        for (int s = 0; s < 4; ++s) v[4 * g + s] += t[s];
    }
}

// LayerNorm (no affine) of full rows held as 4 row-layout blocks -> B-operand registers
__device__ __forceinline__ void layernorm_regs(const f32x16 (&x)[4], f32x4 (&xg)[16]) {
    float s = 0.0f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) s += x[nb][r];
    s = half_sum(s);
    const float mean = s * (1.0f / D);
    float ss = 0.0f;
#pragma unroll
    for (int nb = 0; nb < 4; ++nb)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const float d = x[nb][r] - mean;
            xg[4 * nb + (r >> 2)][r & 3] = d;
            ss += d * d;
        }
    ss = half_sum(ss);
    const float rstd = 1.0f / sqrtf(ss * (1.0f / D) + LN_EPS);
#pragma unroll
    for (int G = 0; G < 16; ++G) xg[G] *= rstd;
}

// Drain this wave's vector-memory operations (global loads AND the LDS-DMA issued through inline asm).
// It must be the BUILTIN, not an asm string: the compiler's wait-count pass cannot see into asm, would
// still believe earlier global loads (e.g. the Q rows read before the key loop) to be pending, and
// would then guard their first use INSIDE the loop with vmcnt(N) waits -- which the hardware counts
// against the DMA just issued for the next tile, exposing its full latency on every iteration.
__device__ __forceinline__ void wait_vmem_all() {
    __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0), expcnt / lgkmcnt untouched (gfx9 encoding)
    asm volatile("" ::: "memory");
}

// Workgroup -> (sequence, index among the sequence's `per_seq` workgroups) for the attention-type kernels.
// Workgroups go to the 8 XCDs round-robin by blockIdx (each XCD has its own L2); the linear order (sequence major)
// is cut into 8 equal chunks, one per XCD, so that a sequence's workgroups -- which all read the same K/V -- share an
// L2 (a sequence straddles at most two XCDs) AND every XCD gets the same number of workgroups for any batch size.
// (Binding whole sequences to XCDs, b = 8 j + xcd, left XCDs 0-1 with twice the work at B = 10: 76 us against 47.)
// Launch 8 * ceil(B * per_seq / 8) workgroups.
__device__ __forceinline__ bool xcd_balanced_map(int B, int per_seq, int& b, int& rr) {
    const long W = (long)B * per_seq;
    const int per_xcd = (int)((W + 7) / 8);
    const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3;
    const long lin = (long)xcd * per_xcd + slot;
    if (slot >= per_xcd || lin >= W) return false;
    b = (int)(lin / per_seq);
    rr = (int)(lin % per_seq);
    return true;
}

// Phase timing (experiments only, scripts/ablate.sh -DSAVAD_TIMING): wave 0 of workgroup 0 stamps
// s_memtime at phase boundaries into g_savad_dbg.
#ifdef SAVAD_TIMING
__device__ long long g_savad_dbg[64];
#define SAVAD_STAMP(i)                                                                  \
    do {                                                                                \
        if (blockIdx.x == 0 && threadIdx.x == 0) g_savad_dbg[i] = __builtin_readcyclecounter(); \
    } while (0)
#else
#define SAVAD_STAMP(i) \
    do {               \
    } while (0)
#endif
// Fault injection for the NEGATIVE tests of the hazard checkers (tests/test_async_load_hazards.py, tests/test_gpu_cache_pressure.py;
// never defined in the product build): bit 1 = the single-launch fp32 forward re-targets the query block's registers (a request
// for the key block) while the query GEMM still reads them: the load lands inside the GEMM on any box, whatever the caches hold
// (until round 6 the fault was a missing wait behind a request one LayerNorm earlier, which an L2 hit survived), bit 16 = the bf16 row chain hands ring
// block 2 over at a barrier without its wait, the DMA issued right in front of it (every wave then reads block 0's bytes), bit 2 = the bf16
// ring GEMMs wait for one LDS fragment too few, bit 4 = the bf16 weight ring skips its workgroup barrier, bit 8 = the ring waits that
// leave a wave's own stores in flight allow one operation too many (the newest DMA piece may not have landed at the barrier).
#ifndef SAVAD_FAULT_INJECT
#define SAVAD_FAULT_INJECT 0
#endif
#ifndef SAVAD_ABLATE
#define SAVAD_ABLATE 0  // experiment switch (scripts/ablate.sh): 1 = no DMA, 2 = no ring barrier, 4 = no softmax, 8 = no LDS operand reads (bf16 attention)
#endif

// Biases live in LDS for the whole kernel (loaded once, published by the first ring barrier): a
// global load inside the block loop would be drained by the ring's vmcnt(0) at full L2 latency,
// once per block.  For the same reason results are stored one block LATE (after the next block's
// barrier), so that a store's write-ack is never waited for.
__device__ __forceinline__ void stage_bias(float* dst, const float* __restrict__ src, int count) {
    for (int i = threadIdx.x * 4; i < count; i += 256 * 4) st4(dst + i, ld4(src + i));
}
// Several pieces at once (each <= 1024 floats, a multiple of 4; count 0 = none): ALL the loads first, then the LDS stores.
// Piece by piece (stage_bias four times in a row) the compiler emits load -> s_waitcnt vmcnt(0) -> ds_write per piece: four
// dependent round trips to the L2 at the start of every row chain, the first of which also drains whatever else the wave has
// in flight (round 5, read off the disassembly; the loads are unconditional -- a lane past a piece's end re-reads its last
// float4 -- so that no branch separates them).
struct BiasPiece {
    float* dst;
    const float* src;
    int count;
};
template <int N>
struct BiasRegs {
    f32x4 v[N];
};
template <int N>
__device__ __forceinline__ BiasRegs<N> request_bias_pieces(const BiasPiece (&p)[N]) {
    const int i = threadIdx.x * 4;
    BiasRegs<N> r;
#pragma unroll
    for (int n = 0; n < N; ++n) {
        const int j = i < p[n].count ? i : (p[n].count >= 4 ? p[n].count - 4 : 0);
        r.v[n] = ld4(p[n].src + j);
    }
    return r;
}
template <int N>
__device__ __forceinline__ void commit_bias_pieces(const BiasPiece (&p)[N], const BiasRegs<N>& r) {
    const int i = threadIdx.x * 4;
#pragma unroll
    for (int n = 0; n < N; ++n)
        if (i < p[n].count) st4(p[n].dst + i, r.v[n]);
}
template <int N>
__device__ __forceinline__ void stage_bias_pieces(const BiasPiece (&p)[N]) {
    commit_bias_pieces(p, request_bias_pieces(p));
}
__device__ __forceinline__ f32x16 bias_block(const float* lds_bias /* &bias[n0] */, int h) {
    f32x16 r;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const f32x4 b4 = ld4(lds_bias + 8 * g + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) r[4 * g + e] = b4[e];
    }
    return r;
}

// window geometry of the predictor (vad/predictor.py:186-212): W relative frame offsets
struct WindowOffsets {
    int w;
    int off[64];
};

// ---- steps of the row chain that every family writes the same way

// MFMA C/D layout: accumulator register r of a lane in half h belongs to row (of the 32) 8 (r >> 2) + 4 h + (r & 3)
__device__ __forceinline__ constexpr int acc_row(int r, int h) { return 8 * (r >> 2) + 4 * h + (r & 3); }

// Block-diagonal key mask of packed block `blk` (floor(32 / T) whole sequences of a batch of B) for the query in slot m: key slot jk
// counts if it is a slot of the block, belongs to the query's own sequence, and that sequence exists.
// One key at a time, jk = acc_row(r, h) for score register r: a form that fills a caller's bool[16] through a reference changed
// register and wait counts in five kernels (scripts/kernel_diff.py); this one leaves them as they were.
__device__ __forceinline__ bool packed_key_ok(int B, int T, int blk, int m, int jk) {
    const int G = 32 / T;
    return (jk < G * T) && (jk / T == m / T) && (blk * G + jk / T < B);
}

// Final LayerNorm rows (affine folded into the classifier) -> Linear(D, 2) -> log-softmax (vad/models/self_attention.py:26-28):
// the two log-probabilities of the lane's row, the same in both of its lanes.  wc: [2][D], bc: [2], global or LDS.
__device__ __forceinline__ f32x2 classify_rows(const f32x4 (&xg)[16], const float* wc, const float* bc, int h) {
    float z0 = 0.0f, z1 = 0.0f;
#pragma unroll
    for (int G = 0; G < 16; ++G) {
        const f32x4 c0 = ld4(wc + 8 * G + 4 * h), c1 = ld4(wc + D + 8 * G + 4 * h);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            z0 = __builtin_fmaf(xg[G][e], c0[e], z0);
            z1 = __builtin_fmaf(xg[G][e], c1[e], z1);
        }
    }
    z0 = half_sum(z0) + bc[0];
    z1 = half_sum(z1) + bc[1];
    const float mx = fmaxf(z0, z1);
    const float lse = mx + logf(expf(z0 - mx) + expf(z1 - mx));
    return f32x2{z0 - lse, z1 - lse};
}

}  // namespace savad
