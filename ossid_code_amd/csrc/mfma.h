// Matrix-core primitives shared by the convolution and weight-gradient kernels (gfx950): operand vector types, the f32 and
// split-bf16 MFMA steps, the row map of a 32x32 accumulator, the split of f32 values into bf16 pieces and, for kernels that
// keep their operands in LDS as [pixel][channel] bf16 images, the store into such images and the transposed operand read.
#pragma once
#include <hip/hip_runtime.h>

typedef float v16f __attribute__((ext_vector_type(16)));
typedef float v4f __attribute__((ext_vector_type(4)));      // (vector arithmetic lowers to v_pk_add_f32 with neg modifiers)
typedef __bf16 v8bf __attribute__((ext_vector_type(8)));
typedef short v4i16 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ v16f mfma(float a, float b, v16f c) {
    return __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, c, 0, 0, 0);
}
// row of register r (0..15) of a 32x32 accumulator in the lanes of wave half `half` (lane >> 5); the column is lane & 31
__device__ __forceinline__ constexpr int acc_row(int r, int half) { return (r & 3) + 8 * (r >> 2) + 4 * half; }

// Split-bf16 arithmetic (csrc/conv.hip: kernel template argument FORM = 1; chosen per launch, see ossid_conv_desc::exact): every f32 operand is a pair
// of bf16 values, x = hi + lo with hi = bf16(x), lo = bf16(x - hi) (16 significant bits together), and a 16-channel slice
// of the reduction is three v_mfma_f32_32x32x16_bf16 -- w_lo*x_hi + w_hi*x_lo + w_hi*x_hi, accumulated in f32 -- instead of
// eight v_mfma_f32_32x32x2_f32: 96 pipe cycles instead of 512. The dropped w_lo*x_lo term is ~2^-16 of a product; measured
// against float64 the results sit at ~5e-6 of the output scale (exact form: ~1e-6), tests hold 2e-5. Weights are split when
// they are packed (csrc/pack.hip), activations when they are staged into LDS ([position][hi of the chunk's
// channels | lo ...] bf16: an MFMA operand is one ds_read_b128 of 8 channels).
// FORM = 2, the three-way split: x = p0 + p1 + p2 with p0 = bf16(x), p1 = bf16(x - p0), p2 = bf16(x - p0 - p1) -- 24
// significant bits, i.e. the f32 value itself up to its last bit -- and six products per slice (all pairs (i, j) with
// i + j <= 2; the dropped ones are <= 2^-24 of a product, the size of f32's own rounding): f32-level accuracy (measured
// like the exact form: ~1e-6 of the output scale) at 192 pipe cycles per 16-channel slice instead of 512. For the layers
// whose output a ReLU / max-pool decides on in training (ossid_conv_desc::exact = 2).
// The ORDER of the products is part of the numerical contract: smallest terms first.
__device__ __forceinline__ v16f mfma3(v8bf ah, v8bf al, v8bf bh, v8bf bl, v16f c) {
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bh, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bl, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bh, c, 0, 0, 0);
}
__device__ __forceinline__ v16f mfma3(const float4& whi, const float4& wlo, const float4& xhi, const float4& xlo, v16f c) {
    return mfma3(__builtin_bit_cast(v8bf, whi), __builtin_bit_cast(v8bf, wlo), __builtin_bit_cast(v8bf, xhi),
                 __builtin_bit_cast(v8bf, xlo), c);
}
__device__ __forceinline__ v16f mfma6(const float4 (&w)[3], const float4& x0, const float4& x1, const float4& x2, v16f c) {
    const v8bf a0 = __builtin_bit_cast(v8bf, w[0]), a1 = __builtin_bit_cast(v8bf, w[1]), a2 = __builtin_bit_cast(v8bf, w[2]);
    const v8bf b0 = __builtin_bit_cast(v8bf, x0), b1 = __builtin_bit_cast(v8bf, x1), b2 = __builtin_bit_cast(v8bf, x2);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a2, b0, c, 0, 0, 0);          // smallest terms first
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b2, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b1, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a1, b0, c, 0, 0, 0);
    c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b1, c, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a0, b0, c, 0, 0, 0);
}

// four floats -> N bf16 quads (8 bytes each): pc[0] = bf16(v), pc[k] = bf16(v - pc[0] - .. - pc[k-1]); N = 2: (hi, lo)
template <int N>
__device__ __forceinline__ void split_bf16(const float (&v)[4], uint2 (&pc)[N]) {
    union {
        __bf16 b[4];
        uint2 u;
    } q[N];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        float r = v[i];
#pragma unroll
        for (int k = 0; k < N; ++k) {
            q[k].b[i] = (__bf16)r;
            r -= (float)q[k].b[i];          // exact: the remainder is representable
        }
    }
#pragma unroll
    for (int k = 0; k < N; ++k) pc[k] = q[k].u;
}

// ---- split-bf16 operands kept in LDS as [pixel][channel] bf16 images, one image per part (hi, lo), `part_stride` bytes apart
// a thread's four channels of one pixel -> the hi quad at hi_at, the lo quad one part further
__device__ __forceinline__ void split_store(const float4& f, char* hi_at, int part_stride) {
    uint2 pc[2];
    split_bf16({f.x, f.y, f.z, f.w}, pc);
    *(uint2*)hi_at = pc[0];
    *(uint2*)(hi_at + part_stride) = pc[1];
}
// The matrix cores want the REDUCTION index (pixels) contiguous per lane, the images have the channels contiguous:
// ds_read_b64_tr_b16 (cdna_hip_programming.md T10) reads a block of 4 pixels x 16 channels and hands lane i the 4 pixels of
// channel i. Within its group of 16 lanes, lane 4q+p supplies the address of block row q (a pixel), channels 4p..4p+3 of the
// block's 16; groups 0 / 1 take channels 0-15 / 16-31 of a 32-channel tile, the wave's halves the pixels 8h..8h+7 of a 16-pixel
// k-step. tr_lane_offset: this lane's byte offset into an image of `pitch` bytes per pixel whose 32-channel tile starts at
// channel `ch0`; a tap's column shift or a later k-step is just more pixels added to it.
__device__ __forceinline__ size_t tr_lane_offset(int lane, int pitch, int ch0) {
    const int tq = (lane >> 2) & 3, tp = lane & 3, tg = (lane >> 4) & 1, h = lane >> 5;
    return (size_t)(8 * h + tq) * pitch + (ch0 + 16 * tg + 4 * tp) * 2;
}
// two blocks of 4 pixels joined: the 8-pixel operand of v_mfma_f32_32x32x16_bf16
__device__ __forceinline__ v8bf tr8(const char* at, int pitch) {
    const v4i16 lo4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)at);
    const v4i16 hi4 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) v4i16*)(at + 4 * pitch));
    typedef short v8i16 __attribute__((ext_vector_type(8)));
    const v8i16 v = __builtin_shufflevector(lo4, hi4, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(v8bf, v);
}
