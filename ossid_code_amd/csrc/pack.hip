// The packed convolution-weight formats: the ONE writer of the operand layouts that csrc/conv.hip, csrc/wino.hip,
// csrc/dense.hip and csrc/dense_bwd.hip read, and every entry point that sizes or fills them.
//
// Winograd F(2x2, 3x3) filter transform U = G g G^T (G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]) in the packed layout of
// csrc/wino.hip. w is the forward weight [Cout][Cin][3][3]; dgrad != 0 packs the data gradient's layer (M = Cin output
// channels, K = Cout reduction channels, filter rotated by 180 degrees). Element i is one 16-byte unit.
//   split-bf16 form (default):  [ceil(M/32)][K/16][16 xi][2 parts][64 lanes][8 bf16] -- lane (c,h) of (mt, chunk, xi, part)
//       holds U_xi[32mt+c][16chunk+8h+0..7] as bf16: part 0 = hi = bf16(U), part 1 = lo = bf16(U - hi); the kernel forms
//       U*V ~ hi*vh + hi*vl + lo*vh on v_mfma_f32_32x32x16_bf16 (the dropped lo*vl term is ~2^-16 of the product)
//   exact-f32 form (-DOSSID_WINO_F32): [ceil(M/32)][K/8][16 xi][64 lanes][4 floats] -- lane (c,h) of (mt, kb, xi) holds
//       U_xi[32mt+c][8kb+4h+0..3]
// Both have the same size (ossid_conv_wino_packed_floats).
//
// Direct-convolution weights (csrc/conv.hip): element i = one 16-byte unit of the packed layout of a layer with M output and
// K reduction channels. Forward (dgrad == 0): M = Cout, K = Cin, value w[m][k][tap]; data gradient: M = Cin, K = Cout,
// value w[k][m][taps-1-tap] (transposed, rotated by 180 degrees). w is [Cout][Cin][taps].
//   split-bf16 form (default):  [ceil(M/32)][K/16][taps][2 parts][64 lanes][8 bf16] -- lane (c,h) of (mt, u, tap, part) holds
//       W[32mt+c][16u+8h+0..7][tap]: part 0 = hi = bf16(W), part 1 = lo = bf16(W - hi)
//   exact-f32 form (exact == 1; every layer of a -DOSSID_CONV_F32 build): [ceil(M/32)][K/8][taps][64 lanes][4 floats] --
//       lane (c,h) holds W[32mt+c][8kb+4h+0..3][tap]
//   three-way split (exact == 2): as the split form with [3 parts] -- p0 = bf16(W), p1 = bf16(W - p0), p2 = bf16(W - p0 - p1)
// The first two have the same size (ossid_conv_packed_floats), the third 1.5 x that (ossid_conv_packed_floats_form).
#include "common.h"

namespace {

// one (layer, layout) to pack; the rows of ossid_conv_pack_weights_table's device table (ossid_pack_row)
struct PackRow {
    const float* w;
    float4* wpk;
    long long first_block;      // prefix sum of blocks (256 float4 each)
    int Cout, Cin, taps, kind;  // kind 0: forward layout, 1: data-gradient layout, 2 / 3: their Winograd forms, 4 / 5: 0 / 1 for exact-f32 launches, 6 / 7: for three-way-split launches
};
static_assert(sizeof(PackRow) == sizeof(ossid_pack_row), "pack row layout");

#ifdef OSSID_WINO_F32
__device__ __forceinline__ float wino_u(const float* __restrict__ w, int Cout, int Cin, int dgrad, int m, int k, int xi) {
    const int ti = xi >> 2, tj = xi & 3;
    const float* g = dgrad ? w + ((size_t)k * Cin + m) * 9 : w + ((size_t)m * Cin + k) * 9;
    float t[3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        const float g0 = dgrad ? g[8 - b] : g[b], g1 = dgrad ? g[5 - b] : g[3 + b], g2 = dgrad ? g[2 - b] : g[6 + b];
        t[b] = ti == 0 ? g0 : (ti == 1 ? 0.5f * (g0 + g1 + g2) : (ti == 2 ? 0.5f * (g0 - g1 + g2) : g2));
    }
    return tj == 0 ? t[0] : (tj == 1 ? 0.5f * (t[0] + t[1] + t[2]) : (tj == 2 ? 0.5f * (t[0] - t[1] + t[2]) : t[2]));
}

// the exact-f32 Winograd form, one 16-byte unit i
__device__ __forceinline__ float4 wino_pack_quad(const float* __restrict__ w, int Cout, int Cin, int dgrad, size_t i) {
    const int lane = (int)(i & 63);
    size_t r = i >> 6;
    const int K = dgrad ? Cout : Cin, M = dgrad ? Cin : Cout;
    const int xi = (int)(r & 15);
    r >>= 4;
    const int KB = K / 8;
    const int kb = (int)(r % KB), mt = (int)(r / KB);
    const int m = mt * 32 + (lane & 31), k0 = kb * 8 + 4 * (lane >> 5);
    float v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = m < M ? wino_u(w, Cout, Cin, dgrad, m, k0 + e, xi) : 0.0f;
    return make_float4(v[0], v[1], v[2], v[3]);
}
#endif

// TABLE: every convolution weight of the training step packed in ONE launch (forward and data-gradient layouts): `table` has
// one row per (layer, layout): {w, wpk, first block, Cout, Cin, taps, kind}; a block finds its row by binary search.
// !TABLE: one layer, one layout -- the row `one` by value (first_block = 0). One kernel body for both, in the kernel's own
// scope: as an inlined function the same statements compile to other code (fewer instructions, 249 instead of 171 registers).
//
// A thread packs EVERYTHING that derives from one lane's group of reduction channels of one output row: all taps and all
// bf16 pieces (direct layouts), all 16 transform positions and both pieces (Winograd layouts). Round 3 had one thread per
// 16-byte output unit, each gathering its 8 (direct) or 72 (Winograd) source weights again: 2 reads per weight for the direct
// layouts, 32 for the Winograd ones, 4 bytes at a time -- 1.5 ms per step for 0.5 GB of traffic. Here a weight is read once per
// layout (a thread's 8 x taps source values are contiguous in the forward layouts, 8 runs of `taps` in the data-gradient ones),
// and a wave's stores are whole 1 KB units. A row's grid counts 256 output units per block (first_block in a table): a row
// simply needs fewer of its blocks, the rest return at once.
template <bool TABLE>
__global__ __launch_bounds__(256) void pack_kernel(const PackRow* __restrict__ table, int n_rows, const PackRow one) {
    int lo = 0, hi = n_rows - 1;
    const long long b = blockIdx.x;
    while (TABLE && lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_block <= b) lo = mid; else hi = mid - 1;
    }
    const PackRow R = TABLE ? table[lo] : one;
    const size_t i = (size_t)(b - R.first_block) * 256 + threadIdx.x;
    const float* __restrict__ w = R.w;
    const int Cout = R.Cout, Cin = R.Cin;
    if (R.kind == 2 || R.kind == 3) {      // Winograd layouts (csrc/wino.hip)
#ifndef OSSID_WINO_F32
        const int dgrad = R.kind == 3;
        const int K = dgrad ? Cout : Cin, M = dgrad ? Cin : Cout, KC = K / 16, M32 = (M + 31) / 32;
        if (i >= (size_t)M32 * KC * 64) return;
        const int lane = (int)(i & 63);
        const size_t r = i >> 6;
        const int ch = (int)(r % KC), mt = (int)(r / KC);
        const int m = mt * 32 + (lane & 31), k0 = ch * 16 + 8 * (lane >> 5);
        union Oct {
            __bf16 hv[8];
            float4 f;
        } hi_o[16], lo_o[16];
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float g[9];
            if (m < M) {
                const float* src = dgrad ? w + ((size_t)(k0 + e) * Cin + m) * 9 : w + ((size_t)m * Cin + k0 + e) * 9;
#pragma unroll
                for (int t = 0; t < 9; ++t) g[t] = src[t];
            }
#pragma unroll
            for (int xi = 0; xi < 16; ++xi) {
                float u = 0.0f;
                if (m < M) {                                   // U_xi = (G g G^T)[ti][tj], g rotated for the data gradient
                    const int ti = xi >> 2, tj = xi & 3;
                    float t3[3];
#pragma unroll
                    for (int bb = 0; bb < 3; ++bb) {
                        const float g0 = dgrad ? g[8 - bb] : g[bb], g1 = dgrad ? g[5 - bb] : g[3 + bb], g2 = dgrad ? g[2 - bb] : g[6 + bb];
                        t3[bb] = ti == 0 ? g0 : (ti == 1 ? 0.5f * (g0 + g1 + g2) : (ti == 2 ? 0.5f * (g0 - g1 + g2) : g2));
                    }
                    u = tj == 0 ? t3[0] : (tj == 1 ? 0.5f * (t3[0] + t3[1] + t3[2]) : (tj == 2 ? 0.5f * (t3[0] - t3[1] + t3[2]) : t3[2]));
                }
                const __bf16 h = (__bf16)u;
                hi_o[xi].hv[e] = h;
                lo_o[xi].hv[e] = (__bf16)(u - (float)h);
            }
        }
        float4* out = R.wpk + (((size_t)mt * KC + ch) * 16) * 2 * 64 + lane;
#pragma unroll
        for (int xi = 0; xi < 16; ++xi) {
            out[(size_t)(xi * 2 + 0) * 64] = hi_o[xi].f;
            out[(size_t)(xi * 2 + 1) * 64] = lo_o[xi].f;
        }
#else
        const int K8 = (R.kind == 2 ? R.Cin : R.Cout) / 8, M32 = ((R.kind == 2 ? R.Cout : R.Cin) + 31) / 32;
        if (i < (size_t)M32 * K8 * 16 * 64) R.wpk[i] = wino_pack_quad(R.w, R.Cout, R.Cin, R.kind == 3, i);
#endif
        return;
    }
    if (R.kind < 0 || R.kind > 7) return;
    const int dgrad = R.kind & 1, exact = R.kind >= 6 ? 2 : (R.kind >= 4 ? 1 : 0);
    const int taps = R.taps;
    const int K = dgrad ? Cout : Cin, M = dgrad ? Cin : Cout, MT = (M + 31) / 32;
    auto at = [&](int m, int k, int tap) {
        return dgrad ? w[((size_t)k * Cin + m) * taps + (taps - 1 - tap)] : w[((size_t)m * Cin + k) * taps + tap];
    };
    if (OSSID_CONV_SB && exact != 1) {     // split forms: [mt][K/16][taps][parts][64 lanes] x 8 bf16
        const int parts = exact == 2 ? 3 : 2, KU = K / 16;
        if (i >= (size_t)MT * KU * 64) return;
        const int lane = (int)(i & 63);
        const size_t r = i >> 6;
        const int u = (int)(r % KU), mt = (int)(r / KU);
        const int m = mt * 32 + (lane & 31), k0 = u * 16 + 8 * (lane >> 5);
        float4* out = R.wpk + (((size_t)mt * KU + u) * taps) * parts * 64 + lane;
        for (int tap = 0; tap < taps; ++tap) {
            union {
                __bf16 hv[8];
                float4 f;
            } o[3];
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float v = m < M ? at(m, k0 + e, tap) : 0.0f;
#pragma unroll
                for (int p = 0; p < 3; ++p) {
                    const __bf16 pc = (__bf16)v;
                    o[p].hv[e] = pc;
                    v -= (float)pc;
                }
            }
            for (int p = 0; p < parts; ++p) out[((size_t)tap * parts + p) * 64] = o[p].f;
        }
        return;
    }
    {                                      // exact-f32 form: [mt][K/8][taps][64 lanes] x 4 floats
        const int KB = K / 8;
        if (i >= (size_t)MT * KB * 64) return;
        const int lane = (int)(i & 63);
        const size_t r = i >> 6;
        const int kb = (int)(r % KB), mt = (int)(r / KB);
        const int m = mt * 32 + (lane & 31), k0 = kb * 8 + 4 * (lane >> 5);
        float4* out = R.wpk + (((size_t)mt * KB + kb) * taps) * 64 + lane;
        for (int tap = 0; tap < taps; ++tap) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = m < M ? at(m, k0 + e, tap) : 0.0f;
            out[(size_t)tap * 64] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// the one-row launch: as many blocks as the layout has 256-unit pieces, like a table row
int pack_one(const float* w, int Cout, int Cin, int taps, int kind, float* wpk, size_t packed_floats, void* stream) {
    const PackRow R = {w, (float4*)wpk, 0, Cout, Cin, taps, kind};
    hipLaunchKernelGGL(pack_kernel<false>, dim3((unsigned)((packed_floats / 4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream, nullptr, 0, R);
    return ossid_launch_status();
}

}  // namespace

extern "C" {

size_t ossid_conv_packed_floats(int Cout, int Cin, int taps) {
    return (size_t)((Cout + 31) / 32) * (Cin / 8) * taps * 64 * 4;
}

size_t ossid_conv_packed_floats_form(int Cout, int Cin, int taps, int exact) {
    const size_t n = ossid_conv_packed_floats(Cout, Cin, taps);
    return (exact == 2 && OSSID_CONV_SB) ? n / 2 * 3 : n;       // three pieces per value instead of two
}

int ossid_conv_pack_weights_form(const float* w, int Cout, int Cin, int taps, int dgrad, int exact, float* wpk, void* stream) {
    if (!w || !wpk || Cout <= 0 || Cin <= 0 || (dgrad ? Cout : Cin) % 16 || (taps != 1 && taps != 9 && taps != 4)) return OSSID_EINVAL;
    if (exact < 0 || exact > 2) return OSSID_EINVAL;
    const size_t n = dgrad ? ossid_conv_packed_floats_form(Cin, Cout, taps, exact) : ossid_conv_packed_floats_form(Cout, Cin, taps, exact);
    return pack_one(w, Cout, Cin, taps, (dgrad ? 1 : 0) + (exact == 1 ? 4 : (exact == 2 ? 6 : 0)), wpk, n, stream);
}

int ossid_conv_pack_weights(const float* w, int Cout, int Cin, int taps, float* wpk, void* stream) {
    return ossid_conv_pack_weights_form(w, Cout, Cin, taps, 0, 0, wpk, stream);
}

int ossid_conv_pack_weights_dgrad(const float* w, int Cout, int Cin, int taps, float* wpk, void* stream) {
    if (taps != 1 && taps != 9) return OSSID_EINVAL;
    return ossid_conv_pack_weights_form(w, Cout, Cin, taps, 1, 0, wpk, stream);
}

size_t ossid_conv_wino_packed_floats(int Cout, int Cin) {
    return (size_t)((Cout + 31) / 32) * (Cin / 8) * 16 * 64 * 4;
}

// U = G g G^T packed as csrc/wino.hip streams it. dgrad != 0: the weights of the data gradient (the transposed layer:
// output channels = the forward's inputs, filter rotated by 180 degrees), w stays the forward [Cout][Cin][3][3].
int ossid_conv_pack_weights_wino(const float* w, int Cout, int Cin, int dgrad, float* wpk, void* stream) {
    if (!w || !wpk || Cout <= 0 || Cin <= 0 || (dgrad ? Cout : Cin) % 16) return OSSID_EINVAL;
    const size_t n = dgrad ? ossid_conv_wino_packed_floats(Cin, Cout) : ossid_conv_wino_packed_floats(Cout, Cin);
    return pack_one(w, Cout, Cin, 9, dgrad ? 3 : 2, wpk, n, stream);
}

int ossid_conv_pack_weights_table(const ossid_pack_row* rows_device, int n_rows, long long total_blocks, void* stream) {
    if (!rows_device || n_rows <= 0 || total_blocks <= 0 || total_blocks > 0x7fffffffLL) return OSSID_EINVAL;
    hipLaunchKernelGGL(pack_kernel<true>, dim3((unsigned)total_blocks), dim3(256), 0, (hipStream_t)stream,
                       (const PackRow*)rows_device, n_rows, PackRow{});
    return ossid_launch_status();
}

}  // extern "C"
