// PointNet++ (SSG) hypothesis scorer for gfx950: furthest-point sampling, ball query, and the three
// set-abstraction MLPs + FC head on the f32 matrix cores (v_mfma_f32_32x32x2_f32).
//
// Stands behind zephyr.models.pointnet2.PointNet2SSG.forward({"point_x": ...})
// (ctor /root/reference/python/ossid/scripts/online_learning.py:212-227, call
// utils/zephyr_utils.py:34); the algorithm is pointnet2_ops v3.0.0's, restated in SPEC.md 4 and
// oracle/zephyr_oracle.c. Results are bit-identical to the oracle: each output is ONE fmaf chain
// started from the folded bias, walking input channels in the canonical order (8-blocks
// ascending, offsets 0,4,1,5,2,6,3,7) -- which is exactly what a chain of 32x32x2 f32 MFMAs
// produces when lane half h supplies channel 8b+4h+i at step i: D = fma(a_k1,b_k1,fma(a_k0,b_k0,C)).
//
// MLP design (sa1/sa2/sa3 kernels): samples sit on the MFMA N axis (lane&31), channels on M.
// A layer's 32x32 accumulator tile IS the next layer's B operand (register r of lane half h holds
// channel (r&3)+8(r>>2)+4h), so activations never leave the register file between layers: no LDS,
// no barriers, 64-wide waves each carrying 32 samples. Weights are pre-packed on the host so one
// coalesced 16-B load per lane feeds four MFMAs. The max-pool over a group's samples is a
// butterfly reduce-scatter across the 32 lanes (16 shuffles per 32 channels).
#include "common.h"
#include "mfma.h"
#include "slice_balance.h"
#include "workgroup.h"

namespace {

// accumulator tile initialised with the folded bias: register 4q+e of lane half h <- b[32mt+8q+4h+e]
__device__ __forceinline__ v16f bias_tile(const float* __restrict__ b, int mt, int h) {
    v16f acc;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        float4 t = *(const float4*)(b + mt * 32 + 8 * q + 4 * h);
        acc[4 * q + 0] = t.x;
        acc[4 * q + 1] = t.y;
        acc[4 * q + 2] = t.z;
        acc[4 * q + 3] = t.w;
    }
    return acc;
}

// max of two floats as ONE instruction. fmaxf() on an MFMA result costs two: the compiler cannot prove the value is not a
// signalling NaN and puts a canonicalising v_max_f32 x, x in front of the real one. v_med3_f32 with +inf as third operand
// returns the hardware's own MAX(a, b) (and MIN3 = the non-NaN operand when one is a NaN, as v_max_f32 does), so the value
// is the same in every case, signed zeros and NaNs included. It matters because a vector instruction does not hide beside
// an f32 MFMA: each one takes about four cycles out of the matrix stream (profiles/r08_sa1_after.txt).
// (The +inf goes through an empty asm into a scalar register: given the literal, the compiler folds the median back into
// fmaxf and its canonicalisation. The statement is not volatile, so one copy per kernel survives.)
__device__ __forceinline__ float max1(float a, float b) {
    float inf = __builtin_inff();
    asm("" : "+s"(inf));
    return __builtin_amdgcn_fmed3f(a, b, inf);
}

__device__ __forceinline__ v16f relu16(v16f a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = max1(a[i], 0.0f);
    return a;
}

// Launder the weight pointers once per loop iteration: without it LICM hoists every weight load of a fully
// unrolled layer out of the enclosing tile/centre loop -- the whole weight set -- and spills it. The laundering is an
// opaque ZERO added to the pointer (an SGPR the compiler cannot see through), so the pointer keeps its global
// address space (laundering the pointer itself degrades every load to flat_load).
__device__ __forceinline__ int opaque_zero() {
    int z = 0;
    asm volatile("" : "+s"(z));
    return z;
}
template <class T>
__device__ __forceinline__ const T* opaque(const T* p) {
    return p + opaque_zero();
}

// four chained MFMAs: one packed weight quad against registers 4q..4q+3 of an activation tile
__device__ __forceinline__ v16f mfma4(float4 a, const v16f& x, int q4, v16f acc) {
    acc = mfma(a.x, x[q4 + 0], acc);
    acc = mfma(a.y, x[q4 + 1], acc);
    acc = mfma(a.z, x[q4 + 2], acc);
    acc = mfma(a.w, x[q4 + 3], acc);
    return acc;
}

// ---- weight streaming --------------------------------------------------------------------------------
// A layer's packed weights are one linear sequence of "quads" (a float4 per lane = the A operands of four
// chained MFMAs), ordered [m-tile][k-block]. hipcc left alone hoists every load of a fully unrolled
// layer to the top and spills hundreds of registers, so the stream is cut into groups of G quads with
// an explicit two-deep register pipeline: group g+1 is loaded while group g feeds the matrix core, and a
// sched_barrier between groups keeps the compiler from re-merging them (G quads = 4G MFMAs = 256G cycles
// of matrix work cover the L2 latency of the next group's loads).

// A weight load of the two forms sa3_kernel uses is ONE global_load_dwordx4 with no address arithmetic in the vector pipe:
// a group of G <= 8 consecutive quads shares a base in scalar registers (the layer's uniform pointer plus the group's
// offset, one scalar add per group), the lane's 16-byte slot is a 32-bit offset register computed once per kernel, and
// the quad's place in the group is the instruction's immediate (13 bits, signed: the base points at the group's middle).
// The group's offset goes through an empty asm: seen through, the compiler folds lane and base into one 64-bit vector pointer per
// kernel and then adds every group's offset to it with a v_add_co / v_addc pair.
// s_waitcnt operand that waits for the vector-memory counter alone (gfx9 encoding: vmcnt in bits 3:0 and 15:14, the
// export and LDS / scalar counters at their maxima = not waited for)
constexpr int vmcnt_only(int n) { return (n & 15) | ((n >> 4) << 14) | 0x0F70; }

template <int G>
__device__ __forceinline__ const char* group_base(const float* __restrict__ Wu, int quad0) {
    static_assert(G <= 8, "a group must fit the immediate offset");
    int off = quad0 * 1024 + (G > 4 ? 4096 : 0);
    asm("" : "+s"(off));               // (the offset, not the pointer: a laundered pointer loses its address space)
    return (const char*)Wu + off;
}
template <int G>
__device__ __forceinline__ float4 load_quad(const char* gb, unsigned lane_off, int i) {
    return *(const float4*)(gb + lane_off + (i * 1024 - (G > 4 ? 4096 : 0)));
}

// Fully unrolled form for layers whose output tiles stay in registers (Y[t][mt] statically indexed).
template <int KT, int MT, int NT, int G, class Epi>
__device__ __forceinline__ void stream_layer(const float* __restrict__ Wu, unsigned lane_off, const float* __restrict__ bias,
                                             const v16f (&X)[NT][KT], int h, Epi&& epi) {
    constexpr int QPM = KT * 4, TOTAL = MT * QPM, NG = TOTAL / G, NGM = QPM / G;
    static_assert(QPM % G == 0 && NGM >= 2, "an m-tile must be at least two whole groups");
    float4 cur[G], nxt[G];
    {
        const char* gb = group_base<G>(Wu, 0);
#pragma unroll
        for (int i = 0; i < G; ++i) cur[i] = load_quad<G>(gb, lane_off, i);
    }
    // the bias tile of an m-tile is fetched with the weights of its first group, a group ahead (its one consumer, the
    // m-tile's first MFMA, would otherwise sit on an L2 latency sixteen times per layer)
    v16f bt = bias_tile(bias, 0, h);
    v16f acc[NT];
#pragma unroll
    for (int g = 0; g < NG; ++g) {
        const bool more = g + 1 < NG, bias_too = more && (g + 1) % NGM == 0;
        if (more) {
            const char* gb = group_base<G>(Wu, (g + 1) * G);
#pragma unroll
            for (int i = 0; i < G; ++i) nxt[i] = load_quad<G>(gb, lane_off, i);
        }
        if (bias_too) bt = bias_tile(bias, (g + 1) / NGM, h);
        __builtin_amdgcn_sched_barrier(0);   // the prefetch stays AHEAD of this group's MFMAs
        // one wait per group (loads return in order: all but the ones just issued have landed), not one per quad
        if (!more)
            __builtin_amdgcn_s_waitcnt(vmcnt_only(0));
        else if (bias_too)
            __builtin_amdgcn_s_waitcnt(vmcnt_only(G + 4));
        else
            __builtin_amdgcn_s_waitcnt(vmcnt_only(G));
#pragma unroll
        for (int i = 0; i < G; ++i) {
            const int quad = g * G + i, mt = quad / QPM, kq = quad % QPM, kt = kq / 4, q = kq % 4;
            if (kq == 0) {
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = bt;
            }
#pragma unroll
            for (int t = 0; t < NT; ++t) acc[t] = mfma4(cur[i], X[t][kt], 4 * q, acc[t]);
            if (kq == QPM - 1) epi(mt, acc);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int i = 0; i < G; ++i) cur[i] = nxt[i];
    }
}

// ---- a module's LAST layer, operands swapped ---------------------------------------------------------------
// D = A.B is symmetric in how lanes index the two non-k dimensions, so feeding the activation register as the A
// operand and the packed weight as the B operand yields the TRANSPOSED tile: rows (registers) = the 32 samples,
// columns (lane&31) = 32 output channels -- from the same packed weights and with the same per-element fmaf chain
// (fma(a,b,c) == fma(b,a,c)), hence bit-identical values. In this orientation the max-pool over samples is an
// in-register max over the 16 accumulator registers plus ONE exchange between the two lane halves, and each lane
// ends up owning one channel: a coalesced 128-byte store instead of a 16-shuffle butterfly per 32 channels.
__device__ __forceinline__ v16f mfma4_swapped(const v16f& x, int q4, float4 w, v16f acc) {
    acc = mfma(x[q4 + 0], w.x, acc);
    acc = mfma(x[q4 + 1], w.y, acc);
    acc = mfma(x[q4 + 2], w.z, acc);
    acc = mfma(x[q4 + 3], w.w, acc);
    return acc;
}

__device__ __forceinline__ v16f splat16(float v) {
    v16f a;
#pragma unroll
    for (int i = 0; i < 16; ++i) a[i] = v;
    return a;
}

// The pool of a swapped tile is max(0, max_j acc_j): the max over the samples with the ReLU folded in (it commutes with
// max). It runs on the values' BIT PATTERNS as signed integers: non-negative floats order like their patterns, and every
// negative float, -0.0 included, is a negative integer and loses to the 0 the chain starts from -- so the integer maximum
// is the largest positive value, or +0.0, which is what a float max followed by the ReLU returns (SPEC 4: activations are
// not NaN). A three-input integer max is one plain instruction (v_max3_i32) and needs no canonicalisation: 16 values and
// the running maximum cost 8 instructions instead of 16.
// pool_acc folds a tile's 16 registers into a running maximum m >= 0 (0, or what earlier tiles of the centre left);
// pool_halves merges the two lane halves of TWO m-tiles' running maxima at once: lanes 0-31 return the pooled value of
// channel lane&31 of tile a, lanes 32-63 that of tile b -- the form a full-wave store of two m-tiles wants.
__device__ __forceinline__ int pool_acc(const v16f& a, int m) {
#pragma unroll
    for (int i = 0; i < 16; i += 2) m = max(max(m, __float_as_int(a[i])), __float_as_int(a[i + 1]));
    return m;
}
__device__ __forceinline__ float pool_halves(int a, int b) {
    // v_permlane32_swap (gfx950) exchanges the upper 32 lanes of its first operand with the lower 32 of its second: r[0] is
    // (a's lower half, b's lower half), r[1] is (a's upper half, b's upper half). It is a plain VALU op; __shfl_xor(m, 32)
    // goes through the LDS crossbar (ds_bpermute: address VGPR, lgkmcnt wait) in the middle of an MFMA stream
    const auto r = __builtin_amdgcn_permlane32_swap((unsigned)a, (unsigned)b, false, false);
    return __int_as_float(max((int)r[0], (int)r[1]));
}
// sa3_kernel's pool: one tile per m-tile, as a float max tree. (The integer form saves 8 of its ~180 non-MFMA instructions
// per m-tile there and measured nothing, profiles/r11_sa1_p2_pool_after.txt, so sa3 keeps the form it was measured with.)
__device__ __forceinline__ float pool_swapped(const v16f& a) {
    float m0 = max1(max1(a[0], a[1]), max1(a[2], a[3]));
    float m1 = max1(max1(a[4], a[5]), max1(a[6], a[7]));
    float m2 = max1(max1(a[8], a[9]), max1(a[10], a[11]));
    float m3 = max1(max1(a[12], a[13]), max1(a[14], a[15]));
    float m = max1(max1(m0, m1), max1(m2, m3));
    const auto r = __builtin_amdgcn_permlane32_swap(__float_as_uint(m), __float_as_uint(m), false, false);
    m = max1(__uint_as_float(r[0]), __uint_as_float(r[1]));
    return max1(m, 0.0f);
}

template <int KT, int NT, int G, class Epi>
__device__ __forceinline__ void stream_last_layer(const float* __restrict__ Wu, unsigned lane_off,
                                                  const float* __restrict__ bias, const v16f (&X)[NT][KT], int c, int MT,
                                                  Epi&& epi) {
    constexpr int QPM = KT * 4, NG = QPM / G;
    static_assert(QPM % G == 0, "group size must divide the quads per m-tile");
    float4 cur[G], nxt[G];
    {
        const char* gb = group_base<G>(Wu, 0);
#pragma unroll
        for (int i = 0; i < G; ++i) cur[i] = load_quad<G>(gb, lane_off, i);
    }
    const float* wm = Wu;                  // this m-tile's quads: uniform, advanced once per m-tile
    float bvn = bias[c];                   // the lane's bias, fetched an m-tile ahead
#pragma unroll 1
    for (int mt = 0; mt < MT; ++mt) {
        v16f acc[NT];
        const float bv = bvn;
#pragma unroll
        for (int t = 0; t < NT; ++t) acc[t] = splat16(bv);
        // the group after this m-tile's last is the next m-tile's first; after the last m-tile the prefetch wraps to quad 0
        // (loaded for nothing, in bounds) instead of clamping every address
        const float* wn = mt + 1 < MT ? wm + QPM * 256 : Wu;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            const char* gb = g + 1 < NG ? group_base<G>(wm, (g + 1) * G) : group_base<G>(wn, 0);
#pragma unroll
            for (int i = 0; i < G; ++i) nxt[i] = load_quad<G>(gb, lane_off, i);
            if (g == 0) bvn = bias[(mt + 1 < MT ? mt + 1 : mt) * 32 + c];
            __builtin_amdgcn_sched_barrier(0);
            if (g == 0)                      // one wait per group, as in stream_layer
                __builtin_amdgcn_s_waitcnt(vmcnt_only(G + 1));
            else
                __builtin_amdgcn_s_waitcnt(vmcnt_only(G));
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int kq = g * G + i, kt = kq / 4, q = kq % 4;
#pragma unroll
                for (int t = 0; t < NT; ++t) acc[t] = mfma4_swapped(X[t][kt], 4 * q, cur[i], acc[t]);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < G; ++i) cur[i] = nxt[i];
        }
        epi(mt, acc);
        wm = wn;
    }
}

// ---- furthest point sampling: one workgroup per point set -----------------------------------------
// LDS: pts[n] = (x,y,z,|p|^2), tmp[n] running min distance. One barrier per pick: the four waves'
// (best, index) pairs go through a double-buffered 4-entry LDS slot. (The slot is carved from the dynamic LDS too: the
// launcher raises the kernel's dynamic limit to the whole 160 KiB, which a kernel with static LDS beside it is refused.)
constexpr int FPS_LDS_SLOT_BYTES = 2 * 4 * 8;
__global__ __launch_bounds__(256) void fps_kernel(const float* __restrict__ xyz, int stride, int n, int npoint,
                                                  int* __restrict__ idx_out, float* __restrict__ new_xyz) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* pts = (float4*)smem;
    float* tmp = (float*)(pts + n);
    float (*rbest)[4] = (float (*)[4])(tmp + n);
    int (*rbesti)[4] = (int (*)[4])(tmp + n + 8);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* base = xyz + (size_t)blockIdx.x * n * stride;
    for (int k = tid; k < n; k += 256) {
        float x = base[(size_t)k * stride], y = base[(size_t)k * stride + 1], z = base[(size_t)k * stride + 2];
        pts[k] = make_float4(x, y, z, (x * x + y * y) + z * z);
        tmp[k] = 1e10f;
    }
    __syncthreads();
    int old = 0;
    int* io = idx_out + (size_t)blockIdx.x * npoint;
    float* xo = new_xyz + (size_t)blockIdx.x * npoint * 3;
    if (tid == 0) {
        io[0] = 0;
        xo[0] = pts[0].x;
        xo[1] = pts[0].y;
        xo[2] = pts[0].z;
    }
    for (int j = 1; j < npoint; ++j) {
        const float4 po = pts[old];
        float best = -1.0f;
        int besti = 0;
        for (int k = tid; k < n; k += 256) {
            float4 p = pts[k];
            if (p.w <= 1e-3f) continue;
            float dx = p.x - po.x, dy = p.y - po.y, dz = p.z - po.z;
            float d = (dx * dx + dy * dy) + dz * dz;
            float d2 = fminf(d, tmp[k]);
            tmp[k] = d2;
            if (d2 > best) {
                best = d2;
                besti = k;
            }
        }
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            float ob = __shfl_xor(best, m);
            int oi = __shfl_xor(besti, m);
            if (ob > best || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        const int buf = j & 1;
        if (lane == 0) {
            rbest[buf][wave] = best;
            rbesti[buf][wave] = besti;
        }
        __syncthreads();
        best = rbest[buf][0];
        besti = rbesti[buf][0];
#pragma unroll
        for (int w = 1; w < 4; ++w) {
            float ob = rbest[buf][w];
            int oi = rbesti[buf][w];
            if (ob > best || (ob == best && oi < besti)) {
                best = ob;
                besti = oi;
            }
        }
        old = besti;
        if (tid == 0) {
            io[j] = old;
            float4 p = pts[old];
            xo[3 * j] = p.x;
            xo[3 * j + 1] = p.y;
            xo[3 * j + 2] = p.z;
        }
    }
}

// ---- furthest point sampling, register-resident form -------------------------------------------------
// Thread t owns the CONTIGUOUS indices [t*P, t*P+P): coordinates and running distances live in registers, so a
// pick costs P distance updates per lane (VALU), one DPP max-scan across the wave, one ballot and one LDS hand-off
// between the four waves. Because lower lanes (and lower waves) own lower indices, "first maximum in index order"
// -- pointnet2's tie rule -- is simply the lowest lane holding the maximum: no (value, index) pair reduction.
//
// What a pick costs is what this kernel costs: 1000 workgroups x 4 waves x 511 picks issue every instruction of the pick
// loop, at four waves per SIMD, and the vector pipe is the limit (profiles/r10_sampling_before.txt). So the loop is
// written for instruction COUNT:
//   distances     x and y of the points (2i, 2i+1) sit in adjacent registers and go through the packed f32 instructions
//                 as a PAIR: dx, dy, dx*dx, dy*dy, + = 5 v_pk for two points. (Packing dx with dy of ONE point, as the
//                 compiler does by itself, makes every packed instruction wait for the one before it.) The operation
//                 order is SPEC 4.1's, (dx*dx + dy*dy) + dz*dz, each operation rounded on its own.
//   running min   one v_min_f32 per point (min1: fminf() puts a canonicalising v_max x, x in front of it, since the
//                 compiler cannot see that a value carried round the loop is no signalling NaN; a distance never is).
//   arg-max       running distances are >= +0 or the sentinel -1, never NaN and never -0, so as SIGNED INTEGERS they order
//                 exactly as floats. The lane maximum is v_max3_i32 (P/2 instructions), the wave scan is v_max_i32 in
//                 its DPP form (one instruction per step), and no index travels with the value: the winner's index is
//                 recovered afterwards from P ballots "tmp[j] == wave maximum" -- the lowest lane of mask j is the first
//                 lane whose j-th point holds the maximum, lane * P + j is its index, and the smallest of those is the
//                 first maximum in index order. The rest of that is scalar. The sentinel needs no case of its own: with
//                 nothing selectable every value is -1, the first maximum is lane 0 / j 0 of wave 0 = index 0, which
//                 is what pointnet2 keeps.
//   hand-off      lane 0 of each wave writes (maximum, index) as one 8-byte LDS word, double-buffered; after the pick's
//                 one barrier every lane reads the four pairs with two ds_read_b128, takes the first wave holding the
//                 largest maximum and reads that point's coordinates for the next pick.
//   output        the picked indices collect in LDS (one ds_write per pick, no global store and so no vmcnt wait in
//                 front of the barrier) and leave, with their coordinates, in one coalesced pass after the last pick.
typedef float v2f __attribute__((ext_vector_type(2)));

// min of two floats as ONE instruction (see max1; here the second operand is carried round a loop)
__device__ __forceinline__ float min1(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// one step of the wave's max-scan: lanes with no source lane (and rows outside ROW_MASK) keep their own value. `old` is
// the identity of the signed max, which lets the compiler fold the move into v_max_i32's own DPP form.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ int dpp_imax(int v) {
    const int moved = __builtin_amdgcn_update_dpp((int)0x80000000, v, CTRL, ROW_MASK, 0xf, false);
    return max(v, moved);
}

// maximum of a wave64 (gfx9 DPP: row_shr 1,2,4,8 then row_bcast 15 / 31 leave it in lane 63), as a wave-uniform value
__device__ __forceinline__ int wave_imax_dpp(int v) {
    v = dpp_imax<0x111, 0xf>(v);   // row_shr:1
    v = dpp_imax<0x112, 0xf>(v);   // row_shr:2
    v = dpp_imax<0x114, 0xf>(v);   // row_shr:4
    v = dpp_imax<0x118, 0xf>(v);   // row_shr:8
    v = dpp_imax<0x142, 0xa>(v);   // row_bcast:15 into rows 1 and 3
    v = dpp_imax<0x143, 0xc>(v);   // row_bcast:31 into rows 2 and 3
    return __builtin_amdgcn_readlane(v, 63);
}

constexpr int FPS_REG_MAX_N = 256 * 12;   // the register form's limits: 12 points per lane,
constexpr int FPS_REG_MAX_NPOINT = 3072;  // and the picked-index list beside the points in 64 KiB of LDS

// the pick loop. A pick travels as the LDS ADDRESS of its point (pts + 16 * index, made in scalar registers by the wave
// that found it), so the next pick's coordinates are read with no address arithmetic; picked[jj] receives pick jj in that
// form, one pick late (by the lanes that are writing anyway). Returns the last pick.
typedef float v4f __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) const v2f lds_v2f;
typedef __attribute__((address_space(3))) const v4f lds_v4f;

template <int P, bool PLANAR>
__device__ __forceinline__ unsigned fps_pick_loop(const v2f (&X)[P / 2], const v2f (&Y)[P / 2], const v2f (&Z)[P / 2],
                                                  float (&tmp)[P], unsigned pts_addr, unsigned* picked, int2 (*slot)[4],
                                                  int npoint, int lane, int wave) {
    unsigned old = pts_addr;   // index 0
    for (int jj = 1; jj < npoint; ++jj) {
        float pox, poy, poz = 0.0f;
        if (PLANAR) {
            const v2f po = *(lds_v2f*)(size_t)old;
            pox = po.x, poy = po.y;
        } else {
            const v4f po = *(lds_v4f*)(size_t)old;
            pox = po.x, poy = po.y, poz = po.z;
        }
#pragma unroll
        for (int i = 0; i < P / 2; ++i) {
            const v2f dx = X[i] - pox, dy = Y[i] - poy;
            v2f d = dx * dx + dy * dy;
            if (!PLANAR) {
                const v2f dz = Z[i] - poz;
                d = d + dz * dz;
            }
            tmp[2 * i] = min1(d.x, tmp[2 * i]);
            tmp[2 * i + 1] = min1(d.y, tmp[2 * i + 1]);
        }
        int m = __float_as_int(tmp[0]);
#pragma unroll
        for (int j = 1; j < P; ++j) m = max(m, __float_as_int(tmp[j]));
        const int wmax = wave_imax_dpp(m);
        // the wave's first maximum: the lowest lane that holds one, and in it the lowest j (scalar from here on)
        unsigned long long mk[P], any = 0;
#pragma unroll
        for (int j = 0; j < P; ++j) {
            mk[j] = __ballot(__float_as_int(tmp[j]) == wmax);
            any |= mk[j];
        }
        const int src = __builtin_ctzll(any);   // (some lane holds the maximum: `any` is never 0)
        int jsel = P - 1;
#pragma unroll
        for (int j = P - 2; j >= 0; --j) jsel = ((mk[j] >> src) & 1) ? j : jsel;
        const unsigned wpick = pts_addr + 16u * (unsigned)(wave * (64 * P) + src * P + jsel);
        const int buf = jj & 1;
        if (lane == 0) {
            slot[buf][wave] = make_int2(wmax, (int)wpick);
            picked[jj - 1] = old;
        }
        __syncthreads();
        const int4 a = *(const int4*)&slot[buf][0], b = *(const int4*)&slot[buf][2];
        const int M = max(max(a.x, a.z), max(b.x, b.z));
        // the FIRST wave with the largest maximum: an equal maximum in a later wave has a higher index
        old = (unsigned)(a.x == M ? a.y : a.z == M ? a.w : b.x == M ? b.y : b.w);
    }
    return old;
}

template <int P>
__global__ __launch_bounds__(256) void fps_reg_kernel(const float* __restrict__ xyz, int stride, int n, int npoint,
                                                      int* __restrict__ idx_out, float* __restrict__ new_xyz) {
    static_assert(P % 2 == 0, "points go through the packed instructions in pairs");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* pts = (float4*)smem;        // read-only copy for the "current point" broadcast
    unsigned* picked = (unsigned*)(pts + n);   // the picks, in order, as LDS addresses of their points
    const unsigned pts_addr = (unsigned)(size_t)(__attribute__((address_space(3))) char*)smem;
    __shared__ __attribute__((aligned(16))) int2 slot[2][4];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const float* base = xyz + (size_t)blockIdx.x * n * stride;
    v2f X[P / 2], Y[P / 2], Z[P / 2];
    float tmp[P];
    int anyz = 0;
#pragma unroll
    for (int j = 0; j < P; ++j) {
        const int k = tid * P + j;
        float x = 0.f, y = 0.f, z = 0.f;
        if (k < n) {
            x = base[(size_t)k * stride];
            y = base[(size_t)k * stride + 1];
            z = base[(size_t)k * stride + 2];
            pts[k] = make_float4(x, y, z, 0.f);
        }
        X[j / 2][j % 2] = x, Y[j / 2][j % 2] = y, Z[j / 2][j % 2] = z;
        anyz |= (z != 0.0f);
        // a point that may never be picked (|p|^2 <= 1e-3, or padding) gets running distance -1: min(d, -1) stays -1
        // and -1 never beats a live point's distance (>= 0), which is exactly pointnet2's `continue`
        tmp[j] = ((k < n) && (((x * x + y * y) + z * z) > 1e-3f)) ? 1e10f : -1.0f;
    }
    // the scorer's point sets are planar (SPEC 3.4: channel 2 is 0): with every z == 0 the dz terms are exact zeros and
    // can be skipped without changing a single bit; any non-zero z in the set selects the general loop
    const bool planar = !__syncthreads_or(anyz);
    const unsigned last = planar ? fps_pick_loop<P, true>(X, Y, Z, tmp, pts_addr, picked, slot, npoint, lane, wave)
                                 : fps_pick_loop<P, false>(X, Y, Z, tmp, pts_addr, picked, slot, npoint, lane, wave);
    if (tid == 0) picked[npoint - 1] = last;
    __syncthreads();
    int* io = idx_out + (size_t)blockIdx.x * npoint;
    float* xo = new_xyz + (size_t)blockIdx.x * npoint * 3;
    for (int j = tid; j < npoint; j += 256) {
        const int k = (int)((picked[j] - pts_addr) >> 4);
        const float4 p = pts[k];
        io[j] = k;
        xo[3 * j] = p.x;
        xo[3 * j + 1] = p.y;
        xo[3 * j + 2] = p.z;
    }
}

// ---- ball query, register-resident form: the whole point set in every wave's registers ------------------
// A workgroup of BQR_WAVES waves stages the point set once in LDS (coordinate planes, padded to NCH chunks of 64 with NaN,
// which is inside no ball: the tail of the last chunk needs no bound check and no mask), every wave copies ALL of it into
// registers -- lane l holds point 64 c + l of every chunk c, x (y, z) of chunks 2i and 2i+1 in adjacent registers -- and
// then walks the centres wave, wave + W, ... of its hypothesis. Per centre nothing is read but the centre itself (a
// wave-uniform scalar load, issued a centre ahead), and a chunk costs, with its hits:
//   2.5 (4 with z)  distances of two chunks at a time in the packed f32 instructions, `cx - p.x` and the operation
//                   order of the oracle, each operation rounded on its own
//   1               the compare, whose result IS the chunk's ballot over 64 consecutive indices, in scalar registers
//   2               v_mbcnt_lo / v_mbcnt_hi: the lane's rank among the chunk's hits
//   2               address (rank * 4 + the scalar base that carries the running count) and ds_write_b32 of 64 c + lane
//                   (which the compiler keeps as a register per chunk, made once per wave)
// and everything else -- count (s_bcnt1), early exit -- is scalar. Hits go to a row of the wave in LDS; the row has room
// for a whole group of BQR_GROUP chunks past the 64th hit, so the body of a group has no bound check, and
// "64 found" is tested once per group. The centre's 64 indices, padded with the first hit (= row[0]), then leave as one
// coalesced 256-byte store. There is no wait inside the chunk loop: the only LDS traffic are the writes.
//
// The planar fast path skips the dz term where it is an exact +0 for every pair the workgroup looks at, which changes no
// bit: it is taken when every point AND every centre of the workgroup has z == 0 (a workgroup-wide OR while staging, as in
// fps_reg_kernel; the scorer's sets are planar and their centres are members). A centre off the plane selects the general path.
//
// 8 waves per workgroup: NCH = 48 with z needs 144 registers for the points alone, over the 128 a 16-wave workgroup
// can have; at 8 waves the 8/16/32-chunk forms stay within 128 registers, so two workgroups share a CU (4 waves per SIMD),
// and the LDS for two (2 x (12 B x 2048 + 10 KiB)) is there. A workgroup covers up to BQR_CPB = 256 centres of one hypothesis
// (SA1: two workgroups per hypothesis, 2000 over the chip's 512 places). Measured at 1000 x 2048 points, 512 centres each
// (profiles/r10_sampling_after.txt): 256 centres per workgroup 0.247 ms, 512 centres 0.254 ms (staging twice costs less than
// the coarser tail), BQR_GROUP = 2 instead of 4 0.259 ms.
constexpr int BQ_CPB = 512;       // centres per workgroup, LDS form
constexpr int BQR_CPB = 256;      // centres per workgroup, register form
constexpr int BQR_WAVES = 8, BQR_THREADS = 64 * BQR_WAVES;
constexpr int BQR_GROUP = 4;                          // chunks between two tests of the count
constexpr int BQR_ROW = 64 * (BQR_GROUP + 1);         // ints per wave: slots < 64 + 64 * BQR_GROUP inside a group
constexpr int BQR_MAX_N = 64 * 48;
// centres per ball-query workgroup for a set of n points (either form), and workgroups per hypothesis
inline int ball_cpb(int n) { return n <= BQR_MAX_N ? BQR_CPB : BQ_CPB; }
inline int ball_parts(int n, int npoint) { return (npoint + ball_cpb(n) - 1) / ball_cpb(n); }

typedef __attribute__((address_space(3))) int lds_int;

// Besides the rows, the ball query can say what the SA kernel that reads them will spend (SPEC 4.5, slice_balance.h):
// each centre's hit count, capped at 64, as a byte, and the cost of each workgroup's centres as one total. The count is
// wave-uniform where it is made; the function returns the cost of the centres this wave answered for.
template <int NCH, bool PLANAR>
__device__ __forceinline__ int ball_reg_centres(const float* xs, const float* ys, const float* zs, int* row,
                                                const float* __restrict__ cen, int* __restrict__ out,
                                                unsigned char* __restrict__ hits, int sa2, int jbeg, int jend,
                                                float r2, int lane) {
    v2f X[NCH / 2], Y[NCH / 2], Z[PLANAR ? 1 : NCH / 2];
#pragma unroll
    for (int i = 0; i < NCH / 2; ++i) {
        X[i] = v2f{xs[128 * i + lane], xs[128 * i + 64 + lane]};
        Y[i] = v2f{ys[128 * i + lane], ys[128 * i + 64 + lane]};
        if (!PLANAR) Z[i] = v2f{zs[128 * i + lane], zs[128 * i + 64 + lane]};
    }
    const unsigned row_addr = (unsigned)(size_t)(lds_int*)row;   // (LDS addresses are 32 bits)
    float cx = 0.f, cy = 0.f, cz = 0.f;
    int cost = 0;
    if (jbeg < jend) cx = cen[3 * (size_t)jbeg], cy = cen[3 * (size_t)jbeg + 1], cz = cen[3 * (size_t)jbeg + 2];
    for (int j = jbeg; j < jend; j += BQR_WAVES) {
        const float ccx = cx, ccy = cy, ccz = cz;
        const int jn = min(j + BQR_WAVES, jend - 1);   // the next centre, a centre ahead (the last one reads itself again)
        cx = cen[3 * (size_t)jn], cy = cen[3 * (size_t)jn + 1], cz = cen[3 * (size_t)jn + 2];
        int cnt = 0;
#pragma unroll
        for (int g = 0; g < NCH / BQR_GROUP; ++g) {
#pragma unroll
            for (int i = g * (BQR_GROUP / 2); i < (g + 1) * (BQR_GROUP / 2); ++i) {
                const v2f dx = ccx - X[i], dy = ccy - Y[i];
                v2f d = dx * dx + dy * dy;
                if (!PLANAR) {
                    const v2f dz = ccz - Z[i];
                    d = d + dz * dz;
                }
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const bool hit = d[h] < r2;
                    const unsigned long long mk = __ballot(hit);
                    const int rank = __builtin_amdgcn_mbcnt_hi((unsigned)(mk >> 32),
                                                               __builtin_amdgcn_mbcnt_lo((unsigned)mk, 0));
                    // the slot's address is rank * 4 + a SCALAR base; seen through, the compiler adds count and rank in the
                    // vector pipe first
                    unsigned base = row_addr + 4 * cnt;
                    asm("" : "+s"(base));
                    if (hit) *(lds_int*)(size_t)(base + 4 * rank) = (2 * i + h) * 64 + lane;
                    cnt += __popcll(mk);
                }
            }
            if (cnt >= 64) break;
        }
        // row[0] is the first hit; with no hit at all the row is stale and the answer is 0 everywhere
        const int mine = row[lane];
        int first = __builtin_amdgcn_readfirstlane(mine);
        first = cnt > 0 ? first : 0;
        out[(size_t)j * 64 + lane] = lane < cnt ? mine : first;
        if (hits) {
            const int capped = min(cnt, 64);
            if (lane == 0) hits[j] = (unsigned char)capped;
            cost += centre_cost(capped, sa2);
        }
    }
    return cost;
}

// the waves' costs, summed through LDS and written with one plain store (every thread of the workgroup calls this)
template <int NW>
__device__ __forceinline__ void store_cost_total(int* lds, int wave, int cost, int* __restrict__ dst) {
    if ((threadIdx.x & 63) == 0) lds[wave] = cost;
    __syncthreads();
    if (threadIdx.x == 0) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < NW; ++w) sum += lds[w];
        *dst = sum;
    }
}

template <int NCH>
__global__ __launch_bounds__(BQR_THREADS, NCH <= 32 ? 4 : 2) void ball_query_reg_kernel(const float* __restrict__ xyz, int stride, int n,
                                                                     const float* __restrict__ new_xyz, int npoint,
                                                                     float r2, int* __restrict__ idx,
                                                                     unsigned char* __restrict__ hits,
                                                                     int* __restrict__ cost_part, int sa2) {
    static_assert(NCH % BQR_GROUP == 0 && BQR_GROUP % 2 == 0, "whole groups of chunk pairs");
    constexpr int N = 64 * NCH;
    __shared__ float xs[N], ys[N], zs[N];
    __shared__ int rows[BQR_WAVES][BQR_ROW];
    __shared__ int wave_cost[BQR_WAVES];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int b = blockIdx.x;
    const float* base = xyz + (size_t)b * n * stride;
    const float nan = __builtin_nanf("");
    int offplane = 0;
    for (int k = tid; k < N; k += BQR_THREADS) {
        float x = nan, y = nan, z = 0.0f;
        if (k < n) x = base[(size_t)k * stride], y = base[(size_t)k * stride + 1], z = base[(size_t)k * stride + 2];
        xs[k] = x, ys[k] = y, zs[k] = z;
        offplane |= (z != 0.0f);
    }
    const int jbeg = blockIdx.y * BQR_CPB, jend = min(jbeg + BQR_CPB, npoint);
    const float* cen = new_xyz + (size_t)b * npoint * 3;
    for (int j = jbeg + tid; j < jend; j += BQR_THREADS) offplane |= (cen[3 * (size_t)j + 2] != 0.0f);
    const bool planar = !__syncthreads_or(offplane);
    int* out = idx + (size_t)b * npoint * 64;
    unsigned char* hb = hits ? hits + (size_t)b * npoint : nullptr;
    int cost;
    if (planar)
        cost = ball_reg_centres<NCH, true>(xs, ys, zs, rows[wave], cen, out, hb, sa2, jbeg + wave, jend, r2, lane);
    else
        cost = ball_reg_centres<NCH, false>(xs, ys, zs, rows[wave], cen, out, hb, sa2, jbeg + wave, jend, r2, lane);
    if (cost_part) store_cost_total<BQR_WAVES>(wave_cost, wave, cost, cost_part + (size_t)b * gridDim.y + blockIdx.y);
}

// ---- ball query, LDS form: the fallback for point sets over BQR_MAX_N points ----------------------------
// One wave per centre, 64 candidate points per ballot, the points read from LDS chunk by chunk.
// A workgroup of 16 waves stages the point set ONCE in LDS and covers up to 512 centres (all of SA1's): with 64 centres
// per 4-wave workgroup the same 2048 points were staged eight times per hypothesis (and the strided 12-of-32-byte row
// reads cost twice their bytes), which was most of the kernel.
constexpr int BQ_THREADS = 1024;
__global__ __launch_bounds__(BQ_THREADS) void ball_query_kernel(const float* __restrict__ xyz, int stride, int n,
                                                                const float* __restrict__ new_xyz, int npoint, float r2,
                                                                int* __restrict__ idx, unsigned char* __restrict__ hits,
                                                                int* __restrict__ cost_part, int sa2) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float4* pts = (float4*)smem;
    int* wave_cost = (int*)(pts + n);  // one int per wave behind the points (dynamic too: the kernel may be given all the LDS)
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.x;
    const float* base = xyz + (size_t)b * n * stride;
    for (int k = tid; k < n; k += BQ_THREADS)
        pts[k] = make_float4(base[(size_t)k * stride], base[(size_t)k * stride + 1], base[(size_t)k * stride + 2], 0.f);
    __syncthreads();
    const int jend = min((int)(blockIdx.y + 1) * BQ_CPB, npoint);
    int cost = 0;
    for (int j = blockIdx.y * BQ_CPB + wave; j < jend; j += BQ_THREADS / 64) {
        const float* c = new_xyz + ((size_t)b * npoint + j) * 3;
        const float cx = c[0], cy = c[1], cz = c[2];
        int* o = idx + ((size_t)b * npoint + j) * 64;
        int cnt = 0, first = -1;
        // four 64-point chunks per trip (most centres need ~25 chunks to collect 64 neighbours: the trip's latency
        // chain -- LDS read, compare, ballot, scalar bookkeeping -- is what bounds the kernel, so give it 4x the work);
        // slots are still handed out in index order, hits past the 64th are simply not stored
        for (int k0 = 0; k0 < n && cnt < 64; k0 += 256) {
            bool hit[4];
            unsigned long long bal[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int k = k0 + 64 * u + lane;
                hit[u] = false;
                if (k < n) {
                    float4 p = pts[k];
                    float dx = cx - p.x, dy = cy - p.y, dz = cz - p.z;
                    float d2 = (dx * dx + dy * dy) + dz * dz;
                    hit[u] = d2 < r2;
                }
                bal[u] = __ballot(hit[u]);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (bal[u]) {
                    if (first < 0) first = k0 + 64 * u + __ffsll((long long)bal[u]) - 1;
                    int slot = cnt + __popcll(bal[u] & ((1ull << lane) - 1ull));
                    if (hit[u] && slot < 64) o[slot] = k0 + 64 * u + lane;
                    cnt += __popcll(bal[u]);
                }
            }
        }
        if (first < 0) first = 0;
        if (cnt > 64) cnt = 64;
        if (lane >= cnt) o[lane] = first;
        if (hits) {
            if (lane == 0) hits[(size_t)b * npoint + j] = (unsigned char)cnt;
            cost += centre_cost(cnt, sa2);
        }
    }
    if (cost_part) store_cost_total<BQ_THREADS / 64>(wave_cost, wave, cost, cost_part + (size_t)b * gridDim.y + blockIdx.y);
}

// ---- SA1: gather (K=8) -> 64 -> 64 -> 128 -> max over the group's 64 samples -------------------------
// One wave per BODY of two 32-column tiles, which carry the distinct samples of one or more centres in granules of 8 columns
// (the granule stream, below; "centre" in the figures that follow is such a body, and a centre whose 64 samples are all
// distinct fills one). The kernel is persistent and runs ONE wave per SIMD
// (512 registers per lane): each wave loads the three packed layers once, straight from the blob, into 50 float4 = 200
// registers (the packed image is lane-linear: quad q of a layer is the float4 at W4[q * 64 + lane]) and the folded biases of
// layers 1-2 as four ready-made accumulator tiles (64 registers, the C operand of each chain's first MFMA), then walks a
// contiguous slice of the centres. All three layers are fully unrolled over their quads (16 + 128 + 256 = 400 MFMAs per
// body) and read no operand between MFMAs. A centre's 128 pooled values gather in a row of the wave's own staging tile in LDS
// (16 ds_max_i32 per body), and once per 32 centres the wave applies the per-point part of SA2's first layer to
// that tile (sa1_p2_tile: 256 MFMAs, operands and weights read from LDS) and stores P. The layer's weights are staged in LDS
// once per workgroup behind the kernel's only barrier, in the prologue; after it the four waves run free of each other.
//
// What sets this kernel's rate (profiles/r08_sa1_before.txt, r08_sa1_after.txt): it runs at the clock of a bare
// register-fed MFMA stream, and the time it loses is proportional to the number of vector / LDS instructions per centre --
// about four to five cycles of matrix time each, wherever they sit in the stream (re-ordering them between the MFMAs of an
// independent accumulator measured nothing). So the design is about instruction COUNT: no ds_read per weight quad, no bias
// read, one instruction per ReLU (max1), one per TWO pooled values (pool_acc), accumulators in vector registers so that ReLU
// and pool read them in place.
//
// Register budget (per lane), centre loop: weights 200 + bias tiles 64 + last-layer bias 4 + x 8 + Y1 64 + Y2 64 + accumulators
// 32 + next body's gather (map entries 2, indices 2) = 440 at the widest point (layer 2); rows 8 and centre coordinates 6 arrive
// under the last layer. The per-tile phase runs when the layer temporaries
// (x, Y1, Y2, accumulators: 168) are dead and needs less: the staged tile as B operand 64 + weight quads of the group in use
// and of the next 32 + one m-tile's accumulator 16 + the next bias tile 16 = 128 beside the same 281 of weights, bias tiles
// and gather. The build stands at 256 VGPRs + 256 AGPRs (230 before the granule stream, 216 before the phase was added: the
// allocator parks some of its addressing in the AGPR half, 33 v_accvgpr_read per body). tests/test_pn2_resources.py holds the build to zero scratch and 512 registers.
//
// The weights are only ever MFMA operands, which may come from the accumulator (AGPR) half of the register file; ReLU and
// pool are vector instructions, which may not read it. The file is compiled with the VGPR form of the MFMA (_build.py:
// accumulators in vector registers), and the weights are pinned to the AGPR half as they arrive: without the pin the
// allocator keeps them on the vector side's books and copies each one back (v_accvgpr_read) before the MFMA that uses it.
__device__ __forceinline__ void pin_acc(float4& w) { asm volatile("" : "+a"(w.x), "+a"(w.y), "+a"(w.z), "+a"(w.w)); }

// An activation tile that only MFMAs will read from here on (sa3_kernel: 384 activation registers live beside the weight
// stream). Left to the allocator, the tiles that do not fit in the vector half are SPILLED to the accumulator half and
// copied back one register at a time in front of every MFMA that reads them (v_accvgpr_read + a hazard nop, per MFMA);
// pinned, they are written there once and the MFMAs take them as operands in place.
__device__ __forceinline__ void pin_acc16(v16f& a) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        float t = a[i];
        asm volatile("" : "+a"(t));
        a[i] = t;
    }
}

template <int N>
__device__ __forceinline__ void load_quads(float4 (&w)[N], const float* __restrict__ Wp, int lane) {
#pragma unroll
    for (int q = 0; q < N; ++q) w[q] = ((const float4*)Wp)[q * 64 + lane], pin_acc(w[q]);
}

__device__ __forceinline__ void stage_lds(float* dst, const float* __restrict__ src, int nfloats) {
    for (int i = threadIdx.x * 4; i < nfloats; i += blockDim.x * 4) *(float4*)(dst + i) = *(const float4*)(src + i);
}

// LDS of sa1_kernel (floats): the p2 layer's packed weights [4 m-tiles][16 quads][64 lanes] x 4 | its 128 biases | one
// staging tile of SA1_ROWS centres x 128 pooled channels per wave. The row pitch of 132 floats puts the 16 lanes of a
// ds_read_b128 lane group (same lane half, 16 different rows) on 16 different 16-byte slots of the 256-byte bank row.
constexpr int SA1_ROWS = 32, SA1_PITCH = 132;
constexpr int SA1_WP = 0, SA1_BP = 16384, SA1_STAGE = SA1_BP + 128;   // 64 KB | 0.5 KB | 4 x 16.5 KB (| the maps, below)

// The per-point part of SA2's first layer, p[pt][o] = chain(bias, W[:, :128] . feat1[pt]) (the grouped-xyz columns are
// applied per sample in sa2_kernel, continuing the same chain), for the SA1_ROWS centres of a wave's staging tile: the
// tile is the B operand (register 4q+e of lane half h = channel 32kt+8q+4h+e, column = row of the tile), an m-tile is
// the bias tile as the C operand and then the 16 weight quads in order. Rows >= nvalid are computed and not stored.
__device__ __forceinline__ void sa1_p2_tile(const float* w, const float* stage, float* __restrict__ P, int row0, int nvalid,
                                            int lane) {
    const int h = lane >> 5, c = lane & 31;
    v16f X[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 v = *(const float4*)(stage + c * SA1_PITCH + kt * 32 + 8 * q + 4 * h);
            X[kt][4 * q + 0] = v.x, X[kt][4 * q + 1] = v.y, X[kt][4 * q + 2] = v.z, X[kt][4 * q + 3] = v.w;
        }
    constexpr int G = 4, NG = 16 / G;    // weight quads per LDS read group, read a group ahead of the MFMAs that use them
    const float4* w4 = (const float4*)(w + SA1_WP) + lane;
    float4 cur[G], nxt[G];
#pragma unroll
    for (int i = 0; i < G; ++i) cur[i] = w4[i * 64];
    v16f bt = bias_tile(w + SA1_BP, 0, h);
    float* o = P + ((size_t)row0 + c) * 128 + 4 * h;
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) {
        v16f acc = bt;
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            // the group after the last wraps to quad 0 (read for nothing, in bounds)
#pragma unroll
            for (int i = 0; i < G; ++i) nxt[i] = w4[((mt * 16 + (g + 1) * G + i) & 63) * 64];
            if (g == NG - 1) bt = bias_tile(w + SA1_BP, (mt + 1) & 3, h);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < G; ++i) {
                const int kq = g * G + i;
                acc = mfma4(cur[i], X[kq / 4], 4 * (kq % 4), acc);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int i = 0; i < G; ++i) cur[i] = nxt[i];
        }
        if (c < nvalid) {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                *(float4*)(o + mt * 32 + 8 * q) = make_float4(acc[4 * q], acc[4 * q + 1], acc[4 * q + 2], acc[4 * q + 3]);
        }
    }
}

// ---- a persistent wave's slice of the centres (SPEC 4.5, slice_balance.h) --------------------------------------------
// The 64 lanes share the search: each sums its chunk of the ball query's cost totals into `scratch` (2 x 64 ints of LDS,
// the wave's own; LDS operations of one wave complete in order), and the walk over the sums is uniform.
__device__ __forceinline__ void wave_slice(const SliceCosts& sc, int gw, int nw, int* scratch, int lane, int& first, int& end) {
    scratch[lane] = lane_part_sum(sc, lane);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    auto lane_sums = [&](int k) { return __builtin_amdgcn_readfirstlane(scratch[k]); };
    auto fill = [&](int p) {
        scratch[64 + lane] = lane_centre_sum(sc, p, lane);
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        return [=](int k) { return __builtin_amdgcn_readfirstlane(scratch[64 + k]); };
    };
    slice_bounds(sc, gw, nw, lane_sums, fill, first, end);
    first = __builtin_amdgcn_readfirstlane(first), end = __builtin_amdgcn_readfirstlane(end);
}

// ---- sa1_kernel's granule stream (SPEC 4.5) ----------------------------------------------------------------------------
// The swapped last layer puts sample column s of a tile in lane half (s >> 2) & 1, register r with r >> 2 == s >> 3: the
// registers 0..7 and 8..15 of a lane half are two separate sets of 8 columns, and layers 1-2 treat every column on its own.
// A tile is therefore four GRANULES of 8 columns, keyed (lane half h', j = r >> 3): columns 16 j + 8 k + 4 h' + e, and each
// granule may carry 8 consecutive slots of a different centre. A centre with d distinct hits needs its first ceil(d / 8)
// granules (the slots behind repeat the first hit and the pool is a max), so the wave packs the granules its centres need
// into two-tile bodies, 8 granules each, instead of spending 8 on every centre:
//   per group of 32 consecutive centres of the slice (one staging tile; the slice's last group may be partial) lanes 0..31
//   take their centre's hit count, a wave scan places each centre's granules in the group's stream, and a per-wave MAP in
//   LDS says for every granule of the stream where its first slot is in the ball array (which gives centre, hence staging
//   row and hypothesis) and the LDS address of its owner's staging row. The stream is padded to whole bodies by repeating
//   its last granule: the max is idempotent. The next group's map is built when a group opens, into the other buffer;
//   granule 4 t + 2 j + h' of a body is tile t's (h', j); the gather's lane column c reads slot 4 k + e of it;
//   the pool is one chain per (tile, j) and lane half, ending in an LDS integer max (no return) into the owner's staging
//   row, which was zeroed when the group opened: the values are non-negative bit patterns (pool_acc), so the integer max is
//   the float max, whichever granule of whichever body feeds a row.
// Every column's fmaf chain and every centre's set of pooled values is what it was; sa1_p2_tile runs when the group's
// stream is done.
constexpr int SA1_MAP = 256;           // entries of a map: 32 centres x 8 granules at most, whole bodies
constexpr int SA1_MAPS = SA1_STAGE + 4 * SA1_ROWS * SA1_PITCH,
              SA1_LDS_FLOATS = SA1_MAPS + 4 * 2 * 2 * SA1_MAP;   // ... | per wave 2 buffers x (gather map, row map): 150 016 B

__global__ __launch_bounds__(256, 1) void sa1_kernel(const float* __restrict__ point_x, int M,
                                                     const int* __restrict__ ball, const float* __restrict__ cxyz,
                                                     int np, int total, const unsigned char* __restrict__ hits,
                                                     const int* __restrict__ part, int ppb, int cpb,
                                                     const float* __restrict__ W1p,
                                                     const float* __restrict__ b1, const float* __restrict__ W2p,
                                                     const float* __restrict__ b2, const float* __restrict__ W3p,
                                                     const float* __restrict__ b3, const float* __restrict__ Wpp,
                                                     const float* __restrict__ bp, float* __restrict__ feat,
                                                     float* __restrict__ P) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    stage_lds(wl + SA1_WP, Wpp, 16384);
    stage_lds(wl + SA1_BP, bp, 128);
    __syncthreads();                   // the only barrier: every wave passes it before any may leave
    // this wave's contiguous slice of the centres, cut by work (consecutive centres mostly share a hypothesis, i.e. a gather
    // base); the wave index is made visibly uniform so that the walk lives in scalar registers
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    int* maps = (int*)(wl + SA1_MAPS) + wave * (4 * SA1_MAP);
    int first, end;
    wave_slice(SliceCosts{part, hits, (total / np) * ppb, ppb, cpb, np, total, 0}, gw, nw, maps, lane, first, end);
    if (first >= end) return;          // nothing to do, no weights loaded
    float* stage = wl + SA1_STAGE + wave * (SA1_ROWS * SA1_PITCH);
    const unsigned stage_addr = (unsigned)(size_t)(lds_int*)stage, maps_addr = (unsigned)(size_t)(lds_int*)maps;
    float4 w1[2], w2[16], w3[32];
    load_quads(w1, W1p, lane);
    load_quads(w2, W2p, lane);
    load_quads(w3, W3p, lane);
    v16f B1[2], B2[2];
    float b3v[4];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) B1[mt] = bias_tile(b1, mt, h), B2[mt] = bias_tile(b2, mt, h);
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) b3v[mt] = b3[mt * 32 + c];

    // The map of the group of n centres from g0 (its hit counts in lanes 0..31 of cb), into buffer buf: returns its bodies.
    auto build_map = [&](int buf, int g0, int n, int cb) {
        const int gc = lane < n ? centre_cost(cb, 0) : 0;
        const int inc = wave_scan_up(gc, OpAdd(), lane), pos = inc - gc;
        const int G = __builtin_amdgcn_readlane(inc, 63), Gpad = (G + 7) & ~7;
        int* gm = maps + buf * (2 * SA1_MAP);
        int* rm = gm + SA1_MAP;
        const int e0 = (g0 + lane) * 64, ra = (int)stage_addr + lane * (SA1_PITCH * 4);
#pragma unroll
        for (int g = 0; g < 8; ++g)
            if (g < gc) gm[pos + g] = e0 + 8 * g, rm[pos + g] = ra;
        if (lane == n - 1) {           // the filler: the stream's last granule again
#pragma unroll
            for (int k = 0; k < 7; ++k)
                if (G + k < Gpad) gm[G + k] = e0 + 8 * (gc - 1), rm[G + k] = ra;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        return Gpad >> 3;
    };
    auto gather_map = [&](int buf, int body) { return maps_addr + (unsigned)(buf * (2 * SA1_MAP) + body * 8) * 4u; };

    // The gather of a body's 64 columns is an LDS read (the column's granule) and two dependent global loads (ball index
    // -> feature row): it is issued one body AHEAD -- the map entry at the top, the indices under the current body's second
    // layer, the rows and the owners' centre coordinates under its last layer -- so that a wave never sits on ~2 memory
    // latencies between bodies (there is no partner wave to cover them).
    const int lq = 2 * (c >> 4) + ((c >> 2) & 1), slot = 4 * ((c >> 3) & 1) + (c & 3);
    int e_n[2], i_n[2];
    float4 r_n[2];
    float cn[2][3];
    auto read_map = [&](unsigned gm_addr) {
        const lds_int* m = (const lds_int*)(size_t)(gm_addr + 4 * lq);
        e_n[0] = m[0], e_n[1] = m[4];
    };
    auto fetch_index = [&]() {
#pragma unroll
        for (int t = 0; t < 2; ++t) i_n[t] = ball[(size_t)(unsigned)(e_n[t] + slot)];
    };
    // a group of 32 straddles at most one hypothesis boundary: the granules from ball offset bound64 on gather from base_hi
    auto fetch_rows = [&](int base_lo, int base_hi, int bound64) {
#pragma unroll
        for (int t = 0; t < 2; ++t) {
            // the index is consumed HERE: left alone, the compiler widens it right behind its load in fetch_index and
            // waits for it there, a memory latency with nothing in flight
            int i0 = i_n[t];
            asm volatile("" : "+v"(i0));
            const int base = e_n[t] >= bound64 ? base_hi : base_lo;
            r_n[t] = *(const float4*)(point_x + ((size_t)base + i0) * 8 + 4 * h);
            const float* cc = cxyz + (size_t)(unsigned)(e_n[t] >> 6) * 3;
            cn[t][0] = cc[0], cn[t][1] = cc[1], cn[t][2] = cc[2];
        }
    };

    int g0 = first, buf = 0;
    int nb = build_map(0, first, min(32, end - first), hits[min(first + c, end - 1)]);
    int cbn = hits[min(first + 32 + c, end - 1)];          // the NEXT group's hit counts, a group ahead
    int base_lo = (first / np) * M, bound64 = (first / np + 1) * np * 64;
    read_map(gather_map(0, 0));
    fetch_index();
    fetch_rows(base_lo, base_lo + M, bound64);
#pragma unroll 1
    for (;;) {
        const int n = min(32, end - g0), g1 = g0 + 32;
        for (int i = lane; i < SA1_ROWS * SA1_PITCH / 4; i += 64) ((float4*)stage)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        int nb1 = 0, base_lo1 = base_lo, bound641 = bound64;
        if (g1 < end) {
            nb1 = build_map(buf ^ 1, g1, min(32, end - g1), cbn);
            cbn = hits[min(g1 + 32 + c, end - 1)];
            base_lo1 = (g1 / np) * M, bound641 = (g1 / np + 1) * np * 64;
        }
#pragma unroll 1
        for (int body = 0; body < nb; ++body) {
            float4 x[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                float4 r = r_n[t];
                if (h == 0) {
                    r.x = r.x - cn[t][0];
                    r.y = r.y - cn[t][1];
                    r.z = r.z - cn[t][2];
                }
                x[t] = r;
            }
            // the next body: of this group, the first of the next group, or (the slice's last) itself again: harmless
            const bool same = body + 1 < nb, cross = !same && nb1 > 0;
            const int nbase = cross ? base_lo1 : base_lo, nbound = cross ? bound641 : bound64;
            __builtin_amdgcn_sched_barrier(0);
            read_map(same ? gather_map(buf, body + 1) : cross ? gather_map(buf ^ 1, 0) : gather_map(buf, body));
            __builtin_amdgcn_sched_barrier(0);
            v16f Y1[2][2], Y2[2][2];
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    v16f acc = mfma(w1[mt].x, x[t].x, B1[mt]);
                    acc = mfma(w1[mt].y, x[t].y, acc);
                    acc = mfma(w1[mt].z, x[t].z, acc);
                    acc = mfma(w1[mt].w, x[t].w, acc);
                    Y1[t][mt] = relu16(acc);
                }
            }
            __builtin_amdgcn_sched_barrier(0);
            fetch_index();
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                v16f acc[2] = {B2[mt], B2[mt]};
#pragma unroll
                for (int kq = 0; kq < 8; ++kq) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[t] = mfma4(w2[mt * 8 + kq], Y1[t][kq / 4], 4 * (kq % 4), acc[t]);
                }
                Y2[0][mt] = relu16(acc[0]);
                Y2[1][mt] = relu16(acc[1]);
            }
            __builtin_amdgcn_sched_barrier(0);
            fetch_rows(nbase, nbase + M, nbound);
            // the owners' staging rows: entries 4 t + 2 j + h of this body's row map, at the lane's channel
            unsigned own[2][2];
            {
                const lds_int* m = (const lds_int*)(size_t)(gather_map(buf, body) + SA1_MAP * 4 + 4 * h);
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 2; ++j) own[t][j] = (unsigned)m[4 * t + 2 * j] + 4 * c;
            }
            __builtin_amdgcn_sched_barrier(0);
            // last layer, operands swapped (see mfma4_swapped): registers 0..7 and 8..15 of a tile are a granule each
#pragma unroll
            for (int mt = 0; mt < 4; ++mt) {
                v16f acc[2];
                acc[0] = acc[1] = splat16(b3v[mt]);
#pragma unroll
                for (int kq = 0; kq < 8; ++kq) {
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[t] = mfma4_swapped(Y2[t][kq / 4], 4 * (kq % 4), w3[mt * 8 + kq], acc[t]);
                }
#pragma unroll
                for (int t = 0; t < 2; ++t)
#pragma unroll
                    for (int j = 0; j < 2; ++j) {
                        int m = 0;
#pragma unroll
                        for (int i = 8 * j; i < 8 * j + 8; i += 2)
                            m = max(max(m, __float_as_int(acc[t][i])), __float_as_int(acc[t][i + 1]));
                        __hip_atomic_fetch_max((lds_int*)(size_t)(own[t][j] + 128 * mt), m, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_WAVEFRONT);
                    }
            }
        }
        // other lanes of this wave wrote the rows a lane reads now: a wavefront-scope fence (no instruction) states it
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        if (feat) {                    // the debug copy of feat1 (one uniform branch per group)
            for (int r = 0; r < n; ++r) {
                float* o = feat + (size_t)(g0 + r) * 128 + lane;
                o[0] = stage[r * SA1_PITCH + lane], o[64] = stage[r * SA1_PITCH + 64 + lane];
            }
        }
        sa1_p2_tile(wl + opaque_zero(), stage, P, g0, n, lane);
        if (!nb1) break;
        g0 = g1, buf ^= 1, nb = nb1, base_lo = base_lo1, bound64 = bound641;
    }
}

// ---- the order in which a persistent wave visits its centres, and the shared tile (SPEC 4.5) -------------------------
// A ball row with d <= 48 distinct hits repeats its first hit in slots 48..63, and the pool is a max: those 16 columns
// cannot change it. Such a row is SMALL, and it shows without a count: hits are distinct and ascending and the padding is
// the first hit, so a row is small iff slot 48 equals slot 0. A small centre needs slots 0..47 only, a tile and a half --
// and the last layer, run with its operands swapped, keeps the halves of a tile apart by itself: sample column c lands in
// lane half (c >> 2) & 1 (row 8(r>>2) + 4h + (r&3) of the accumulator, see mfma4_swapped), so pool_acc returns one maximum
// per lane half and they meet only in pool_halves. A SHARED tile S(A, B) carries slots 32..47 of small centre A in the 16
// columns with bit 2 clear and those of small centre B in the 16 columns with bit 2 set, each column with its own centre's
// coordinates and gather base; lane half 0 of its pool belongs to A, lane half 1 to B. Two small centres then cost three
// tiles (A.0, S, B.0) instead of four, and every value is what it was: the same fmaf chain per column, a max over the same
// set of values.
//
// The schedule is wave-uniform and lives in scalar registers. A wave's slice [first, end) is cut into groups of 32
// consecutive centres from its start (the last one partial). Per group, lanes 0..31 load slot 0 and slot 48 of their
// centre's row -- a group ahead, there is no partner wave to cover the latency -- and a ballot of their equality is the
// group's mask of small centres. The wave visits the group's large centres in ascending order, then its small ones in
// ascending order in pairs (1st with 2nd, 3rd with 4th, ...); an odd last one runs as an ordinary two-tile centre. A pair
// may straddle a hypothesis boundary: its two centres carry a hypothesis each. (sa2_kernel walks this way; sa1_kernel
// visits its slice in ascending order and packs granules of 8 columns instead, see its granule stream.)
enum { T_FIRST = 0, T_SECOND = 1, T_SHARED = 2, T_LAST = 3 };   // slots 0..31 of a | 32..63 of a | S(a, b) | 0..31 of b

struct CentreWalk {
    const int* ball;
    int end, np, c;                // the slice's end, centres per hypothesis, lane & 31
    int g0, gh, gr;                // the group's first centre, its hypothesis and its place in it
    unsigned large, small;         // the group's centres not yet visited (bit j = centre g0 + j)
    int n0, n48;                   // slots 0 and 48 of the NEXT group's rows (lane j and 32 + j: centre g0 + 32 + j)
    int a, b, ha, hb;              // the centre(s) being visited and their hypotheses; a == b unless paired
    int kind;                      // sa2_kernel walks tile by tile

    __device__ __forceinline__ void load_rows(int g) {
        const int ce = min(g + c, end - 1);
        n0 = ball[(size_t)ce * 64], n48 = ball[(size_t)ce * 64 + 48];
    }
    __device__ __forceinline__ void open_group(int g) {
        g0 = g;
        const int left = __builtin_amdgcn_readfirstlane(end - g);
        const unsigned valid = left >= 32 ? ~0u : (1u << left) - 1u;
        const unsigned sm = __builtin_amdgcn_readfirstlane((unsigned)__builtin_amdgcn_ballot_w64(n0 == n48));
        small = sm & valid, large = ~sm & valid;
        load_rows(min(g + 32, end - 1));
    }
    __device__ __forceinline__ void start(const int* ball_, int first, int end_, int np_, int c_) {
        ball = ball_, end = end_, np = np_, c = c_;
        gh = first / np, gr = first % np;
        load_rows(first);
        open_group(first);
        next_centre();
        kind = T_FIRST;
    }
    __device__ __forceinline__ int hyp(int ce) const {
        int h = gh, r = gr + (ce - g0);
        while (r >= np) r -= np, ++h;
        return h;
    }
    // the next centre, or pair of small centres, of the schedule; false (and nothing changed) when the slice is done
    __device__ __forceinline__ bool next_centre() {
        if (!(large | small)) {
            if (g0 + 32 >= end) return false;
            gr += 32;
            while (gr >= np) gr -= np, ++gh;
            open_group(g0 + 32);
        }
        if (large) {
            a = b = g0 + __builtin_ctz(large), large &= large - 1;
        } else {
            a = b = g0 + __builtin_ctz(small), small &= small - 1;
            if (small) b = g0 + __builtin_ctz(small), small &= small - 1;
        }
        ha = hyp(a), hb = hyp(b);
        return true;
    }
    // the next TILE: a two-tile centre is FIRST, SECOND; a pair is FIRST (of a), SHARED, LAST (of b)
    __device__ __forceinline__ bool next_tile() {
        if (kind == T_FIRST) {
            kind = a != b ? T_SHARED : T_SECOND;
        } else if (kind == T_SHARED) {
            a = b, ha = hb, kind = T_LAST;
        } else {
            if (!next_centre()) return false;
            kind = T_FIRST;
        }
        return true;
    }
};

// ---- SA2: (P gather + xyz columns) -> relu -> 128 -> 256 -> max over 64 samples ----------------------
// Persistent like sa1_kernel: one 4-wave workgroup per CU, one wave per SIMD, every wave walking a contiguous slice of the
// B * np2 centres in the order of CentreWalk above, tile by tile: a centre's two 32-sample column tiles one after the other,
// or three tiles for a pair of small centres. What sa1 measured holds here: the kernel's
// loss is its count of vector / LDS / memory instructions, so the design keeps operands where an MFMA reads them in place.
//   middle layer 128 -> 128: its 64 weight quads are loaded once per wave and pinned to the AGPR half (256 registers): no
//     LDS ring, no LDS-DMA, no barrier after the prologue -- the four waves run free of each other;
//   last layer 128 -> 256: its 128 KB stay in LDS for the kernel's lifetime (they do not fit beside the middle layer), read
//     one group of four quads ahead of the MFMAs that use them, with one s_waitcnt per group; b2 is read from LDS a tile
//     ahead (its four ready-made tiles would take the budget past 256 vector registers), and b3 too, as ready-made
//     accumulator tiles of the swapped form (16 copies of the lane's bias: four ds_read_b128 instead of 16 v_mov);
//   xyz columns: X1 = relu(fma(wz,dz, fma(wy,dy, fma(wx,dx, P)))) is the matrix core's own chain. The gathered P quads
//     already have the accumulator layout (register 4q+e of half h = channel 32kt+8q+4h+e, column = sample), so an m-tile
//     of X1 is two MFMAs with P as the C operand: k = (x, y), then k = (z, 0). The padding product fma(0, 0, acc) returns
//     acc (a -0 becomes +0, which the ReLU that follows does anyway);
//   the first tile's pooled maxima wait in 8 registers, not in LDS.
// Register budget per lane: AGPR half = W2 256. Vector half: X1 64 (the next tile's 16-quad gather lands in the same
// registers under the last layer, when X1 is dead) + Y2 64 + accumulator 16 + W3 read buffers 32 + the bias tile read
// ahead 16 + xyz weights 8 + kept maxima 8 + addressing. tests/test_pn2_resources_sa2_sa3.py holds the build to zero scratch.
constexpr int SA2_W3 = 0, SA2_B2 = 32768, SA2_B3S = SA2_B2 + 128,
              SA2_SLICE = SA2_B3S + 8 * 4 * 32 * 4,        // W3p 128 KB | b2 | b3 splat tiles 16 KB | wave_slice's scratch
              SA2_LDS_FLOATS = SA2_SLICE + 4 * 128;        // = 150 016 B

__global__ __launch_bounds__(256, 1) void sa2_kernel(const float* __restrict__ P, const float* __restrict__ xyz1,
                                                     int np1, const int* __restrict__ ball,
                                                     const float* __restrict__ cxyz, int np2, int total,
                                                     const unsigned char* __restrict__ hits,
                                                     const int* __restrict__ part, int ppb, int cpb,
                                                     const float* __restrict__ wxyz,
                                                     const float* __restrict__ W2p, const float* __restrict__ b2,
                                                     const float* __restrict__ W3p, const float* __restrict__ b3,
                                                     float* __restrict__ feat) {
    extern __shared__ __attribute__((aligned(16))) float wl[];
    const int lane = threadIdx.x & 63, h = lane >> 5, c = lane & 31;
    stage_lds(wl + SA2_W3, W3p, 32768);
    stage_lds(wl + SA2_B2, b2, 128);
    {   // b3 as ready-made accumulator tiles of the swapped form: [m-tile][register quad][channel c] x 4 copies of b3[32 mt + c]
        const float v = b3[threadIdx.x];
#pragma unroll
        for (int q = 0; q < 4; ++q)
            *(float4*)(wl + SA2_B3S + (((threadIdx.x >> 5) * 4 + q) * 32 + (threadIdx.x & 31)) * 4) = make_float4(v, v, v, v);
    }
    __syncthreads();                   // the only barrier: every wave passes it before any may leave
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int gw = blockIdx.x * 4 + wave, nw = gridDim.x * 4;
    int first, end;                    // the slice, cut by work in half tiles (3 for a small centre, 4 for a large one)
    wave_slice(SliceCosts{part, hits, (total / np2) * ppb, ppb, cpb, np2, total, 1}, gw, nw, (int*)(wl + SA2_SLICE) + wave * 128,
               lane, first, end);
    if (first >= end) return;          // nothing to do
    float4 w2[64];
    load_quads(w2, W2p, lane);
    // A operands of the xyz step for m-tile kt: lane half 0 carries (wx, wz), half 1 (wy, 0), of channel 32 kt + c
    float a_xy[4], a_z[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
        a_xy[kt] = wxyz[h * 128 + kt * 32 + c];
        const float z = wxyz[256 + kt * 32 + c];
        a_z[kt] = h ? 0.0f : z;
    }

    // The gather of the next tile of the walk is issued a tile ahead, in two steps (there is no partner wave to cover a
    // memory latency): its sample index and centre under this tile's first layers, its 16 P quads and the sample's xyz under
    // this tile's last layer. Centre, hypothesis and slot are per column: in a shared tile the columns with bit 2 set
    // belong to centre b (in every other tile a == b).
    CentreWalk nx;                     // the NEXT tile
    nx.start(ball, first, end, np2, c);
    const bool colb = (c >> 2) & 1;
    const int slot16 = 32 + ((c & 3) | ((c >> 3) << 2));   // a shared tile's slot of column c: 32..47 in each half-set
    int inext;
    float s_xy, s_z, c_xy, c_z;        // sample and centre coordinates: half 0 holds (x, z), half 1 (y, -)
    v16f X1[4];
    auto fetch_index = [&]() {
        const int ce = colb && nx.kind == T_SHARED ? nx.b : nx.a;
        const int slot = nx.kind == T_SHARED ? slot16 : nx.kind == T_SECOND ? c + 32 : c;
        inext = ball[(size_t)ce * 64 + slot];
        c_xy = cxyz[(size_t)ce * 3 + h], c_z = cxyz[(size_t)ce * 3 + 2];
    };
    auto fetch_rows = [&]() {
        int i0 = inext;
        asm volatile("" : "+v"(i0));   // consumed HERE, not behind its load (see sa1_kernel)
        const size_t pt = (size_t)(colb && nx.kind == T_SHARED ? nx.hb : nx.ha) * np1 + i0;
        s_xy = xyz1[pt * 3 + h], s_z = xyz1[pt * 3 + 2];
        const float* r = P + pt * 128 + 4 * h;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const float4 v = *(const float4*)(r + kt * 32 + 8 * q);
                X1[kt][4 * q + 0] = v.x;
                X1[kt][4 * q + 1] = v.y;
                X1[kt][4 * q + 2] = v.z;
                X1[kt][4 * q + 3] = v.w;
            }
    };
    fetch_index();
    fetch_rows();
    constexpr int G = 4;               // W3 quads per LDS read group: 16 MFMAs = 1024 pipe cycles cover the next group's reads
    float4 cur[G], nxt[G];
    {
        const float4* w3 = (const float4*)(wl + SA2_W3) + lane;
#pragma unroll
        for (int i = 0; i < G; ++i) cur[i] = w3[i * 64];
    }
    // the last layer's accumulator starts as 16 copies of the lane's bias: four 16-byte LDS reads of a ready-made tile
    // instead of 16 register moves, issued an m-tile ahead like the weights
    auto b3_tile = [&](const float* w, int mt) {
        v16f a;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 t = *(const float4*)(w + SA2_B3S + ((mt * 4 + q) * 32 + c) * 4);
            a[4 * q + 0] = t.x, a[4 * q + 1] = t.y, a[4 * q + 2] = t.z, a[4 * q + 3] = t.w;
        }
        return a;
    };
    v16f bs = b3_tile(wl, 0);
    int kp[8];                         // the centre's running maxima, as bit patterns (see pool_acc)
#pragma unroll
    for (int mt = 0; mt < 8; ++mt) kp[mt] = 0;
#pragma unroll 1
    for (;;) {
        const float* w = wl + opaque_zero();      // keeps the LDS reads of this iteration inside it
        const int centre = nx.a, kind = nx.kind;  // this tile: what it pools into and which centre it completes
        const float d_xy = s_xy - c_xy, d_z = h ? 0.0f : s_z - c_z;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) X1[kt] = relu16(mfma(a_z[kt], d_z, mfma(a_xy[kt], d_xy, X1[kt])));
        const bool more = nx.next_tile();         // (the last tile prefetches itself: harmless)
        __builtin_amdgcn_sched_barrier(0);
        fetch_index();
        __builtin_amdgcn_sched_barrier(0);
        v16f Y2[4];
        v16f bt = bias_tile(w + SA2_B2, 0, h);
#pragma unroll
        for (int mt = 0; mt < 4; ++mt) {
            v16f acc = bt;
            if (mt < 3) bt = bias_tile(w + SA2_B2, mt + 1, h);   // read a tile ahead: nobody covers an LDS latency here
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int kq = 0; kq < 16; ++kq) acc = mfma4(w2[mt * 16 + kq], X1[kq / 4], 4 * (kq % 4), acc);
            Y2[mt] = relu16(acc);
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_sched_barrier(0);
        fetch_rows();                                          // in flight under the last layer; X1 is dead
        __builtin_amdgcn_sched_barrier(0);
        // last layer, operands swapped (see mfma4_swapped); the read of the group after the last wraps to quad 0, which is
        // the next tile's first
        const float4* w3 = (const float4*)(w + SA2_W3) + lane;
        float* out = feat + (size_t)centre * 256 + lane;
        int fprev = 0;
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) {
            v16f acc = bs;
#pragma unroll
            for (int g = 0; g < 16 / G; ++g) {
                constexpr int LASTG = 16 / G - 1;
#pragma unroll
                for (int i = 0; i < G; ++i) nxt[i] = w3[((mt * 16 + (g + 1) * G + i) & 127) * 64];
                if (g == LASTG) bs = b3_tile(w, (mt + 1) & 7);
                __builtin_amdgcn_sched_barrier(0);
                // ONE wait for the group, not one per quad: LDS reads return in order, so everything but the reads just
                // issued (G weight quads, and the 4 of the bias tile behind the m-tile's last group) has landed
                if (g == LASTG)
                    __builtin_amdgcn_s_waitcnt(0xC07F | ((G + 4) << 8));   // lgkmcnt(G + 4)
                else
                    __builtin_amdgcn_s_waitcnt(0xC07F | (G << 8));         // lgkmcnt(G)
#pragma unroll
                for (int i = 0; i < G; ++i) {
                    const int kq = g * G + i;
                    acc = mfma4_swapped(Y2[kq / 4], 4 * (kq % 4), cur[i], acc);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < G; ++i) cur[i] = nxt[i];
            }
            if (kind == T_SHARED) {
                // lane half 0 of the tile's maxima completes centre a, whose first tile waits in kp; lane half 1 starts the
                // chain of centre b, whose own tile comes next
                const int p = pool_acc(acc, 0);
                const int fa = max(kp[mt], h ? 0 : p);
                kp[mt] = h ? p : 0;
                if (mt & 1)
                    out[(mt - 1) * 32] = pool_halves(fprev, fa);
                else
                    fprev = fa;
            } else {
                // the kept maximum of the centre's earlier tiles (or the 0 of a fresh centre, which is the ReLU) starts the
                // chain; the lane halves are merged once per centre, below
                kp[mt] = pool_acc(acc, kp[mt]);
            }
        }
        if (kind == T_SECOND || kind == T_LAST) {
            // after the merge both lane halves hold every tile's 32 maxima, so one full-wave store writes two m-tiles
            // (lane = 32 h + c)
#pragma unroll
            for (int mt = 0; mt < 8; mt += 2) out[mt * 32] = pool_halves(kp[mt], kp[mt + 1]);
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) kp[mt] = 0;
        }
        if (!more) break;
    }
}

// ---- SA3 (GroupAll): (feat2, xyz2) K=264 -> 256 -> 512 -> 1024 -> max over all np2 points -----------
// One workgroup per hypothesis, one 32-point column tile per wave at a time, one wave per SIMD
// (the 256->512 layer keeps 128 + 256 accumulator registers live).
__global__ __launch_bounds__(256, 1) void sa3_kernel(const float* __restrict__ feat2, const float* __restrict__ xyz2,
                                                     int np2, const float* __restrict__ W1p,
                                                     const float* __restrict__ b1, const float* __restrict__ W2p,
                                                     const float* __restrict__ b2, const float* __restrict__ W3p,
                                                     const float* __restrict__ b3, float* __restrict__ feat3) {
    __shared__ float red[4][1024];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, c = lane & 31;
    const int n = blockIdx.x;
    for (int i = tid; i < 4096; i += 256) (&red[0][0])[i] = -INFINITY;
    __syncthreads();
    const int ntiles = np2 / 32;
#pragma unroll 1
    for (int t = wave; t < ntiles; t += 4) {
        W1p = opaque(W1p), W2p = opaque(W2p), W3p = opaque(W3p);
        b1 = opaque(b1), b2 = opaque(b2), b3 = opaque(b3);
        const size_t pt = (size_t)n * np2 + t * 32 + c;
        const float* r = feat2 + pt * 256 + 4 * h;
        v16f Y1[1][8], Y2[1][16];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) Y1[0][mt] = bias_tile(b1, mt, h);
        // first layer, k-outer: one activation quad (this lane's 4 channels of block kb) against the
        // eight output tiles; weights [8][33][64][4]. Two-deep pipeline over kb like stream_layer.
        const float4* W4 = (const float4*)W1p + lane;
        float4 bc = *(const float4*)(r), bn;
        float4 ac[8], an[8];
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) ac[mt] = W4[(size_t)(mt * 33) * 64];
#pragma unroll 1
        for (int kb = 0; kb < 33; ++kb) {
            const int kn = kb + 1 < 33 ? kb + 1 : 32;
            if (kn < 32) {
                bn = *(const float4*)(r + 8 * kn);
            } else {  // the (x, y, z, 0 | 0, 0, 0, 0) block
                bn = make_float4(0.f, 0.f, 0.f, 0.f);
                if (h == 0) {
                    bn.x = xyz2[pt * 3];
                    bn.y = xyz2[pt * 3 + 1];
                    bn.z = xyz2[pt * 3 + 2];
                }
            }
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) an[mt] = W4[(size_t)(mt * 33 + kn) * 64];
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) {
                Y1[0][mt] = mfma(ac[mt].x, bc.x, Y1[0][mt]);
                Y1[0][mt] = mfma(ac[mt].y, bc.y, Y1[0][mt]);
                Y1[0][mt] = mfma(ac[mt].z, bc.z, Y1[0][mt]);
                Y1[0][mt] = mfma(ac[mt].w, bc.w, Y1[0][mt]);
            }
            __builtin_amdgcn_sched_barrier(0);
            bc = bn;
#pragma unroll
            for (int mt = 0; mt < 8; ++mt) ac[mt] = an[mt];
        }
        // Y1 and the first half of Y2 are from here on only MFMA operands: they move to the accumulator half of the register
        // file once, as they are made, and the MFMAs read them there (see pin_acc16)
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) Y1[0][mt] = relu16(Y1[0][mt]), pin_acc16(Y1[0][mt]);
        stream_layer<8, 16, 1, 4>(W2p, lane * 16, b2, Y1, h, [&](int mt, v16f(&acc)[1]) { Y2[0][mt] = relu16(acc[0]); });
#pragma unroll
        for (int mt = 0; mt < 8; ++mt) pin_acc16(Y2[0][mt]);
        stream_last_layer<16, 1, 8>(W3p, lane * 16, b3, Y2, c, 32, [&](int mt, v16f(&acc)[1]) {
            const float v = pool_swapped(acc[0]);
            if (h == 0) {
                float* sl = &red[wave][mt * 32 + c];
                *sl = fmaxf(*sl, v);
            }
        });
    }
    __syncthreads();
    for (int o = tid; o < 1024; o += 256)
        feat3[(size_t)n * 1024 + o] = fmaxf(fmaxf(red[0][o], red[1][o]), fmaxf(red[2][o], red[3][o]));
}

// ---- FC head 1024 -> 512 -> 256 -> 1, eight hypotheses per workgroup ---------------------------------
// Weights are stored transposed [k][cout] so a wave's loads are contiguous; activations sit in LDS.
constexpr int FC_HB = 8;
__device__ __forceinline__ int canon(int e) { return (e >> 1) + 4 * (e & 1); }  // 0,4,1,5,2,6,3,7

__global__ __launch_bounds__(256) void fc_head_kernel(const float* __restrict__ feat3, int B,
                                                      const float* __restrict__ Wt1, const float* __restrict__ bb1,
                                                      const float* __restrict__ Wt2, const float* __restrict__ bb2,
                                                      const float* __restrict__ W3, const float* __restrict__ bb3,
                                                      float* __restrict__ scores) {
    __shared__ float x[FC_HB][1024];
    __shared__ float h1[FC_HB][512];
    __shared__ float h2[FC_HB][256];
    const int tid = threadIdx.x;
    const int b0 = blockIdx.x * FC_HB;
    for (int i = tid; i < FC_HB * 1024; i += 256) {
        int hb = i >> 10, k = i & 1023;
        x[hb][k] = (b0 + hb < B) ? feat3[(size_t)(b0 + hb) * 1024 + k] : 0.0f;
    }
    __syncthreads();
    {
        float acc[2][FC_HB];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int hb = 0; hb < FC_HB; ++hb) acc[j][hb] = bb1[tid + 256 * j];
        for (int kb = 0; kb < 1024; kb += 8)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = kb + canon(e);
                const float w0 = Wt1[(size_t)k * 512 + tid], w1 = Wt1[(size_t)k * 512 + tid + 256];
#pragma unroll
                for (int hb = 0; hb < FC_HB; ++hb) {
                    const float xv = x[hb][k];
                    acc[0][hb] = fmaf(w0, xv, acc[0][hb]);
                    acc[1][hb] = fmaf(w1, xv, acc[1][hb]);
                }
            }
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int hb = 0; hb < FC_HB; ++hb) h1[hb][tid + 256 * j] = fmaxf(acc[j][hb], 0.0f);
    }
    __syncthreads();
    {
        float acc[FC_HB];
#pragma unroll
        for (int hb = 0; hb < FC_HB; ++hb) acc[hb] = bb2[tid];
        for (int kb = 0; kb < 512; kb += 8)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = kb + canon(e);
                const float w = Wt2[(size_t)k * 256 + tid];
#pragma unroll
                for (int hb = 0; hb < FC_HB; ++hb) acc[hb] = fmaf(w, h1[hb][k], acc[hb]);
            }
#pragma unroll
        for (int hb = 0; hb < FC_HB; ++hb) h2[hb][tid] = fmaxf(acc[hb], 0.0f);
    }
    __syncthreads();
    if (tid < FC_HB && b0 + tid < B) {
        float acc = bb3[0];
        for (int kb = 0; kb < 256; kb += 8)
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int k = kb + canon(e);
                acc = fmaf(W3[k], h2[tid][k], acc);
            }
        scores[b0 + tid] = acc;
    }
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Workspace {
    int* fps1;
    float* xyz1;
    int* ball1;
    float* feat1;
    float* p2;
    int* fps2;
    float* xyz2;
    int* ball2;
    float* feat2;
    float* feat3;
    unsigned char *hits1, *hits2;      // the centres' hit counts and the ball-query workgroups' cost totals (slice_balance.h)
    int *part1, *part2;
    size_t bytes;
};

Workspace carve(char* base, int B, int M, int np1, int np2) {
    Workspace w;
    size_t off = 0;
    auto take = [&](size_t n) {
        char* p = base ? base + off : nullptr;
        off += align256(n);
        return p;
    };
    w.fps1 = (int*)take((size_t)B * np1 * 4);
    w.xyz1 = (float*)take((size_t)B * np1 * 12);
    w.ball1 = (int*)take((size_t)B * np1 * 64 * 4);
    w.feat1 = (float*)take((size_t)B * np1 * 128 * 4);
    w.p2 = (float*)take((size_t)B * np1 * 128 * 4);
    w.fps2 = (int*)take((size_t)B * np2 * 4);
    w.xyz2 = (float*)take((size_t)B * np2 * 12);
    w.ball2 = (int*)take((size_t)B * np2 * 64 * 4);
    w.feat2 = (float*)take((size_t)B * np2 * 256 * 4);
    w.feat3 = (float*)take((size_t)B * 1024 * 4);
    w.hits1 = (unsigned char*)take((size_t)B * np1);
    w.hits2 = (unsigned char*)take((size_t)B * np2);
    w.part1 = (int*)take((size_t)B * ball_parts(M, np1) * 4);
    w.part2 = (int*)take((size_t)B * ball_parts(np1, np2) * 4);
    w.bytes = off;
    return w;
}

template <int P>
int launch_fps_reg(const float* xyz, int stride, int B, int n, int npoint, int* idx, float* new_xyz, hipStream_t s) {
    // points (16 B each) and the picked-index list: at most 3072 * 16 + 3072 * 4 bytes, under the 64 KiB every launch may have
    const size_t lds = (size_t)n * 16 + (size_t)npoint * 4;
    hipLaunchKernelGGL(fps_reg_kernel<P>, dim3(B), dim3(256), lds, s, xyz, stride, n, npoint, idx, new_xyz);
    return ossid_launch_status();
}

int launch_fps(const float* xyz, int stride, int B, int n, int npoint, int* idx, float* new_xyz, hipStream_t s) {
    if (n <= FPS_REG_MAX_N && npoint <= FPS_REG_MAX_NPOINT) {
        if (n <= 256 * 2) return launch_fps_reg<2>(xyz, stride, B, n, npoint, idx, new_xyz, s);
        if (n <= 256 * 4) return launch_fps_reg<4>(xyz, stride, B, n, npoint, idx, new_xyz, s);
        if (n <= 256 * 8) return launch_fps_reg<8>(xyz, stride, B, n, npoint, idx, new_xyz, s);
        return launch_fps_reg<12>(xyz, stride, B, n, npoint, idx, new_xyz, s);
    }
    // larger sets (or more picks than the register form lists): points and running distances in LDS
    size_t lds = (size_t)n * 20 + FPS_LDS_SLOT_BYTES;
    if (lds > 160 * 1024 - 1024) return OSSID_EINVAL;
    OSSID_ENSURE_LDS(fps_kernel, lds);
    hipLaunchKernelGGL(fps_kernel, dim3(B), dim3(256), lds, s, xyz, stride, n, npoint, idx, new_xyz);
    return ossid_launch_status();
}

// What the ball query tells the SA kernel that reads its rows (null pointers: nothing): the centres' hit counts, the cost
// total of each workgroup's centres in the unit of `sa2` (ball_cpb says how many centres a workgroup takes).
struct BallCosts {
    unsigned char* hits;
    int* part;
    int sa2;
};

template <int NCH>
int launch_ball_reg(const float* xyz, int stride, int B, int n, const float* new_xyz, int npoint, float r2, int* idx,
                    const BallCosts& k, hipStream_t s) {
    hipLaunchKernelGGL(ball_query_reg_kernel<NCH>, dim3(B, (npoint + BQR_CPB - 1) / BQR_CPB), dim3(BQR_THREADS), 0, s, xyz,
                       stride, n, new_xyz, npoint, r2, idx, k.hits, k.part, k.sa2);
    return ossid_launch_status();
}

int launch_ball(const float* xyz, int stride, int B, int n, const float* new_xyz, int npoint, float radius, int* idx,
                const BallCosts& k, hipStream_t s) {
    const float r2 = radius * radius;
    if (n <= 64 * 8) return launch_ball_reg<8>(xyz, stride, B, n, new_xyz, npoint, r2, idx, k, s);
    if (n <= 64 * 16) return launch_ball_reg<16>(xyz, stride, B, n, new_xyz, npoint, r2, idx, k, s);
    if (n <= 64 * 32) return launch_ball_reg<32>(xyz, stride, B, n, new_xyz, npoint, r2, idx, k, s);
    if (n <= BQR_MAX_N) return launch_ball_reg<48>(xyz, stride, B, n, new_xyz, npoint, r2, idx, k, s);
    // larger sets: the points stay in LDS
    size_t lds = (size_t)n * 16;
    if (lds > 160 * 1024 - 1024) return OSSID_EINVAL;
    lds += (BQ_THREADS / 64) * 4;      // the waves' cost totals
    OSSID_ENSURE_LDS(ball_query_kernel, lds);
    hipLaunchKernelGGL(ball_query_kernel, dim3(B, (npoint + BQ_CPB - 1) / BQ_CPB), dim3(BQ_THREADS), lds, s, xyz, stride,
                       n, new_xyz, npoint, r2, idx, k.hits, k.part, k.sa2);
    return ossid_launch_status();
}

}  // namespace

extern "C" {

int ossid_pn2_fps(const float* xyz, int stride, int B, int n, int npoint, int32_t* idx, float* new_xyz,
                  void* stream) {
    if (B < 0 || n <= 0 || npoint <= 0 || stride < 3) return OSSID_EINVAL;
    if (B == 0) return OSSID_OK;
    if (!xyz || !idx || !new_xyz) return OSSID_EINVAL;
    return launch_fps(xyz, stride, B, n, npoint, idx, new_xyz, (hipStream_t)stream);
}

int ossid_pn2_ball_query(const float* xyz, int stride, int B, int n, const float* new_xyz, int npoint, float radius,
                         int nsample, int32_t* idx, void* stream) {
    if (B < 0 || n <= 0 || npoint <= 0 || stride < 3 || nsample != 64) return OSSID_EINVAL;
    if (B == 0) return OSSID_OK;
    if (!xyz || !idx || !new_xyz) return OSSID_EINVAL;
    return launch_ball(xyz, stride, B, n, new_xyz, npoint, radius, idx, BallCosts{nullptr, nullptr, 0}, (hipStream_t)stream);
}

size_t ossid_pn2_workspace_bytes(int B, int M, int npoint1, int npoint2) {
    if (B <= 0) return 256;
    return carve(nullptr, B, M, npoint1, npoint2).bytes;
}

const char* ossid_pn2_stage_names(void) { return "fps1,ball1,sa1,p2,fps2,ball2,sa2,sa3,fc"; }

int ossid_event_create(void** event_out_host) {
    if (!event_out_host) return OSSID_EINVAL;
    hipEvent_t e;
    if (hipEventCreate(&e) != hipSuccess) return OSSID_ELAUNCH;
    *event_out_host = (void*)e;
    return OSSID_OK;
}
int ossid_event_destroy(void* event) { return hipEventDestroy((hipEvent_t)event) == hipSuccess ? OSSID_OK : OSSID_ELAUNCH; }
int ossid_event_record(void* event, void* stream) {
    return hipEventRecord((hipEvent_t)event, (hipStream_t)stream) == hipSuccess ? OSSID_OK : OSSID_ELAUNCH;
}
int ossid_event_elapsed_ms(void* start, void* stop, float* ms_out_host) {
    if (!ms_out_host) return OSSID_EINVAL;
    if (hipEventSynchronize((hipEvent_t)stop) != hipSuccess) return OSSID_ELAUNCH;
    return hipEventElapsedTime(ms_out_host, (hipEvent_t)start, (hipEvent_t)stop) == hipSuccess ? OSSID_OK : OSSID_ELAUNCH;
}

const char* ossid_pn2_kernel_names(void) {
    return "fps_reg_kernel,fps_kernel,ball_query_reg_kernel,ball_query_kernel,sa1_kernel,sa2_kernel,sa3_kernel,fc_head_kernel";
}

// The nine stages of ossid_pn2_score, one launcher each.
}  // extern "C"
namespace {
struct Pn2Call {
    const float* point_x;
    int B, M, np1, np2;
    const ossid_pn2_weights* w;
    Workspace ws;
    hipStream_t s;
};

int pn2_check(const float* point_x, int B, int M, const ossid_pn2_weights* w, void* workspace, size_t workspace_bytes,
              void* stream, Pn2Call* c) {
    if (B < 0 || !w) return OSSID_EINVAL;
    if (B == 0) return 1;      // nothing to do
    const int np1 = w->npoint1, np2 = w->npoint2;
    if (!point_x || !workspace || !w->blob) return OSSID_EINVAL;
    if (np1 <= 0 || np2 <= 0 || np1 % 32 || np2 % 32 || M < np1 || np1 < np2) return OSSID_EINVAL;
    if ((long long)B * np1 * 64 > 0x7fffffffLL) return OSSID_EINVAL;     // sa1_kernel's maps hold ball-array offsets as ints
    if (((uintptr_t)workspace & 255) || ((uintptr_t)point_x & 15)) return OSSID_EINVAL;
    c->ws = carve((char*)workspace, B, M, np1, np2);
    if (c->ws.bytes > workspace_bytes) return OSSID_EINVAL;
    c->point_x = point_x; c->B = B; c->M = M; c->np1 = np1; c->np2 = np2; c->w = w; c->s = (hipStream_t)stream;
    return OSSID_OK;
}

int pn2_fps1(const Pn2Call& c) { return launch_fps(c.point_x, 8, c.B, c.M, c.np1, c.ws.fps1, c.ws.xyz1, c.s); }
int pn2_ball1(const Pn2Call& c) {
    return launch_ball(c.point_x, 8, c.B, c.M, c.ws.xyz1, c.np1, c.w->radius1, c.ws.ball1, BallCosts{c.ws.hits1, c.ws.part1, 0}, c.s);
}
int pn2_fps2(const Pn2Call& c) { return launch_fps(c.ws.xyz1, 3, c.B, c.np1, c.np2, c.ws.fps2, c.ws.xyz2, c.s); }
int pn2_ball2(const Pn2Call& c) {
    return launch_ball(c.ws.xyz1, 3, c.B, c.np1, c.ws.xyz2, c.np2, c.w->radius2, c.ws.ball2, BallCosts{c.ws.hits2, c.ws.part2, 1}, c.s);
}

// persistent grid of sa1_kernel and sa2_kernel: one 4-wave workgroup per CU (one wave per SIMD), cached per device --
// unless ossid_pn2_set_persistent_grid chose a size (tests: few workgroups make a wave's slice long at a small batch)
int g_persistent_workgroups = 0;
int persistent_grid() {
    if (g_persistent_workgroups) return g_persistent_workgroups;
    static int cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return 256;
    if (!cache[dev]) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) != hipSuccess || p.multiProcessorCount <= 0) return 256;
        cache[dev] = p.multiProcessorCount;
    }
    return cache[dev];
}

// feat1 leaves sa1_kernel only for the caller's debug copy: SA2 reads the layer applied to it (ws.p2), not feat1 itself
int pn2_sa1(const Pn2Call& c, bool want_feat1) {
    const float* blob = c.w->blob;
    const int total = c.B * c.np1;
    OSSID_ENSURE_LDS(sa1_kernel, (size_t)SA1_LDS_FLOATS * 4);
    hipLaunchKernelGGL(sa1_kernel, dim3(persistent_grid()), dim3(256), SA1_LDS_FLOATS * 4, c.s, c.point_x, c.M, c.ws.ball1,
                       c.ws.xyz1, c.np1, total, c.ws.hits1, c.ws.part1, ball_parts(c.M, c.np1), ball_cpb(c.M), blob + c.w->w_off[0], blob + c.w->b_off[0], blob + c.w->w_off[1],
                       blob + c.w->b_off[1], blob + c.w->w_off[2], blob + c.w->b_off[2], blob + c.w->w_off[3],
                       blob + c.w->b_off[3], want_feat1 ? c.ws.feat1 : nullptr, c.ws.p2);
    return ossid_launch_status();
}
// the "p2" stage (the per-point part of SA2's first layer) is computed by sa1_kernel: the stage keeps its name and its event
// marks, and launches nothing
int pn2_p2(const Pn2Call&) { return OSSID_OK; }
int pn2_sa2(const Pn2Call& c) {
    const float* blob = c.w->blob;
    const int total = c.B * c.np2;
    OSSID_ENSURE_LDS(sa2_kernel, (size_t)SA2_LDS_FLOATS * 4);
    hipLaunchKernelGGL(sa2_kernel, dim3(persistent_grid()), dim3(256), SA2_LDS_FLOATS * 4, c.s, c.ws.p2, c.ws.xyz1, c.np1, c.ws.ball2,
                       c.ws.xyz2, c.np2, total, c.ws.hits2, c.ws.part2, ball_parts(c.np1, c.np2), ball_cpb(c.np1),
                       blob + c.w->wxyz2_off, blob + c.w->w_off[4], blob + c.w->b_off[4],
                       blob + c.w->w_off[5], blob + c.w->b_off[5], c.ws.feat2);
    return ossid_launch_status();
}
int pn2_sa3(const Pn2Call& c) {
    const float* blob = c.w->blob;
    hipLaunchKernelGGL(sa3_kernel, dim3(c.B), dim3(256), 0, c.s, c.ws.feat2, c.ws.xyz2, c.np2, blob + c.w->w_off[6],
                       blob + c.w->b_off[6], blob + c.w->w_off[7], blob + c.w->b_off[7], blob + c.w->w_off[8],
                       blob + c.w->b_off[8], c.ws.feat3);
    return ossid_launch_status();
}
int pn2_fc(const Pn2Call& c, float* scores) {
    const float* blob = c.w->blob;
    hipLaunchKernelGGL(fc_head_kernel, dim3((c.B + FC_HB - 1) / FC_HB), dim3(256), 0, c.s, c.ws.feat3, c.B, blob + c.w->w_off[9],
                       blob + c.w->b_off[9], blob + c.w->w_off[10], blob + c.w->b_off[10], blob + c.w->w_off[11],
                       blob + c.w->b_off[11], scores);
    return ossid_launch_status();
}
}  // namespace

extern "C" {

int ossid_pn2_set_persistent_grid(int workgroups) {
    if (workgroups < 0 || workgroups > 65536) return OSSID_EINVAL;
    g_persistent_workgroups = workgroups;
    return OSSID_OK;
}

int ossid_pn2_score(const float* point_x, int B, int M, const ossid_pn2_weights* w, void* workspace,
                    size_t workspace_bytes, float* scores, int32_t* dbg_fps1, int32_t* dbg_ball1, float* dbg_feat1,
                    int32_t* dbg_fps2, int32_t* dbg_ball2, float* dbg_feat2, float* dbg_feat3,
                    void* const* stage_events_host, void* stream) {
    Pn2Call c;
    int rc = pn2_check(point_x, B, M, w, workspace, workspace_bytes, stream, &c);
    if (rc) return rc < 0 ? rc : OSSID_OK;
    if (!scores) return OSSID_EINVAL;
    const Workspace& ws = c.ws;
    const int np1 = c.np1, np2 = c.np2;
    hipStream_t s = c.s;
    int stage = 0;
    auto mark = [&]() {
        if (stage_events_host && hipEventRecord((hipEvent_t)stage_events_host[stage], s) != hipSuccess) rc = OSSID_ELAUNCH;
        ++stage;
    };
    rc = OSSID_OK;
    mark();
    if ((rc = pn2_fps1(c))) return rc;
    mark();
    if ((rc = pn2_ball1(c))) return rc;
    mark();
    if ((rc = pn2_sa1(c, dbg_feat1 != nullptr))) return rc;
    mark();
    if ((rc = pn2_p2(c))) return rc;
    mark();
    if ((rc = pn2_fps2(c))) return rc;
    mark();
    if ((rc = pn2_ball2(c))) return rc;
    mark();
    if ((rc = pn2_sa2(c))) return rc;
    mark();
    if ((rc = pn2_sa3(c))) return rc;
    mark();
    if ((rc = pn2_fc(c, scores))) return rc;
    mark();

    auto cp = [&](void* dst, const void* src, size_t n) {
        if (dst && hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, s) != hipSuccess) rc = OSSID_ELAUNCH;
    };
    cp(dbg_fps1, ws.fps1, (size_t)B * np1 * 4);
    cp(dbg_ball1, ws.ball1, (size_t)B * np1 * 64 * 4);
    cp(dbg_feat1, ws.feat1, (size_t)B * np1 * 128 * 4);
    cp(dbg_fps2, ws.fps2, (size_t)B * np2 * 4);
    cp(dbg_ball2, ws.ball2, (size_t)B * np2 * 64 * 4);
    cp(dbg_feat2, ws.feat2, (size_t)B * np2 * 256 * 4);
    cp(dbg_feat3, ws.feat3, (size_t)B * 1024 * 4);
    return rc;
}

}  // extern "C"
