// Distinct-pose selection (SPEC.md section 16): from N scored pose hypotheses keep the best K that are different objects in
// space -- greedy non-maximum suppression over poses under 8.7's MSSD distance (max over model points, min over the
// object's symmetry transforms), squared, in f64. This build's own definition; the restatement is tests/ref_pose_select.py.
//
// ossid_pose_select. Launches on the caller's stream, nothing read back, no wait between workgroups, capturable:
//   clear     selected = -1, count = 0, owner = -1, keys = 0;
//   per round r = 0 .. K-1, two launches whose grids depend on (N, M, S, K) alone:
//   pick      every eligible candidate without an owner forms the 64-bit key (order-preserving score bits, then the
//             complemented index): the greatest key is the greatest score, the lowest index among equal scores. Maxima per
//             lane over PICK_PER_LANE candidates, across the wave by shuffles, across the waves in LDS, then one integer
//             atomicMax per workgroup on keys[r]. Key 0 is no candidate (-inf maps to a key above it);
//   suppress  grid (tiles of SUP_TILE candidates, chunks of SC symmetries). keys[r] names the pick p; key 0 means the
//             candidates are exhausted and every workgroup returns. SC threads compose G = poses[p] . S each and hand it
//             on through LDS into registers, as bop_mssd_mspd_kernel does. A wave owns SUP_PER_WAVE candidates of the
//             tile: its lanes stream the points coalesced, each point is transformed under the chunk's G once and then
//             compared with the point under every candidate of the wave, so the pick's transformed points are shared;
//             running maxima per lane and (candidate, symmetry). D(n, p) <= thr holds iff some symmetry's maximum is
//             <= thr: an OR, so a wave that finds one claims the candidate by an integer compare-and-swap on owner[n],
//             and chunks in other workgroups meet there. The wave whose tile holds p writes selected[r], count and
//             owner[p] = r (unconditionally: a pose with non-finite entries is at +inf from itself).
// Exact skips only: a candidate that has an owner when the wave starts, an exhausted round, and leaving the point loop
// once every (candidate, symmetry) of the wave has a lane above thr -- every comparison is then decided. Rounds after
// exhaustion see selected[r - 1] < 0 (pick) or keys[r] = 0 (suppress) and return at once. Max, min, the integer atomicMax
// and a compare-and-swap between equal values do not depend on the order of arrival: the outputs are bit-reproducible.
#include <cmath>

#include "bop_points.h"
#include "common.h"

namespace {

constexpr int SC = 4;                 // symmetries per workgroup of the suppress kernel, held in registers (12 doubles each)
constexpr int SUP_PER_WAVE = 4;       // candidates a wave compares against the pick at once
constexpr int SUP_TILE = 4 * SUP_PER_WAVE;   // candidates per workgroup of the suppress kernel (4 waves)
constexpr int PICK_PER_LANE = 4;
constexpr int PICK_SPAN = 256 * PICK_PER_LANE;   // candidates per workgroup of the pick kernel

__global__ __launch_bounds__(256) void select_clear_kernel(int32_t* __restrict__ selected, int32_t* __restrict__ count,
                                                           int32_t* __restrict__ owner, unsigned long long* __restrict__ keys,
                                                           int N, int K) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) owner[i] = -1;
    if (i < K) selected[i] = -1, keys[i] = 0ull;
    if (i == 0) count[0] = 0;
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long w = __shfl_xor(v, m);
        v = w > v ? w : v;
    }
    return v;
}

// Unsigned integers that order like the floats: +0 and -0 meet at one value, -inf is the smallest and still above 0.
__device__ __forceinline__ unsigned int score_bits(float s) {
    const unsigned int b = s == 0.0f ? 0u : __float_as_uint(s);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__global__ __launch_bounds__(256) void select_pick_kernel(const float* __restrict__ scores, int N, float min_score,
                                                          const int32_t* __restrict__ selected,
                                                          const int32_t* __restrict__ owner,
                                                          unsigned long long* __restrict__ keys, int r) {
    if (r > 0 && selected[r - 1] < 0) return;        // exhausted in an earlier round
    __shared__ unsigned long long red[4];
    unsigned long long best = 0ull;
#pragma unroll
    for (int j = 0; j < PICK_PER_LANE; ++j) {
        const int n = blockIdx.x * PICK_SPAN + j * 256 + (int)threadIdx.x;
        if (n < N) {
            const float s = scores[n];
            if (s >= min_score && owner[n] < 0) {    // a NaN score is never eligible
                const unsigned long long key = ((unsigned long long)score_bits(s) << 32) | (unsigned long long)(0xffffffffu - (unsigned)n);
                best = key > best ? key : best;
            }
        }
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < 4; ++w) best = red[w] > best ? red[w] : best;
        if (best) atomicMax(keys + r, best);
    }
}

// One wave's SUP_PER_WAVE candidates (E, the live ones in `act`) against the chunk's transforms G over all points. FULL: the
// chunk holds SC transforms and the loops over them are straight code; otherwise `live_rt` < SC of them exist and the rest
// are neither transformed nor compared (S = 1 pays for one transform, not SC). Both conditions are workgroup-uniform.
template <bool FULL>
__device__ __forceinline__ void suppress_wave(const double (&G)[SC][12], const double (&E)[SUP_PER_WAVE][12], unsigned act,
                                              int live_rt, const float* __restrict__ points, int M, double thr, int lane,
                                              int32_t* owner_wave, int r) {
    const int live = FULL ? SC : live_rt;
    double mx[SUP_PER_WAVE][SC];
#pragma unroll
    for (int c = 0; c < SUP_PER_WAVE; ++c)
#pragma unroll
        for (int s = 0; s < SC; ++s) mx[c][s] = 0.0;
    for (int v0 = 0; v0 < M; v0 += 64) {
        const int v = v0 + lane;
        if (v < M) {
            const double x = (double)points[3 * (size_t)v], y = (double)points[3 * (size_t)v + 1],
                         z = (double)points[3 * (size_t)v + 2];
            double Xg[SC], Yg[SC], Zg[SC];
#pragma unroll
            for (int s = 0; s < SC; ++s)
                if (s < live) bop_transform(G[s], x, y, z, Xg[s], Yg[s], Zg[s]);
#pragma unroll
            for (int c = 0; c < SUP_PER_WAVE; ++c) {
                if (!((act >> c) & 1u)) continue;    // wave-uniform
                double Xe, Ye, Ze;
                bop_transform(E[c], x, y, z, Xe, Ye, Ze);
#pragma unroll
                for (int s = 0; s < SC; ++s) {
                    if (s >= live) break;
                    const double q = bop_sqdist(Xe, Ye, Ze, Xg[s], Yg[s], Zg[s]);
                    mx[c][s] = q > mx[c][s] ? q : mx[c][s];
                }
            }
        }
        // a (candidate, symmetry) with one lane above thr is decided; leave once all of the wave's are
        bool open = false;
#pragma unroll
        for (int c = 0; c < SUP_PER_WAVE; ++c)
#pragma unroll
            for (int s = 0; s < SC; ++s)
                if (((act >> c) & 1u) && s < live && !__any(mx[c][s] > thr)) open = true;
        if (!open) return;
    }
#pragma unroll
    for (int c = 0; c < SUP_PER_WAVE; ++c) {
        if (!((act >> c) & 1u)) continue;
        bool hit = false;
#pragma unroll
        for (int s = 0; s < SC; ++s) {
            const double m = wave_max_f64(mx[c][s]);
            if (s < live && m <= thr) hit = true;
        }
        if (hit && lane == 0) atomicCAS(owner_wave + c, -1, r);
    }
}

__global__ __launch_bounds__(256) void select_suppress_kernel(const double* __restrict__ poses, int N,
                                                              const float* __restrict__ points, int M,
                                                              const double* __restrict__ syms, int S, double thr,
                                                              const unsigned long long* __restrict__ keys, int r,
                                                              int32_t* __restrict__ selected, int32_t* __restrict__ count,
                                                              int32_t* owner) {
    const unsigned long long key = keys[r];
    if (key == 0ull) return;                         // exhausted: selected[r] stays -1
    const int p = (int)(0xffffffffu - (unsigned)(key & 0xffffffffull));
    const int s0 = blockIdx.y * SC, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ double Gs[SC][12];
    // slots past the end hold the last transform and are never compared (live below)
    if (threadIdx.x < SC) bop_compose(poses + 16 * (size_t)p, syms + 16 * (size_t)min(s0 + (int)threadIdx.x, S - 1), Gs[threadIdx.x]);
    __syncthreads();
    const int n0 = blockIdx.x * SUP_TILE + wv * SUP_PER_WAVE;
    // the wave's candidates still to decide, as a wave-uniform mask: in range, not the pick, without an owner
    unsigned act = 0u;
#pragma unroll
    for (int c = 0; c < SUP_PER_WAVE; ++c) {
        const int n = n0 + c;
        if (n >= N) continue;
        if (n == p) {
            if (blockIdx.y == 0 && lane == 0) selected[r] = p, count[0] = r + 1, atomicExch(owner + p, r);
            continue;
        }
        if (__builtin_amdgcn_readfirstlane(__hip_atomic_load(owner + n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) < 0) act |= 1u << c;
    }
    if (!act) return;
    double G[SC][12], E[SUP_PER_WAVE][12];
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
        for (int j = 0; j < 12; ++j) G[s][j] = Gs[s][j];
#pragma unroll
    for (int c = 0; c < SUP_PER_WAVE; ++c)
#pragma unroll
        for (int j = 0; j < 12; ++j) E[c][j] = poses[16 * (size_t)min(n0 + c, N - 1) + j];
    const int live = min(SC, S - s0);                // transforms of this chunk that exist
    if (live == SC)
        suppress_wave<true>(G, E, act, SC, points, M, thr, lane, owner + n0, r);
    else
        suppress_wave<false>(G, E, act, live, points, M, thr, lane, owner + n0, r);
}

}  // namespace

extern "C" {

int ossid_pose_select(const double* poses, const float* scores, int N, const float* points, int M, const double* symmetries,
                      int S, int K, double sep, float min_score, int32_t* selected, int32_t* count, int32_t* owner,
                      uint64_t* keys, void* stream) {
    if (!poses || !scores || !points || !symmetries || !selected || !count || !owner || !keys || N < 1 ||
        N > OSSID_SELECT_MAX_POSES || M < 1 || M > (1 << 22) || S < 1 || S > OSSID_BOP_MAX_SYMMETRIES || K < 1 ||
        K > OSSID_BOP_MAX_INSTANCES || !(sep >= 0.0) || !std::isfinite(sep) || min_score != min_score)
        return OSSID_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    const double thr = sep * sep;
    unsigned long long* k64 = (unsigned long long*)keys;
    hipLaunchKernelGGL(select_clear_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, selected, count, owner, k64, N, K);
    const dim3 pick_grid((unsigned)((N + PICK_SPAN - 1) / PICK_SPAN));
    const dim3 sup_grid((unsigned)((N + SUP_TILE - 1) / SUP_TILE), (unsigned)((S + SC - 1) / SC));
    for (int r = 0; r < K; ++r) {
        hipLaunchKernelGGL(select_pick_kernel, pick_grid, dim3(256), 0, st, scores, N, min_score, selected, owner, k64, r);
        hipLaunchKernelGGL(select_suppress_kernel, sup_grid, dim3(256), 0, st, poses, N, points, M, symmetries, S, thr, k64, r,
                           selected, count, owner);
    }
    return ossid_launch_status();
}

}  // extern "C"
