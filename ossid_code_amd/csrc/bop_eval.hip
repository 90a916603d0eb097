// BOP-19 pose errors (SPEC.md section 8): what the reference's run ends with -- scripts/online_learning.py:603-608 calls
// saveResultsBop(..., run_eval_script=True), and utils/bop_utils.py:51-53 shells out to bop_toolkit's
// scripts/eval_bop19.py --renderer_type=cpp. bop_toolkit is absent from the reference tree: the definitions are this
// build's own restatement of the published ones (Hodan et al., BOP Challenge 2020, section 2.2).
//
// ossid_bop_vsd (8.3-8.5). The two renders come from ossid_raster_depth. Launches on the caller's stream, nothing read back:
//   zero      counts = 0;
//   cost      grid (tiles of TILE pixels, estimates of a chunk). A lane takes four consecutive pixels per step (one
//             16-byte load per image where the image size allows, scalar loads otherwise). A wave whose 256 pixels are
//             empty in both renders does nothing more -- exact: such a pixel is in neither V_gt nor V_est -- and does not
//             load the observed depth. Otherwise distances, visibility and the T comparisons are computed in registers
//             in f64, every flag is counted by ballot + popcount into wave-uniform integers, the waves' counts meet in
//             LDS, and the workgroup issues one integer atomicAdd per non-zero counter. Integer sums do not depend on
//             the order of arrival: the counts are bit-reproducible;
//   finalise  e_k = (c_k + (n_U - n_I)) / n_U in f64, 1 when n_U = 0.
//
// ossid_bop_mssd_mspd (8.7). One workgroup per (estimate, SC symmetries): SC threads compose G = pose_gt . S each and hand
// it on through LDS; the vertices stream through coalesced, each is transformed and projected under pose_est once and then
// compared against the chunk's transforms held in registers (SC of them, fewer in the last chunk: S = 1 pays for one);
// running maxima of the squared distances per lane, reduced across the wave by shuffles and across the waves in LDS; the
// minimum over the chunks by atomicMin on the 64-bit pattern of the non-negative double (it orders like the value; the
// outputs start at +inf). Max and min do not depend on order. The composition, the transform and the squared distance are
// csrc/bop_points.h's, shared with csrc/pose_select.hip.
//
// ossid_bop_vsd_pairs (8.11). ossid_bop_vsd's three launches over a pair table in device memory: row p = (estimate render,
// ground-truth render, frame) picks the two images of vsd_tile, the device function both cost kernels share, so a group of
// E estimates and G instances costs E + G renders and E G cost rows. The indices are checked on the device.
//
// ossid_bop_match (8.12). clear (match = -1, tp = 0), then one wave per (group, 64 threshold columns): each lane runs
// BOP's greedy loop for its column with the matched set as a 64-bit mask in registers; no LDS; tp by integer atomicAdd,
// so nothing depends on the order of arrival.
//
// frame[] and taus[] are host arrays (checked before any launch) and travel as kernel arguments, CHUNK estimates per launch:
// a captured graph replays with the values they had at capture.
#include <cmath>

#include "bop_points.h"
#include "common.h"

namespace {

constexpr int CHUNK = 256;            // estimates per launch: frame indices travel in the kernel arguments
constexpr int TILE = 2048;            // pixels per workgroup of the cost kernel: 256 lanes x 4 pixels x 2 steps
constexpr int SC = 4;                 // symmetries per workgroup, held in registers (12 doubles each)
constexpr unsigned long long DINF = 0x7ff0000000000000ull;

struct FrameIdx {
    int32_t f[CHUNK];
};
struct Taus {
    double t[OSSID_BOP_MAX_TAUS];
};

__global__ __launch_bounds__(256) void bop_zero_kernel(int32_t* __restrict__ counts, size_t n) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) counts[i] = 0;
}

// 8.3-8.5 over this workgroup's tile of one (estimate render ze, ground-truth render zg, observed image ob, camera cam):
// the counts (n_U, n_I, c_0 .. c_{T-1}) of the tile's TILE pixels are added to row[0 .. T+2). Both cost kernels call it:
// ossid_bop_vsd with the n-th image of either stack, ossid_bop_vsd_pairs with the two images a pair row names.
template <bool VEC>
__device__ __forceinline__ void vsd_tile(const float* __restrict__ ob, const float* __restrict__ cam, int H, int W,
                                         const float* __restrict__ ze, const float* __restrict__ zg, double diameter,
                                         double delta, const Taus& taus, int T, int32_t* __restrict__ row) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t hw = (size_t)H * W;
    const double fx = (double)cam[0], fy = (double)cam[1], cx = (double)cam[2], cy = (double)cam[3];
    int nU = 0, nI = 0, c[OSSID_BOP_MAX_TAUS];      // wave-uniform
#pragma unroll
    for (int k = 0; k < OSSID_BOP_MAX_TAUS; ++k) c[k] = 0;
    const size_t tile0 = (size_t)blockIdx.x * TILE;
    for (int step = 0; step < TILE / 1024; ++step) {
        const size_t i0 = tile0 + (size_t)step * 1024 + 4 * (size_t)threadIdx.x;
        float e[4] = {0.0f, 0.0f, 0.0f, 0.0f}, g[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (VEC) {                                   // hw % 4 == 0 and 16-byte aligned bases: i0 + 3 < hw iff i0 < hw
            if (i0 < hw) {
                const float4 a = *reinterpret_cast<const float4*>(ze + i0), b = *reinterpret_cast<const float4*>(zg + i0);
                e[0] = a.x, e[1] = a.y, e[2] = a.z, e[3] = a.w, g[0] = b.x, g[1] = b.y, g[2] = b.z, g[3] = b.w;
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (i0 + j < hw) e[j] = ze[i0 + j], g[j] = zg[i0 + j];
        }
        const bool any = e[0] > 0.0f || e[1] > 0.0f || e[2] > 0.0f || e[3] > 0.0f || g[0] > 0.0f || g[1] > 0.0f ||
                         g[2] > 0.0f || g[3] > 0.0f;
        if (__ballot(any) == 0ull) continue;         // wave-uniform
        float o[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (any) {
            if (VEC) {
                const float4 a = *reinterpret_cast<const float4*>(ob + i0);
                o[0] = a.x, o[1] = a.y, o[2] = a.z, o[3] = a.w;
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (i0 + j < hw) o[j] = ob[i0 + j];
            }
        }
        int y = (int)(i0 / (size_t)W), x = (int)(i0 - (size_t)y * W);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            bool inU = false, inI = false;
            double d = 0.0;
            if (e[j] > 0.0f || g[j] > 0.0f) {
                const double a = ((double)x - cx) / fx, b = ((double)y - cy) / fy;
                const double s = sqrt((a * a + b * b) + 1.0);
                const double De = (double)e[j] * s, Dg = (double)g[j] * s, Do = (double)o[j] * s;
                const bool oinv = !(o[j] > 0.0f);
                const bool vg = Dg > 0.0 && (oinv || Dg - Do <= delta);
                const bool ve = (De > 0.0 && (oinv || De - Do <= delta)) || (vg && De > 0.0);
                inU = vg || ve, inI = vg && ve;
                d = fabs(Dg - De) / diameter;
            }
            nU += __popcll(__ballot(inU));
            const unsigned long long bi = __ballot(inI);
            if (bi != 0ull) {
                nI += __popcll(bi);
#pragma unroll
                for (int k = 0; k < OSSID_BOP_MAX_TAUS; ++k)
                    if (k < T) c[k] += __popcll(__ballot(inI && d >= taus.t[k]));
            }
            if (++x == W) x = 0, ++y;
        }
    }
    __shared__ int part[4][OSSID_BOP_MAX_TAUS + 2];
    if (lane == 0) {
        part[wv][0] = nU, part[wv][1] = nI;
#pragma unroll
        for (int k = 0; k < OSSID_BOP_MAX_TAUS; ++k) part[wv][2 + k] = c[k];
    }
    __syncthreads();
    if ((int)threadIdx.x < T + 2) {
        const int v = (part[0][threadIdx.x] + part[1][threadIdx.x]) + (part[2][threadIdx.x] + part[3][threadIdx.x]);
        if (v) atomicAdd(row + threadIdx.x, v);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void bop_vsd_kernel(const float* __restrict__ depth_obs, const float* __restrict__ cams,
                                                      int H, int W, const float* __restrict__ z_est,
                                                      const float* __restrict__ z_gt, FrameIdx frames, double diameter,
                                                      double delta, Taus taus, int T, int32_t* __restrict__ counts) {
    const int n = blockIdx.y, fr = frames.f[n];
    const size_t hw = (size_t)H * W;
    vsd_tile<VEC>(depth_obs + (size_t)fr * hw, cams + 4 * fr, H, W, z_est + (size_t)n * hw, z_gt + (size_t)n * hw, diameter, delta,
                  taus, T, counts + (size_t)n * (T + 2));
}

// 8.11: row p of the pair table names an estimate render, a ground-truth render and a frame. The three indices are the
// same for the whole workgroup; a row with one of them out of range reads no image and leaves its (zeroed) counts alone,
// which finalise turns into e = 1.
template <bool VEC>
__global__ __launch_bounds__(256) void bop_vsd_pairs_kernel(const float* __restrict__ depth_obs, const float* __restrict__ cams,
                                                            int Fr, int H, int W, const float* __restrict__ z_est, int Ne,
                                                            const float* __restrict__ z_gt, int Ng,
                                                            const int32_t* __restrict__ pairs, double diameter, double delta,
                                                            Taus taus, int T, int32_t* __restrict__ counts) {
    const size_t p = blockIdx.y;
    const int e = pairs[3 * p], g = pairs[3 * p + 1], fr = pairs[3 * p + 2];
    if (e < 0 || e >= Ne || g < 0 || g >= Ng || fr < 0 || fr >= Fr) return;      // workgroup-uniform
    const size_t hw = (size_t)H * W;
    vsd_tile<VEC>(depth_obs + (size_t)fr * hw, cams + 4 * fr, H, W, z_est + (size_t)e * hw, z_gt + (size_t)g * hw, diameter, delta,
                  taus, T, counts + p * (T + 2));
}

__global__ __launch_bounds__(256) void bop_vsd_finalize_kernel(const int32_t* __restrict__ counts, int N, int T,
                                                               double* __restrict__ errors) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)N * T) return;
    const int n = (int)(i / T), k = (int)(i - (size_t)n * T);
    const int32_t* r = counts + (size_t)n * (T + 2);
    const int nU = r[0], nI = r[1];
    errors[i] = nU == 0 ? 1.0 : (double)(r[2 + k] + (nU - nI)) / (double)nU;
}

__global__ __launch_bounds__(256) void bop_inf_kernel(unsigned long long* __restrict__ a, unsigned long long* __restrict__ b,
                                                      int N) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) a[i] = DINF, b[i] = DINF;
}

__global__ __launch_bounds__(256) void bop_mssd_mspd_kernel(const float* __restrict__ vertices, int V,
                                                            const double* __restrict__ syms, int S,
                                                            const double* __restrict__ pose_est,
                                                            const double* __restrict__ pose_gt,
                                                            const float* __restrict__ cams, FrameIdx frames,
                                                            unsigned long long* __restrict__ mssd,
                                                            unsigned long long* __restrict__ mspd) {
    const int n = blockIdx.y, s0 = blockIdx.x * SC, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    __shared__ double Gs[SC][12];
    __shared__ double red[4][2 * SC];
    const double* Pg = pose_gt + 16 * (size_t)n;
    if (threadIdx.x < SC) {
        // slots past the end hold the last transform and are never compared (live below)
        bop_compose(Pg, syms + 16 * (size_t)min(s0 + (int)threadIdx.x, S - 1), Gs[threadIdx.x]);
    }
    __syncthreads();
    double G[SC][12], E[12];
#pragma unroll
    for (int s = 0; s < SC; ++s)
#pragma unroll
        for (int j = 0; j < 12; ++j) G[s][j] = Gs[s][j];
#pragma unroll
    for (int j = 0; j < 12; ++j) E[j] = pose_est[16 * (size_t)n + j];
    const int fr = frames.f[n];
    const double fx = (double)cams[4 * fr], fy = (double)cams[4 * fr + 1], cx = (double)cams[4 * fr + 2],
                 cy = (double)cams[4 * fr + 3];
    const int live = min(SC, S - s0);                // transforms of this chunk that exist
    double m3[SC], m2[SC];
#pragma unroll
    for (int s = 0; s < SC; ++s) m3[s] = 0.0, m2[s] = 0.0;
    for (int v = threadIdx.x; v < V; v += 256) {
        const double x = (double)vertices[3 * (size_t)v], y = (double)vertices[3 * (size_t)v + 1],
                     z = (double)vertices[3 * (size_t)v + 2];
        double Xe, Ye, Ze;
        bop_transform(E, x, y, z, Xe, Ye, Ze);
        const double ue = (Xe / Ze) * fx + cx, ve = (Ye / Ze) * fy + cy;
        const bool oke = Ze > 0.0 && fin(Xe) && fin(Ye) && fin(Ze) && fin(ue) && fin(ve);
#pragma unroll
        for (int s = 0; s < SC; ++s) {
            if (s >= live) break;                    // workgroup-uniform: S = 1 pays for one transform, not SC
            double Xg, Yg, Zg;
            bop_transform(G[s], x, y, z, Xg, Yg, Zg);
            const double q = bop_sqdist(Xe, Ye, Ze, Xg, Yg, Zg);   // NaN counts as +inf
            m3[s] = q > m3[s] ? q : m3[s];
            const double ug = (Xg / Zg) * fx + cx, vg = (Yg / Zg) * fy + cy;
            const bool ok = oke && Zg > 0.0 && fin(Xg) && fin(Yg) && fin(Zg) && fin(ug) && fin(vg);
            const double du = ue - ug, dv = ve - vg;
            const double p = ok ? du * du + dv * dv : (double)INFINITY;
            m2[s] = p > m2[s] ? p : m2[s];
        }
    }
#pragma unroll
    for (int s = 0; s < SC; ++s) {
        const double a = wave_max_f64(m3[s]), b = wave_max_f64(m2[s]);
        if (lane == 0) red[wv][s] = a, red[wv][SC + s] = b;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        const int off = threadIdx.x * SC;            // 0: MSSD, 1: MSPD
        double best = INFINITY;
        for (int s = 0; s < live; ++s) {
            double m = red[0][off + s];
            for (int w = 1; w < 4; ++w) m = red[w][off + s] > m ? red[w][off + s] : m;
            best = m < best ? m : best;
        }
        // sqrt is monotone and correctly rounded: the root of the min-max of the squares is the min-max of the roots
        atomicMin((threadIdx.x == 0 ? mssd : mspd) + n, (unsigned long long)__double_as_longlong(sqrt(best)));
    }
}

constexpr int MATCH_COLS = 10;        // threshold columns j of 8.12
constexpr int PAIR_ROWS = 32768;      // pair rows per launch of the pair kernel (grid.y)

// 8.12 outputs before the greedy pass: every estimate unmatched, no true positive.
__global__ __launch_bounds__(256) void bop_match_clear_kernel(int32_t* __restrict__ match, size_t n_match,
                                                              int32_t* __restrict__ tp, int n_tp) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n_match) match[i] = -1;
    if (i < (size_t)n_tp) tp[i] = 0;
}

// 8.12. One wave per (group, 64 columns); a lane owns column c = (k, j) of its group and walks the group's estimates in
// rank order with the matched instances as a 64-bit mask in registers. The lanes of a wave read the same [E][G] block of
// errors, ten neighbouring lanes the same double. A group row that does not fit the tables is skipped whole (its estimates
// stay unmatched). Matches whose instance is valid are counted per lane and leave as one integer atomicAdd per column.
__global__ __launch_bounds__(64) void bop_match_kernel(const double* __restrict__ err, int Ptot,
                                                       const int32_t* __restrict__ groups, const uint8_t* __restrict__ valid,
                                                       int Itot, const double* __restrict__ thr, int K, int Etot,
                                                       int32_t* __restrict__ match, int32_t* __restrict__ tp) {
    const size_t gr = blockIdx.x;
    const int c = blockIdx.y * 64 + threadIdx.x, C = K * MATCH_COLS;
    const int32_t* row = groups + 5 * gr;
    const int p0 = row[0], e0 = row[1], i0 = row[2], E = row[3], G = row[4];
    if (E < 0 || E > OSSID_BOP_MAX_INSTANCES || G < 1 || G > OSSID_BOP_MAX_INSTANCES || p0 < 0 || e0 < 0 || i0 < 0 ||
        (long long)p0 + (long long)E * G > Ptot || (long long)e0 + E > Etot || (long long)i0 + G > Itot)
        return;                                      // wave-uniform
    if (c >= C) return;
    const int k = c / MATCH_COLS;
    const double th = thr[gr * C + c];
    const double* er = err + (size_t)p0 * K + k;
    unsigned long long taken = 0ull;
    int hits = 0;
    for (int e = 0; e < E; ++e) {
        int best = -1;
        double best_err = 0.0;
        for (int g = 0; g < G; ++g) {
            const double v = er[((size_t)e * G + g) * K];
            // strict <: a NaN is never below; ties keep the lower g
            if (!((taken >> g) & 1ull) && v < th && (best < 0 || v < best_err)) best = g, best_err = v;
        }
        if (best >= 0) {
            taken |= 1ull << best;
            hits += valid[i0 + best] != 0;
        }
        match[((size_t)e0 + e) * C + c] = best;
    }
    if (hits) atomicAdd(tp + c, hits);
}

bool frames_ok(const int32_t* frame_host, int N, int Fr) {
    for (int i = 0; i < N; ++i)
        if (frame_host[i] < 0 || frame_host[i] >= Fr) return false;
    return true;
}

}  // namespace

extern "C" {

int ossid_bop_vsd(const float* depth_obs, const float* cams, int Fr, int H, int W, const float* z_est, const float* z_gt,
                  const int32_t* frame_host, int N, double diameter, double delta, const double* taus_host, int T,
                  int32_t* counts, double* errors, void* stream) {
    if (!depth_obs || !cams || !z_est || !z_gt || !frame_host || !taus_host || !counts || !errors || Fr < 1 || N < 1 || H <= 0 ||
        W <= 0 || (long long)H * W > OSSID_RASTER_MAX_PIXELS || T < 1 || T > OSSID_BOP_MAX_TAUS || !(diameter > 0.0) ||
        !std::isfinite(diameter) || !(delta >= 0.0) || !std::isfinite(delta) || !frames_ok(frame_host, N, Fr))
        return OSSID_EINVAL;
    Taus taus = {};
    for (int k = 0; k < T; ++k) {
        if (!std::isfinite(taus_host[k])) return OSSID_EINVAL;
        taus.t[k] = taus_host[k];
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)H * W, ncount = (size_t)N * (T + 2);
    const bool vec = hw % 4 == 0 && (((uintptr_t)depth_obs | (uintptr_t)z_est | (uintptr_t)z_gt) & 15) == 0;
    hipLaunchKernelGGL(bop_zero_kernel, dim3((unsigned)((ncount + 255) / 256 < 1024 ? (ncount + 255) / 256 : 1024)), dim3(256), 0, s,
                       counts, ncount);
    const unsigned tiles = (unsigned)((hw + TILE - 1) / TILE);
    for (int a = 0; a < N; a += CHUNK) {
        const int nb = N - a < CHUNK ? N - a : CHUNK;
        FrameIdx fi = {};
        for (int i = 0; i < nb; ++i) fi.f[i] = frame_host[a + i];
        if (vec)
            hipLaunchKernelGGL(bop_vsd_kernel<true>, dim3(tiles, nb), dim3(256), 0, s, depth_obs, cams, H, W, z_est + (size_t)a * hw,
                               z_gt + (size_t)a * hw, fi, diameter, delta, taus, T, counts + (size_t)a * (T + 2));
        else
            hipLaunchKernelGGL(bop_vsd_kernel<false>, dim3(tiles, nb), dim3(256), 0, s, depth_obs, cams, H, W, z_est + (size_t)a * hw,
                               z_gt + (size_t)a * hw, fi, diameter, delta, taus, T, counts + (size_t)a * (T + 2));
    }
    hipLaunchKernelGGL(bop_vsd_finalize_kernel, dim3((unsigned)(((size_t)N * T + 255) / 256)), dim3(256), 0, s, counts, N, T, errors);
    return ossid_launch_status();
}

int ossid_bop_vsd_pairs(const float* depth_obs, const float* cams, int Fr, int H, int W, const float* z_est, int Ne,
                        const float* z_gt, int Ng, const int32_t* pairs, int P, double diameter, double delta,
                        const double* taus_host, int T, int32_t* counts, double* errors, void* stream) {
    if (!depth_obs || !cams || !z_est || !z_gt || !pairs || !taus_host || !counts || !errors || Fr < 1 || Ne < 1 || Ng < 1 ||
        P < 1 || H <= 0 || W <= 0 || (long long)H * W > OSSID_RASTER_MAX_PIXELS || T < 1 || T > OSSID_BOP_MAX_TAUS ||
        !(diameter > 0.0) || !std::isfinite(diameter) || !(delta >= 0.0) || !std::isfinite(delta))
        return OSSID_EINVAL;
    Taus taus = {};
    for (int k = 0; k < T; ++k) {
        if (!std::isfinite(taus_host[k])) return OSSID_EINVAL;
        taus.t[k] = taus_host[k];
    }
    hipStream_t s = (hipStream_t)stream;
    const size_t hw = (size_t)H * W, ncount = (size_t)P * (T + 2);
    const bool vec = hw % 4 == 0 && (((uintptr_t)depth_obs | (uintptr_t)z_est | (uintptr_t)z_gt) & 15) == 0;
    hipLaunchKernelGGL(bop_zero_kernel, dim3((unsigned)((ncount + 255) / 256 < 1024 ? (ncount + 255) / 256 : 1024)), dim3(256), 0, s,
                       counts, ncount);
    const unsigned tiles = (unsigned)((hw + TILE - 1) / TILE);
    for (int a = 0; a < P; a += PAIR_ROWS) {
        const int nb = P - a < PAIR_ROWS ? P - a : PAIR_ROWS;
        if (vec)
            hipLaunchKernelGGL(bop_vsd_pairs_kernel<true>, dim3(tiles, nb), dim3(256), 0, s, depth_obs, cams, Fr, H, W, z_est, Ne,
                               z_gt, Ng, pairs + 3 * (size_t)a, diameter, delta, taus, T, counts + (size_t)a * (T + 2));
        else
            hipLaunchKernelGGL(bop_vsd_pairs_kernel<false>, dim3(tiles, nb), dim3(256), 0, s, depth_obs, cams, Fr, H, W, z_est, Ne,
                               z_gt, Ng, pairs + 3 * (size_t)a, diameter, delta, taus, T, counts + (size_t)a * (T + 2));
    }
    hipLaunchKernelGGL(bop_vsd_finalize_kernel, dim3((unsigned)(((size_t)P * T + 255) / 256)), dim3(256), 0, s, counts, P, T, errors);
    return ossid_launch_status();
}

int ossid_bop_match(const double* err, int Ptot, const int32_t* groups, int Gr, const uint8_t* valid, int Itot,
                    const double* thr, int T, int32_t* match, int Etot, int32_t* tp, void* stream) {
    if (!groups || !valid || !thr || !tp || Gr < 1 || Itot < 1 || Ptot < 0 || Etot < 0 || (Ptot > 0 && !err) ||
        (Etot > 0 && !match) || T < 1 || T > OSSID_BOP_MAX_TAUS)
        return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int K = T + 2, C = K * MATCH_COLS;
    const size_t n_match = (size_t)Etot * C, n_clear = n_match > (size_t)C ? n_match : (size_t)C;
    hipLaunchKernelGGL(bop_match_clear_kernel, dim3((unsigned)((n_clear + 255) / 256)), dim3(256), 0, s, match, n_match, tp, C);
    hipLaunchKernelGGL(bop_match_kernel, dim3((unsigned)Gr, (unsigned)((C + 63) / 64)), dim3(64), 0, s, err, Ptot, groups, valid,
                       Itot, thr, K, Etot, match, tp);
    return ossid_launch_status();
}

int ossid_bop_mssd_mspd(const float* vertices, int V, const double* symmetries, int S, const double* pose_est,
                        const double* pose_gt, const float* cams, int Fr, const int32_t* frame_host, int N, double* mssd,
                        double* mspd, void* stream) {
    if (!vertices || !symmetries || !pose_est || !pose_gt || !cams || !frame_host || !mssd || !mspd || V < 1 ||
        V > OSSID_RASTER_MAX_VERTICES || S < 1 || S > OSSID_BOP_MAX_SYMMETRIES || Fr < 1 || N < 1 || !frames_ok(frame_host, N, Fr))
        return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bop_inf_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, (unsigned long long*)mssd,
                       (unsigned long long*)mspd, N);
    for (int a = 0; a < N; a += CHUNK) {
        const int nb = N - a < CHUNK ? N - a : CHUNK;
        FrameIdx fi = {};
        for (int i = 0; i < nb; ++i) fi.f[i] = frame_host[a + i];
        hipLaunchKernelGGL(bop_mssd_mspd_kernel, dim3((unsigned)((S + SC - 1) / SC), nb), dim3(256), 0, s, vertices, V, symmetries, S,
                           pose_est + 16 * (size_t)a, pose_gt + 16 * (size_t)a, cams, fi, (unsigned long long*)mssd + a,
                           (unsigned long long*)mspd + a);
    }
    return ossid_launch_status();
}

}  // extern "C"
