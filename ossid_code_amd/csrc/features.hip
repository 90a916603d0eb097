// Keypoint-feature pose hypotheses as SPEC.md section 11 defines them, in place of zephyr's SIFT featurization
// (scripts/online_learning.py:52-76 builds the models, :427-437 featurizes the frame and matches).
//
//   pyramid      grey (integer luma, 6 fractional bits), then binomial 5x5 passes, one thread per pixel, all int32: exact.
//                Octave o: levels after 1, 2, 4, 8, 16 cumulative passes; octave o + 1 starts from L_2[::2, ::2].
//   detect       one thread per (octave, level, pixel): strict 26-neighbour extremum of the difference of levels, contrast,
//                edge test in int64, mask && depth > 0 -> a flag; per-block counts, one workgroup scans them, an ordered
//                compaction (ascending (o, s, y, x), never arrival order).
//   describe     one wave per keypoint: 36-bin orientation histogram (integer LDS atomics: order-free), 16 x 16 rotated
//                samples soft-binned into 4 x 4 x 8 integer bins in LDS, integer normalisation, the f64 frame by lane 0.
//   match        i8 matrix cores (v_mfma_i32_32x32x32_i8): scene features on the columns (lanes), model features on the
//                rows (registers and lane half), d2 = |a|^2 + |b|^2 - 2 a.b; each lane keeps its running minimum, the lane
//                halves merge once, workgroups over model chunks merge by a 64-bit atomicMin on (d2 << 32) | j.
//   hypotheses   T = F_s . F_m^-1 in f64 and the (j, 0, w) peaks that ossid_ppf_cluster (SPEC 6.6) takes.
// No transcendental function runs on the device: angles are decided by sign tests against host tables.
#include <float.h>
#include <math.h>

#include "mfma.h"
#include "workgroup.h"

namespace {

constexpr int MAX_OCT = OSSID_FEAT_MAX_OCTAVES;
constexpr int NLEV = 5;
constexpr int MIN_SIDE = 8;
constexpr int DNT = 256;                     // detect workgroup
constexpr int EDGE_R = 10;

struct Pyr {
    int n_oct;
    int H[MAX_OCT], W[MAX_OCT];
    long long off[MAX_OCT];                  // int32 offset of the octave's level 0; level l follows at l * H * W
    long long tmp;                           // two scratch planes of H[0] * W[0]
    long long words;
    long long flat[MAX_OCT + 1];             // detect's flat index space: octave o owns [flat[o], flat[o + 1]) = 2 H W
};

bool make_pyr(int H, int W, int octaves, Pyr* p) {
    if (H < MIN_SIDE || W < MIN_SIDE || H > 65535 || (long long)H * W > OSSID_RASTER_MAX_PIXELS || octaves < 1 || octaves > MAX_OCT)
        return false;
    p->n_oct = 0;
    long long off = 0, flat = 0;
    int h = H, w = W;
    for (int o = 0; o < MAX_OCT; ++o) p->H[o] = p->W[o] = 0, p->off[o] = 0;
    for (int o = 0; o < octaves; ++o) {
        if (o > 0) {
            h = (h + 1) / 2, w = (w + 1) / 2;
            if (h < MIN_SIDE || w < MIN_SIDE) break;
        }
        p->H[o] = h, p->W[o] = w, p->off[o] = off, p->flat[o] = flat;
        off += (long long)NLEV * h * w;
        flat += 2ll * h * w;
        p->n_oct = o + 1;
    }
    for (int o = p->n_oct; o <= MAX_OCT; ++o) p->flat[o] = flat;
    p->tmp = off;
    p->words = off + 2ll * H * W;
    return true;
}

struct FeatTables {
    int ow1[7 * 7], ow2[10 * 10];            // orientation weights by (|dy|, |dx|) for s = 1, 2
    float gw[8 * 8];                         // descriptor window by (|i - 7.5| - .5, |j - 7.5| - .5)
    float sec_c[17], sec_s[17];              // cos / sin(k 10 deg), k = 1 .. 17
    float ori_c[36], ori_s[36];              // cos / sin((b + .5) 10 deg)
    float hsp[2];                            // f32(0.75 sigma_s)
    float r8;                                // f32(sqrt(1/2))
};

// cos / sin of (k + offset) 90 / 9 degrees, k = 0 .. 35: the first quadrant's cosines computed in f64, everything else by
// symmetry (sin a = cos(90 - a); a quarter turn maps (c, s) to (-s, c)), so that a 90-degree image rotation shifts bins by 9
void quadrant_table(bool half, float* c, float* s) {
    float q[10];
    if (!half) {
        for (int k = 0; k <= 9; ++k) q[k] = (float)cos((double)k * 10.0 * M_PI / 180.0);
        q[0] = 1.0f, q[9] = 0.0f;
        for (int k = 0; k < 9; ++k) c[k] = q[k], s[k] = q[9 - k];
    } else {
        for (int k = 0; k < 9; ++k) q[k] = (float)cos(((double)k + 0.5) * 10.0 * M_PI / 180.0);
        for (int k = 0; k < 9; ++k) c[k] = q[k], s[k] = q[8 - k];
    }
    for (int k = 9; k < 36; ++k) c[k] = -s[k - 9], s[k] = c[k - 9];
}

FeatTables make_tables() {
    FeatTables t;
    const double sigma[2] = {sqrt(2.0), 2.0};
    for (int s = 0; s < 2; ++s) {
        const int n = s == 0 ? 7 : 10;
        int* ow = s == 0 ? t.ow1 : t.ow2;
        const double sg = 1.5 * sigma[s];
        for (int dy = 0; dy < n; ++dy)
            for (int dx = 0; dx < n; ++dx)
                ow[dy * n + dx] = (int)rint(1024.0 * exp(-((double)(dx * dx) + (double)(dy * dy)) / (2.0 * sg * sg)));
        t.hsp[s] = (float)(0.75 * sigma[s]);
    }
    for (int i = 0; i < 8; ++i)
        for (int j = 0; j < 8; ++j) {
            const double a = i + 0.5, b = j + 0.5;
            t.gw[i * 8 + j] = (float)exp(-(a * a + b * b) / 128.0);
        }
    float c[36], s[36];
    quadrant_table(false, c, s);
    for (int k = 1; k <= 17; ++k) t.sec_c[k - 1] = c[k], t.sec_s[k - 1] = s[k];
    quadrant_table(true, t.ori_c, t.ori_s);
    t.r8 = (float)sqrt(0.5);
    return t;
}

// ---- pyramid ------------------------------------------------------------------------------------------------------------
__global__ void feat_grey_kernel(const uint8_t* __restrict__ img, long long n, int32_t* __restrict__ out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = img[3 * i], g = img[3 * i + 1], b = img[3 * i + 2];
    out[i] = ((77 * r + 150 * g + 29 * b + 128) >> 8) << 6;
}

__device__ __forceinline__ int reflect101(int i, int n) {
    if (i < 0) i = -i;
    if (i >= n) i = 2 * n - 2 - i;
    return i;
}

__global__ void feat_pass_kernel(const int32_t* __restrict__ in, int H, int W, int32_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    const int k[5] = {1, 4, 6, 4, 1};
    int acc = 0;
#pragma unroll
    for (int i = 0; i < 5; ++i) {
        const int32_t* row = in + (size_t)reflect101(y + i - 2, H) * W;
        int r = 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) r += k[j] * row[reflect101(x + j - 2, W)];
        acc += k[i] * r;
    }
    out[(size_t)y * W + x] = (acc + 128) >> 8;
}

__global__ void feat_down_kernel(const int32_t* __restrict__ in, int Wi, int H, int W, int32_t* __restrict__ out) {
    const int x = blockIdx.x * blockDim.x + threadIdx.x, y = blockIdx.y;
    if (x >= W) return;
    out[(size_t)y * W + x] = in[(size_t)(2 * y) * Wi + 2 * x];
}

// ---- detect -------------------------------------------------------------------------------------------------------------
__device__ bool is_keypoint(const Pyr& P, const int32_t* __restrict__ pyr, long long f, const float* __restrict__ depth,
                            const uint8_t* __restrict__ mask, int contrast) {
    int o = 0;
    while (o + 1 < P.n_oct && f >= P.flat[o + 1]) ++o;
    const int H = P.H[o], W = P.W[o];
    const long long plane = (long long)H * W;
    long long r = f - P.flat[o];
    const int s = 1 + (int)(r / plane);
    r -= (long long)(s - 1) * plane;
    const int y = (int)(r / W), x = (int)(r - (long long)y * W);
    if (y < 1 || x < 1 || y > H - 2 || x > W - 2) return false;
    const int32_t* L = pyr + P.off[o];
    const size_t c = (size_t)y * W + x;
    const int d = L[(s + 1) * plane + c] - L[s * plane + c];
    if ((d < 0 ? -d : d) < contrast) return false;
    bool gt = true, lt = true;
    for (int ds = -1; ds <= 1; ++ds) {
        const int32_t* A = L + (s + ds) * plane;
        const int32_t* B = A + plane;
        for (int dy = -1; dy <= 1; ++dy)
            for (int dx = -1; dx <= 1; ++dx) {
                if (ds == 0 && dy == 0 && dx == 0) continue;
                const size_t q = (size_t)(y + dy) * W + (x + dx);
                const int v = B[q] - A[q];
                gt = gt && d > v;
                lt = lt && d < v;
            }
        if (!gt && !lt) return false;
    }
    const int32_t* A = L + s * plane;
    const int32_t* B = A + plane;
#define FEAT_D(yy, xx) ((long long)(B[(size_t)(yy) * W + (xx)] - A[(size_t)(yy) * W + (xx)]))
    const long long dxx = FEAT_D(y, x + 1) + FEAT_D(y, x - 1) - 2 * (long long)d;
    const long long dyy = FEAT_D(y + 1, x) + FEAT_D(y - 1, x) - 2 * (long long)d;
    const long long dxy4 = FEAT_D(y + 1, x + 1) + FEAT_D(y - 1, x - 1) - FEAT_D(y + 1, x - 1) - FEAT_D(y - 1, x + 1);
#undef FEAT_D
    const long long tr = dxx + dyy, det4 = 4 * dxx * dyy - dxy4 * dxy4;
    if (!(det4 > 0) || !(4 * EDGE_R * tr * tr < (long long)(EDGE_R + 1) * (EDGE_R + 1) * det4)) return false;
    const size_t full = (size_t)(y << o) * P.W[0] + (x << o);
    return mask[full] != 0 && depth[full] > 0.0f;
}

// workgroup-wide rank of the flagged threads (DNT = 4 waves) -> this thread's rank, *total = the workgroup's count
__device__ int block_rank(bool flag, int* total) {
    __shared__ int wsum[DNT / 64];
    const unsigned long long b = __ballot(flag);
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rank = __popcll(b & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[wave] = __popcll(b);
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < DNT / 64; ++w) {
        if (w < wave) before += wsum[w];
        all += wsum[w];
    }
    *total = all;
    return before + rank;
}

__global__ __launch_bounds__(DNT) void feat_flag_kernel(Pyr P, const int32_t* __restrict__ pyr, const float* __restrict__ depth,
                                                        const uint8_t* __restrict__ mask, int contrast,
                                                        uint8_t* __restrict__ flags, int32_t* __restrict__ bcount) {
    const long long f = (long long)blockIdx.x * DNT + threadIdx.x;
    const bool k = f < P.flat[MAX_OCT] && is_keypoint(P, pyr, f, depth, mask, contrast);
    if (f < P.flat[MAX_OCT]) flags[f] = k ? 1 : 0;
    int total;
    block_rank(k, &total);
    if (threadIdx.x == 0) bcount[blockIdx.x] = total;
}

// exclusive scan of the block counts in place, count[0] = the total, count[1] = 1 iff it is over the cap
__global__ __launch_bounds__(1024) void feat_scan_kernel(int32_t* __restrict__ bcount, int nb, int cap, int32_t* __restrict__ count) {
    __shared__ int lds[16];
    const int total = wg_scan_range<16>(bcount, nb, lds, [&](int i, int run) { bcount[i] = run; });
    if (threadIdx.x == 0) count[0] = total, count[1] = total > cap ? 1 : 0;
}

__global__ __launch_bounds__(DNT) void feat_compact_kernel(Pyr P, const uint8_t* __restrict__ flags,
                                                           const int32_t* __restrict__ boffset, int cap,
                                                           int32_t* __restrict__ kps) {
    const long long f = (long long)blockIdx.x * DNT + threadIdx.x;
    const bool k = f < P.flat[MAX_OCT] && flags[f] != 0;
    int total;
    const int rank = boffset[blockIdx.x] + block_rank(k, &total);
    if (!k || rank >= cap) return;
    int o = 0;
    while (o + 1 < P.n_oct && f >= P.flat[o + 1]) ++o;
    const long long plane = (long long)P.H[o] * P.W[o];
    long long r = f - P.flat[o];
    const int s = 1 + (int)(r / plane);
    r -= (long long)(s - 1) * plane;
    const int y = (int)(r / P.W[o]);
    kps[4 * rank + 0] = o, kps[4 * rank + 1] = s, kps[4 * rank + 2] = y, kps[4 * rank + 3] = (int)(r - (long long)y * P.W[o]);
}

// ---- describe -----------------------------------------------------------------------------------------------------------
// 6.4's sign-test rule: the sector of (u, v) among 2 * (NB + 1) sectors whose upper-half boundaries are (cs[k], sn[k])
template <int NB>
__device__ __forceinline__ int sector(float u, float v, const float* cs, const float* sn) {
    const bool lower = v < 0.0f || (v == 0.0f && u < 0.0f);
    if (lower) u = -u, v = -v;
    int b = 0;
#pragma unroll
    for (int k = 0; k < NB; ++k) b += ((cs[k] * v) - (sn[k] * u)) >= 0.0f ? 1 : 0;
    return b + (lower ? NB + 1 : 0);
}

struct DescShared {
    int hist[36];
    int acc[128];
    int drop, bin;
    long long cap;
    double root;
};

__device__ __forceinline__ double dot3d(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

// SPEC 11.5 by one thread -> false when the keypoint is dropped
__device__ bool feat_frame(const float* __restrict__ depth, int H, int W, float fx, float fy, float cx, float cy, int o, int s,
                           int y, int x, float c, float sn, double* F) {
    const int xf = x << o, yf = y << o, r = (s == 1 ? 4 : 6) << o;
    if (xf - r < 0 || yf - r < 0 || xf + r > W - 1 || yf + r > H - 1) return false;
    const float Z = depth[(size_t)yf * W + xf];
    const int nx[4] = {xf + r, xf - r, xf, xf}, ny[4] = {yf, yf, yf + r, yf - r};
    double Q[4][3];
    const float tol = 0.05f * Z;
    for (int k = 0; k < 4; ++k) {
        const float zn = depth[(size_t)ny[k] * W + nx[k]];
        if (!(zn > 0.0f) || !(fabsf(zn - Z) <= tol)) return false;
        Q[k][0] = (double)(((float)nx[k] - cx) * zn / fx), Q[k][1] = (double)(((float)ny[k] - cy) * zn / fy), Q[k][2] = (double)zn;
    }
    const double P[3] = {(double)(((float)xf - cx) * Z / fx), (double)(((float)yf - cy) * Z / fy), (double)Z};
    const double a[3] = {Q[0][0] - Q[1][0], Q[0][1] - Q[1][1], Q[0][2] - Q[1][2]};
    const double b[3] = {Q[2][0] - Q[3][0], Q[2][1] - Q[3][1], Q[2][2] - Q[3][2]};
    double n[3] = {a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]};
    double l2 = dot3d(n, n);
    if (!(l2 > 0.0)) return false;
    double l = sqrt(l2);
    for (int k = 0; k < 3; ++k) n[k] = n[k] / l;
    if (dot3d(n, P) > 0.0)
        for (int k = 0; k < 3; ++k) n[k] = -n[k];
    const double ray[3] = {(((double)xf + (double)c) - (double)cx) / (double)fx, (((double)yf + (double)sn) - (double)cy) / (double)fy, 1.0};
    const double den = dot3d(n, ray);
    if (fabs(den) < 1e-6) return false;
    const double nP = dot3d(n, P);
    double e1[3];
    for (int k = 0; k < 3; ++k) e1[k] = (ray[k] * nP) / den - P[k];
    const double along = dot3d(n, e1);
    for (int k = 0; k < 3; ++k) e1[k] = e1[k] - n[k] * along;
    l2 = dot3d(e1, e1);
    if (!(l2 > 0.0)) return false;
    l = sqrt(l2);
    for (int k = 0; k < 3; ++k) e1[k] = e1[k] / l;
    const double e2[3] = {n[1] * e1[2] - n[2] * e1[1], n[2] * e1[0] - n[0] * e1[2], n[0] * e1[1] - n[1] * e1[0]};
    for (int k = 0; k < 3; ++k) F[4 * k + 0] = e1[k], F[4 * k + 1] = e2[k], F[4 * k + 2] = n[k], F[4 * k + 3] = P[k];
    F[12] = 0.0, F[13] = 0.0, F[14] = 0.0, F[15] = 1.0;
    return true;
}

__global__ __launch_bounds__(64) void feat_describe_kernel(Pyr P, FeatTables T, const int32_t* __restrict__ pyr,
                                                           const float* __restrict__ depth, float fx, float fy, float cx,
                                                           float cy, const int32_t* __restrict__ kps,
                                                           const int32_t* __restrict__ count, int cap,
                                                           int32_t* __restrict__ bins, uint8_t* __restrict__ desc,
                                                           double* __restrict__ frames, uint8_t* __restrict__ ok) {
    __shared__ DescShared sh;
    const int kp = blockIdx.x, lane = threadIdx.x;
    if (kp >= count_or_0(count, cap)) return;
    const int o = kps[4 * kp], s = kps[4 * kp + 1], y = kps[4 * kp + 2], x = kps[4 * kp + 3];
    const int H = P.H[o], W = P.W[o];
    const int32_t* L = pyr + P.off[o] + (long long)s * H * W;
    const int rho = s == 1 ? 6 : 9;
    // rows of a dropped keypoint are zero
    desc[(size_t)kp * 128 + lane] = 0, desc[(size_t)kp * 128 + 64 + lane] = 0;
    if (lane == 0) {
        for (int q = 0; q < 16; ++q) frames[(size_t)kp * 16 + q] = 0.0;
        ok[kp] = 0;
    }
    if (x - rho - 1 < 0 || y - rho - 1 < 0 || x + rho + 1 > W - 1 || y + rho + 1 > H - 1) {
        if (lane == 0) bins[kp] = -1;
        return;
    }
    if (lane < 36) sh.hist[lane] = 0;
    sh.acc[lane] = 0, sh.acc[64 + lane] = 0;
    if (lane == 0) sh.drop = 0;
    __syncthreads();
    // 11.3
    const int side = 2 * rho + 1, nw = s == 1 ? 7 : 10;
    const int* ow = s == 1 ? T.ow1 : T.ow2;
    for (int q = lane; q < side * side; q += 64) {
        const int dy = q / side - rho, dx = q % side - rho;
        const int32_t* p = L + (size_t)(y + dy) * W + (x + dx);
        const int gx = p[1] - p[-1], gy = p[W] - p[-W];
        const int m = (int)sqrtf((float)(gx * gx + gy * gy));
        const int w = ow[(dy < 0 ? -dy : dy) * nw + (dx < 0 ? -dx : dx)];
        const int add = (int)(((long long)m * w) >> 10);
        if (add != 0) atomicAdd(&sh.hist[sector<17>((float)gx, (float)gy, T.sec_c, T.sec_s)], add);
    }
    __syncthreads();
    if (lane == 0) {
        int best = 0;
        long long bv = -1;
        for (int b = 0; b < 36; ++b) {
            const long long v = (long long)sh.hist[(b + 35) % 36] + 2ll * sh.hist[b] + (long long)sh.hist[(b + 1) % 36];
            if (v > bv) bv = v, best = b;
        }
        sh.bin = best;
        bins[kp] = best;
    }
    __syncthreads();
    const int bin = sh.bin;
    const float c = T.ori_c[bin], sn = T.ori_s[bin];
    // 11.4
    const float hsp = T.hsp[s - 1], xf = (float)x, yf = (float)y;
    int sx0[4], sy0[4];
    float sax[4], say[4];
    bool out = false;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = lane + 64 * t, i = q >> 4, j = q & 15;
        const float u = ((float)j - 7.5f) * hsp, v = ((float)i - 7.5f) * hsp;
        const float px = xf + ((c * u) - (sn * v)), py = yf + ((sn * u) + (c * v));
        const float fx0 = floorf(px), fy0 = floorf(py);
        sx0[t] = (int)fx0, sy0[t] = (int)fy0, sax[t] = px - fx0, say[t] = py - fy0;
        out = out || sx0[t] - 1 < 0 || sy0[t] - 1 < 0 || sx0[t] + 2 > W - 1 || sy0[t] + 2 > H - 1;
    }
    if (out) sh.drop = 1;
    __syncthreads();
    if (sh.drop) return;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int q = lane + 64 * t, i = q >> 4, j = q & 15;
        const int32_t* p = L + (size_t)sy0[t] * W + sx0[t];
        const float ax = sax[t], ay = say[t];
        const float gx00 = (float)(p[1] - p[-1]), gx01 = (float)(p[2] - p[0]);
        const float gx10 = (float)(p[W + 1] - p[W - 1]), gx11 = (float)(p[W + 2] - p[W]);
        const float gy00 = (float)(p[W] - p[-W]), gy01 = (float)(p[W + 1] - p[1 - W]);
        const float gy10 = (float)(p[2 * W] - p[0]), gy11 = (float)(p[2 * W + 1] - p[1]);
        const float bx = ((gx00 * (1.0f - ax) + gx01 * ax) * (1.0f - ay)) + ((gx10 * (1.0f - ax) + gx11 * ax) * ay);
        const float by = ((gy00 * (1.0f - ax) + gy01 * ax) * (1.0f - ay)) + ((gy10 * (1.0f - ax) + gy11 * ax) * ay);
        const float gu = (c * bx) + (sn * by), gv = (c * by) - (sn * bx);
        const float r8 = T.r8;
        const float dc[3] = {r8, 0.0f, -r8}, ds[3] = {r8, 1.0f, r8};
        const int k = sector<3>(gu, gv, dc, ds), k1 = (k + 1) & 7;
        const float dirx[8] = {1.0f, r8, 0.0f, -r8, -1.0f, -r8, 0.0f, r8}, diry[8] = {0.0f, r8, 1.0f, r8, 0.0f, -r8, -1.0f, -r8};
        const float a = ((gu * diry[k1]) - (gv * dirx[k1])) / r8;
        const float b = ((dirx[k] * gv) - (diry[k] * gu)) / r8;
        const float gw = T.gw[(i < 8 ? 7 - i : i - 8) * 8 + (j < 8 ? 7 - j : j - 8)];
        // cell coordinate (i - 1.5) / 4: floor and fraction from the integer 2 i - 3 (eighths), exact
        const int ey = 2 * i - 3 + 8, ex = 2 * j - 3 + 8;             // +8: keep the dividend positive
        const int cy0 = (ey >> 3) - 1, cx0 = (ex >> 3) - 1;
        const float fyc = (float)(ey & 7) * 0.125f, fxc = (float)(ex & 7) * 0.125f;
#pragma unroll
        for (int yy = 0; yy < 2; ++yy) {
            const int cyy = cy0 + yy;
            if (cyy < 0 || cyy > 3) continue;
            const float wy = yy ? fyc : 1.0f - fyc;
#pragma unroll
            for (int xx = 0; xx < 2; ++xx) {
                const int cxx = cx0 + xx;
                if (cxx < 0 || cxx > 3) continue;
                const float wx = xx ? fxc : 1.0f - fxc;
                const int va = (int)rintf(((a * wy) * wx) * gw), vb = (int)rintf(((b * wy) * wx) * gw);
                int* cell = &sh.acc[(cyy * 4 + cxx) * 8];
                if (va != 0) atomicAdd(&cell[k], va);
                if (vb != 0) atomicAdd(&cell[k1], vb);
            }
        }
    }
    __syncthreads();
    if (lane == 0) {
        long long S = 0;
        for (int q = 0; q < 128; ++q) S += (long long)sh.acc[q] * sh.acc[q];
        const long long cap_v = (long long)floor(0.2 * sqrt((double)S));
        long long S2 = 0;
        for (int q = 0; q < 128; ++q) {
            const long long v = min((long long)sh.acc[q], cap_v);
            S2 += v * v;
        }
        sh.cap = cap_v;
        sh.root = sqrt((double)S2);
        sh.drop = S2 == 0 ? 1 : 0;
        if (!sh.drop) {
            double F[16];
            if (feat_frame(depth, P.H[0], P.W[0], fx, fy, cx, cy, o, s, y, x, c, sn, F)) {
                for (int q = 0; q < 16; ++q) frames[(size_t)kp * 16 + q] = F[q];
                ok[kp] = 1;
            } else {
                sh.drop = 1;
            }
        }
    }
    __syncthreads();
    if (sh.drop) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int q = lane + 64 * t;
        const long long v = min((long long)sh.acc[q], sh.cap);
        const int qv = (int)rint(256.0 * (double)v / sh.root);
        desc[(size_t)kp * 128 + q] = (uint8_t)(int8_t)min(127, qv);
    }
}

// ---- match --------------------------------------------------------------------------------------------------------------
typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v16i __attribute__((ext_vector_type(16)));
constexpr int MT_ROWS = 128;                 // model rows staged per step
constexpr int MT_STRIDE = 144;               // bytes per staged row: 128 + 16, so that 32 rows' 16-byte reads spread over the banks
constexpr int M_CHUNK = 2048;                // model rows per workgroup
constexpr int S_TILE = 128;                  // scene features per workgroup: 4 waves x 32 columns
constexpr int PAD_NORM = 0x3fffffff;         // |a|^2 of a row past Nm: never the minimum

__device__ __forceinline__ int sumsq_i8x16(v4i v) {
    int s = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const int e = (int)(int8_t)((unsigned)v[w] >> (8 * b));
            s += e * e;
        }
    return s;
}

__global__ void feat_fill_u64_kernel(unsigned long long* __restrict__ p, int n, unsigned long long v) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

__global__ __launch_bounds__(256) void feat_match_kernel(const uint8_t* __restrict__ ds, const uint8_t* __restrict__ oks,
                                                         const int32_t* __restrict__ count, int cap,
                                                         const uint8_t* __restrict__ dm, int Nm,
                                                         unsigned long long* __restrict__ keys) {
    __shared__ __attribute__((aligned(16))) unsigned char rows[MT_ROWS * MT_STRIDE];
    __shared__ int norms[MT_ROWS];
    const int n = count_or_0(count, cap);
    const int sbase = blockIdx.x * S_TILE;
    if (sbase >= n) return;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, col = lane & 31, half = lane >> 5;
    const int si = sbase + wave * 32 + col;
    const bool valid = si < n && oks[si] != 0;
    v4i b[4];
    int nb = 0;
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        b[kk] = si < n ? *(const v4i*)(ds + (size_t)si * 128 + kk * 32 + half * 16) : (v4i){0, 0, 0, 0};
        nb += sumsq_i8x16(b[kk]);
    }
    nb += __shfl_xor(nb, 32);
    int best_d2 = 0x7fffffff, best_j = 0x7fffffff;
    const int m_end = min(Nm, (int)((blockIdx.y + 1) * M_CHUNK));
    for (int m0 = blockIdx.y * M_CHUNK; m0 < m_end; m0 += MT_ROWS) {
        __syncthreads();
#pragma unroll
        for (int it = 0; it < MT_ROWS * 8 / 256; ++it) {
            const int q = tid + 256 * it, row = q >> 3, ch = q & 7, j = m0 + row;
            const v4i v = j < Nm ? *(const v4i*)(dm + (size_t)j * 128 + ch * 16) : (v4i){0, 0, 0, 0};
            *(v4i*)(rows + row * MT_STRIDE + ch * 16) = v;
            int sq = sumsq_i8x16(v);
            sq += __shfl_xor(sq, 1);
            sq += __shfl_xor(sq, 2);
            sq += __shfl_xor(sq, 4);
            if (ch == 0) norms[row] = j < Nm ? sq : PAD_NORM;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < MT_ROWS / 32; ++t) {
            v16i acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
                const v4i a = *(const v4i*)(rows + (t * 32 + col) * MT_STRIDE + kk * 32 + half * 16);
                acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(a, b[kk], acc, 0, 0, 0);
            }
            // C / D: column = lane & 31 (scene), row = acc_row(r, lane >> 5) (model; csrc/mfma.h): ascending in r, so a
            // strict < keeps the lowest j among equal d2 within the lane
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = t * 32 + acc_row(r, half);
                const int d2 = (norms[row] + nb) - 2 * acc[r];
                if (d2 < best_d2) best_d2 = d2, best_j = m0 + row;
            }
        }
    }
    unsigned long long key = ((unsigned long long)(unsigned)best_d2 << 32) | (unsigned)best_j;
    const unsigned long long other = __shfl_xor(key, 32);
    key = other < key ? other : key;
    if (half == 0 && valid && best_j != 0x7fffffff) atomicMin(&keys[si], key);
}

__global__ void feat_match_finish_kernel(const unsigned long long* __restrict__ keys, const int32_t* __restrict__ count, int cap,
                                         int32_t* __restrict__ match) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count_or_0(count, cap)) return;
    const unsigned long long k = keys[i];
    int j = -1, d2 = 0, w = 0;
    if (k != ~0ull) {
        j = (int)(k & 0xffffffffu), d2 = (int)(k >> 32);
        w = max(0, 1024 - (d2 >> 6));
    }
    match[3 * i] = j, match[3 * i + 1] = d2, match[3 * i + 2] = w;
}

// ---- hypotheses ---------------------------------------------------------------------------------------------------------
__global__ void feat_hypotheses_kernel(const int32_t* __restrict__ match, const double* __restrict__ Fs,
                                       const int32_t* __restrict__ count, int cap, const double* __restrict__ Fm, int Nm,
                                       int32_t* __restrict__ peaks, double* __restrict__ cand) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count_or_0(count, cap)) return;
    const int j = match[3 * i], w = match[3 * i + 2];
    double* T = cand + 16 * (size_t)i;
    if (w <= 0 || j < 0 || j >= Nm) {
        peaks[3 * i] = 0, peaks[3 * i + 1] = 0, peaks[3 * i + 2] = 0;
        for (int q = 0; q < 16; ++q) T[q] = 0.0;
        return;
    }
    const double* A = Fs + 16 * (size_t)i;
    const double* M = Fm + 16 * (size_t)j;
    double B[12];                                   // [R^T | -(R^T t)] of the model frame
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) B[4 * a + b] = M[4 * b + a];
        B[4 * a + 3] = -((M[a] * M[3] + M[4 + a] * M[7]) + M[8 + a] * M[11]);
    }
    for (int a = 0; a < 3; ++a) {
        for (int b = 0; b < 3; ++b) T[4 * a + b] = (A[4 * a] * B[b] + A[4 * a + 1] * B[4 + b]) + A[4 * a + 2] * B[8 + b];
        T[4 * a + 3] = ((A[4 * a] * B[3] + A[4 * a + 1] * B[7]) + A[4 * a + 2] * B[11]) + A[4 * a + 3];
    }
    T[12] = 0.0, T[13] = 0.0, T[14] = 0.0, T[15] = 1.0;
    peaks[3 * i] = j, peaks[3 * i + 1] = 0, peaks[3 * i + 2] = w;
}

bool intrinsics_ok(float fx, float fy, float cx, float cy) {
    return fx != 0.0f && fy != 0.0f && isfinite(fx) && isfinite(fy) && isfinite(cx) && isfinite(cy);
}

int detect_blocks(const Pyr& P) { return (int)((P.flat[MAX_OCT] + DNT - 1) / DNT); }

}  // namespace

extern "C" {

size_t ossid_feat_pyramid_bytes(int H, int W, int octaves) {
    Pyr P;
    return make_pyr(H, W, octaves, &P) ? (size_t)P.words * 4 : 0;
}

int ossid_feat_pyramid(const uint8_t* img, int H, int W, int octaves, void* pyramid, size_t pyramid_bytes, void* stream) {
    Pyr P;
    if (!make_pyr(H, W, octaves, &P) || !img || !pyramid || pyramid_bytes < (size_t)P.words * 4) return OSSID_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    int32_t* base = (int32_t*)pyramid;
    int32_t* tmp[2] = {base + P.tmp, base + P.tmp + (long long)H * W};
    const long long n = (long long)H * W;
    hipLaunchKernelGGL(feat_grey_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, img, n, tmp[0]);
    for (int o = 0; o < P.n_oct; ++o) {
        const int h = P.H[o], w = P.W[o];
        const long long plane = (long long)h * w;
        int32_t* L = base + P.off[o];
        const dim3 grid((w + 127) / 128, h), block(128);
        if (o == 0)
            hipLaunchKernelGGL(feat_pass_kernel, grid, block, 0, st, (const int32_t*)tmp[0], h, w, L);
        else
            hipLaunchKernelGGL(feat_down_kernel, grid, block, 0, st, (const int32_t*)(base + P.off[o - 1] + 2 * (long long)P.H[o - 1] * P.W[o - 1]),
                               P.W[o - 1], h, w, L);
        for (int l = 1; l < NLEV; ++l) {
            const int passes = 1 << (l - 1);
            const int32_t* src = L + (l - 1) * plane;
            for (int p = 0; p < passes; ++p) {
                int32_t* dst = p == passes - 1 ? L + l * plane : tmp[p & 1];
                hipLaunchKernelGGL(feat_pass_kernel, grid, block, 0, st, src, h, w, dst);
                src = dst;
            }
        }
    }
    return ossid_launch_status();
}

size_t ossid_feat_detect_workspace_bytes(int H, int W, int octaves) {
    Pyr P;
    if (!make_pyr(H, W, octaves, &P)) return 0;
    return (size_t)detect_blocks(P) * 4 + (size_t)P.flat[MAX_OCT];
}

int ossid_feat_detect(const void* pyramid, int H, int W, int octaves, const float* depth, const uint8_t* mask, int contrast,
                      int max_keypoints, void* workspace, size_t workspace_bytes, int32_t* keypoints, int32_t* count,
                      void* stream) {
    Pyr P;
    if (!make_pyr(H, W, octaves, &P) || !pyramid || !depth || !mask || !workspace || !keypoints || !count) return OSSID_EINVAL;
    if (contrast < 1 || max_keypoints < 1 || max_keypoints > OSSID_FEAT_MAX_KEYPOINTS) return OSSID_EINVAL;
    if (workspace_bytes < ossid_feat_detect_workspace_bytes(H, W, octaves)) return OSSID_EINVAL;
    const int nb = detect_blocks(P);
    int32_t* bcount = (int32_t*)workspace;
    uint8_t* flags = (uint8_t*)(bcount + nb);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(feat_flag_kernel, dim3(nb), dim3(DNT), 0, st, P, (const int32_t*)pyramid, depth, mask, contrast, flags, bcount);
    hipLaunchKernelGGL(feat_scan_kernel, dim3(1), dim3(1024), 0, st, bcount, nb, max_keypoints, count);
    hipLaunchKernelGGL(feat_compact_kernel, dim3(nb), dim3(DNT), 0, st, P, (const uint8_t*)flags, (const int32_t*)bcount,
                       max_keypoints, keypoints);
    return ossid_launch_status();
}

int ossid_feat_describe(const void* pyramid, int H, int W, int octaves, const float* depth, float fx, float fy, float cx,
                        float cy, const int32_t* keypoints, const int32_t* count, int max_keypoints, int32_t* bins,
                        uint8_t* descriptors, double* frames, uint8_t* ok, void* stream) {
    Pyr P;
    if (!make_pyr(H, W, octaves, &P) || !pyramid || !depth || !keypoints || !count || !bins || !descriptors || !frames || !ok)
        return OSSID_EINVAL;
    if (max_keypoints < 1 || max_keypoints > OSSID_FEAT_MAX_KEYPOINTS || !intrinsics_ok(fx, fy, cx, cy)) return OSSID_EINVAL;
    static const FeatTables T = make_tables();
    hipLaunchKernelGGL(feat_describe_kernel, dim3(max_keypoints), dim3(64), 0, (hipStream_t)stream, P, T, (const int32_t*)pyramid,
                       depth, fx, fy, cx, cy, keypoints, count, max_keypoints, bins, descriptors, frames, ok);
    return ossid_launch_status();
}

size_t ossid_feat_match_workspace_bytes(int max_keypoints) {
    if (max_keypoints < 1 || max_keypoints > OSSID_FEAT_MAX_KEYPOINTS) return 0;
    return (size_t)max_keypoints * 8;
}

int ossid_feat_match(const uint8_t* scene_descriptors, const uint8_t* scene_ok, const int32_t* count, int max_keypoints,
                     const uint8_t* model_descriptors, int Nm, void* workspace, size_t workspace_bytes, int32_t* match,
                     void* stream) {
    const size_t need = ossid_feat_match_workspace_bytes(max_keypoints);
    if (need == 0 || !scene_descriptors || !scene_ok || !count || !workspace || !match || workspace_bytes < need)
        return OSSID_EINVAL;
    if (Nm < 0 || Nm > OSSID_FEAT_MAX_MODEL_FEATURES || (Nm > 0 && !model_descriptors)) return OSSID_EINVAL;
    if (((uintptr_t)scene_descriptors | (uintptr_t)model_descriptors) & 15 || ((uintptr_t)workspace & 7)) return OSSID_EINVAL;
    unsigned long long* keys = (unsigned long long*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(feat_fill_u64_kernel, dim3((max_keypoints + 255) / 256), dim3(256), 0, st, keys, max_keypoints, ~0ull);
    if (Nm > 0)
        hipLaunchKernelGGL(feat_match_kernel, dim3((max_keypoints + S_TILE - 1) / S_TILE, (Nm + M_CHUNK - 1) / M_CHUNK), dim3(256),
                           0, st, scene_descriptors, scene_ok, count, max_keypoints, model_descriptors, Nm, keys);
    hipLaunchKernelGGL(feat_match_finish_kernel, dim3((max_keypoints + 255) / 256), dim3(256), 0, st,
                       (const unsigned long long*)keys, count, max_keypoints, match);
    return ossid_launch_status();
}

int ossid_feat_hypotheses(const int32_t* match, const double* scene_frames, const int32_t* count, int max_keypoints,
                          const double* model_frames, int Nm, int32_t* peaks, double* cand_poses, void* stream) {
    if (!match || !scene_frames || !count || !peaks || !cand_poses || max_keypoints < 1 ||
        max_keypoints > OSSID_FEAT_MAX_KEYPOINTS || Nm < 0 || Nm > OSSID_FEAT_MAX_MODEL_FEATURES || (Nm > 0 && !model_frames))
        return OSSID_EINVAL;
    hipLaunchKernelGGL(feat_hypotheses_kernel, dim3((max_keypoints + 255) / 256), dim3(256), 0, (hipStream_t)stream, match,
                       scene_frames, count, max_keypoints, model_frames, Nm, peaks, cand_poses);
    return ossid_launch_status();
}

}  // extern "C"
