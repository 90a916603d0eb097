// Point-pair-feature pose hypotheses (Drost et al., CVPR 2010) as SPEC.md section 6 defines them, in place of Halcon's
// find_surface_model (scripts/online_learning.py:295-301 builds the models, :413-418 / :441-447 finds the poses).
//
//   sample       voxel-grid subsampling, shared by model and scene: bounds (one workgroup), an open-addressing hash of
//                voxels keeping the lowest input index (atomicCAS / atomicMin: the result does not depend on the order the
//                atomics run in), per-block representative counts, an ordered compaction (each block sums the counts of
//                the blocks before it: our own scan). Input is an f32 cloud or a depth image + mask (row-major pixels).
//                h = 0 (no diameter given and all valid points in one place, D = 0) keeps nothing: count = 0.
//   model table  one thread per ordered model pair: key and rotation bin, counting sort into a dense [key][chunk] offset
//                table (global atomics count, one workgroup scans, global atomics place) of u32 entries m_r * 32 + bin_m.
//   normals      per sampled scene point: brute-force neighbours in index order, f64 covariance, Jacobi in registers.
//   vote         one workgroup per (reference point, chunk of 1024 model reference points): 1024 x 30 u32 accumulator
//                in LDS; partners' table ranges flattened through an LDS prefix so lanes stride over entries; LDS
//                atomics; workgroup argmax (ties to the lowest m_r * 30 + alpha). A second kernel merges the chunks' peaks
//                and builds the f64 pose.
//   cluster      one workgroup: bitonic sort of the candidates in LDS, the greedy pass with every candidate tested
//                against all seeds in parallel, a second sort of the clusters by votes.
// No output is cleared with a memset: every output and every workspace word a kernel reads is written by a kernel.
#include <float.h>
#include <math.h>

#include "workgroup.h"

namespace {

constexpr int NA = 15;                       // angle bins over [0, pi]
constexpr int NALPHA = 30;                   // rotation bins over 2 pi
constexpr int NKEY_ANG = NA * NA * NA;
constexpr int CHUNK = 1024;                  // model reference points per vote workgroup
constexpr int MAX_DIST_BINS = 128;
constexpr uint32_t EMPTY = 0xffffffffu;
constexpr int SNT = 1024;                    // sampling: points per block
constexpr int VNT = 512;                     // vote workgroup
constexpr int CNT = 1024;                    // cluster workgroup
constexpr int MAX_SORT = 8192;
static_assert(OSSID_PPF_MAX_SCENE_SAMPLES <= MAX_SORT, "cluster sort size");

struct PpfTables {
    float dist2[MAX_DIST_BINS];              // f32((k h)^2), k = 1 .. nd-1
    float d2max;                             // f32(D^2)
    float cos_a[NA - 1];                     // f32(cos(k pi / 15)), k = 1 .. 14: angle bins and sector directions
    float sin_a[NA - 1];
    double rot_c[NALPHA], rot_s[NALPHA];     // cos / sin(alpha 12 degrees)
    int nd;
};

PpfTables make_tables(float h, float D) {
    PpfTables t;
    const double h64 = (double)h;
    t.nd = (int)floor((double)D / h64) + 1;
    for (int k = 0; k < MAX_DIST_BINS; ++k) {
        const double kh = (double)(k + 1) * h64;
        t.dist2[k] = k + 1 < t.nd ? (float)(kh * kh) : FLT_MAX;
    }
    t.d2max = (float)((double)D * (double)D);
    for (int k = 1; k < NA; ++k) {
        const double a = (double)k * M_PI / NA;
        t.cos_a[k - 1] = (float)cos(a);
        t.sin_a[k - 1] = (float)sin(a);
    }
    for (int a = 0; a < NALPHA; ++a) {
        const double th = (double)a * 2.0 * M_PI / NALPHA;
        t.rot_c[a] = cos(th);
        t.rot_s[a] = sin(th);
    }
    return t;
}

bool tables_ok(float h, float D) {
    if (!(h > 0.0f) || !(D > 0.0f) || !isfinite(h) || !isfinite(D)) return false;
    const double nd = floor((double)D / (double)h) + 1.0;
    return nd <= (double)MAX_DIST_BINS;
}

// ---- shared device helpers ----------------------------------------------------------------------------------------------
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// Duff et al. 2017: branch-free orthonormal basis (e1, e2) of a unit normal, f32
__device__ __forceinline__ void onb(const float* n, float* e1, float* e2) {
    const float sign = copysignf(1.0f, n[2]);
    const float a = -1.0f / (sign + n[2]);
    const float b = (n[0] * n[1]) * a;
    e1[0] = 1.0f + ((sign * n[0]) * n[0]) * a, e1[1] = sign * b, e1[2] = -(sign * n[0]);
    e2[0] = b, e2[1] = sign + (n[1] * n[1]) * a, e2[2] = -n[1];
}

// SPEC 6.4: feature of the ordered pair (reference r, partner i), the same for model and scene pairs.
// -> false when the pair has no key (coincident or farther than D apart); else key and the rotation bin.
__device__ __forceinline__ bool pair_feature(const PpfTables& T, const float* pr, const float* nr, const float* e1,
                                             const float* e2, const float* pi, const float* ni, int& key, int& bin) {
    const float dx = pi[0] - pr[0], dy = pi[1] - pr[1], dz = pi[2] - pr[2];
    const float dist2 = (dx * dx + dy * dy) + dz * dz;
    if (!(dist2 > 0.0f) || !(dist2 <= T.d2max)) return false;
    const float ln = sqrtf(dist2);
    const float c1 = dot3(nr[0], nr[1], nr[2], dx, dy, dz) / ln;
    const float c2 = dot3(ni[0], ni[1], ni[2], dx, dy, dz) / ln;
    const float c3 = dot3(nr[0], nr[1], nr[2], ni[0], ni[1], ni[2]);
    int db = 0;
    for (int k = 0; k + 1 < T.nd; ++k) db += dist2 >= T.dist2[k];
    int a1 = 0, a2 = 0, a3 = 0;
#pragma unroll
    for (int k = 0; k < NA - 1; ++k) {
        a1 += c1 <= T.cos_a[k];
        a2 += c2 <= T.cos_a[k];
        a3 += c3 <= T.cos_a[k];
    }
    key = ((db * NA + a1) * NA + a2) * NA + a3;
    float u = dot3(e1[0], e1[1], e1[2], dx, dy, dz), v = dot3(e2[0], e2[1], e2[2], dx, dy, dz);
    const bool lower = v < 0.0f || (v == 0.0f && u < 0.0f);
    if (lower) u = -u, v = -v;
    int b = 0;
#pragma unroll
    for (int k = 0; k < NA - 1; ++k) b += ((T.cos_a[k] * v) - (T.sin_a[k] * u)) >= 0.0f;
    bin = b + (lower ? 15 : 0);
    return true;
}

// ---- sampling ---------------------------------------------------------------------------------------------------------
struct Src {
    const float* pts;        // f32 [N][3] or null
    const float* nrm;        // model normals f32 [N][3] or null (scene)
    const float* depth;      // f32 [H][W] (with mask) when pts is null
    const uint8_t* mask;
    int n, W;
    float fx, fy, cx, cy;
};

// input point i -> validity and coordinates (SPEC 6.2: non-finite points dropped; scene points also need z > 0; model
// vertices also need a finite non-zero normal)
__device__ __forceinline__ bool load_point(const Src& s, int i, float* p) {
    if (s.pts) {
        p[0] = s.pts[3 * (size_t)i], p[1] = s.pts[3 * (size_t)i + 1], p[2] = s.pts[3 * (size_t)i + 2];
        bool ok = isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
        if (s.nrm) {
            const float* n = s.nrm + 3 * (size_t)i;
            const float l2 = (n[0] * n[0] + n[1] * n[1]) + n[2] * n[2];
            ok = ok && isfinite(l2) && l2 > 0.0f;
        } else {
            ok = ok && p[2] > 0.0f;
        }
        return ok;
    }
    const float z = s.depth[i];
    if (!(s.mask[i] != 0 && z > 0.0f)) return false;
    const int y = i / s.W, x = i - y * s.W;
    p[0] = ((float)x - s.cx) * z / s.fx;
    p[1] = ((float)y - s.cy) * z / s.fy;
    p[2] = z;
    return isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]);
}

// stats: lo[3], hi[3], D, h
__device__ __forceinline__ void voxel(const float* p, const float* stats, float* v) {
    const float h = stats[7];
    v[0] = floorf((p[0] - stats[0]) / h), v[1] = floorf((p[1] - stats[1]) / h), v[2] = floorf((p[2] - stats[2]) / h);
}

__device__ __forceinline__ uint32_t voxel_hash(const float* v, uint32_t mask) {
    uint32_t hsh = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int c = (int)fminf(fmaxf(v[a], -1.0e9f), 1.0e9f);
        hsh = (hsh ^ (uint32_t)c) * 0x9E3779B1u;
        hsh ^= hsh >> 15;
    }
    return hsh & mask;
}

__global__ __launch_bounds__(1024) void ppf_bounds_kernel(Src s, float rel, float diam, float* __restrict__ stats) {
    __shared__ float red[16][6];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < s.n; i += 1024) {
        float p[3];
        if (!load_point(s, i, p)) continue;
        for (int a = 0; a < 3; ++a) mn[a] = fminf(mn[a], p[a]), mx[a] = fmaxf(mx[a], p[a]);
    }
    wg_bbox3<16>(mn, mx, red);
    if (threadIdx.x == 0) {
        if (!(mn[0] <= mx[0]))                         // no valid point: an empty sample
            for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f;
        const float ex = mx[0] - mn[0], ey = mx[1] - mn[1], ez = mx[2] - mn[2];
        const float D = sqrtf((ex * ex + ey * ey) + ez * ez);
        for (int a = 0; a < 3; ++a) stats[a] = mn[a], stats[3 + a] = mx[a];
        stats[6] = D;
        stats[7] = rel * (diam > 0.0f ? diam : D);
    }
}

__global__ void ppf_fill_u32_kernel(uint32_t* __restrict__ p, size_t n, uint32_t v) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) p[i] = v;
}

__global__ __launch_bounds__(256) void ppf_hash_insert_kernel(Src s, const float* __restrict__ stats, uint32_t* __restrict__ table,
                                                              uint32_t tmask) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= s.n || !(stats[7] > 0.0f)) return;
    float p[3], v[3];
    if (!load_point(s, i, p)) return;
    voxel(p, stats, v);
    uint32_t slot = voxel_hash(v, tmask);
    for (uint32_t probe = 0; probe <= tmask; ++probe, slot = (slot + 1) & tmask) {
        uint32_t cur = table[slot];
        if (cur == EMPTY) {
            cur = atomicCAS(&table[slot], EMPTY, (uint32_t)i);
            if (cur == EMPTY) return;
        }
        float q[3], w[3];
        load_point(s, (int)cur, q);                    // any index in a slot identifies the slot's voxel
        voxel(q, stats, w);
        if (w[0] == v[0] && w[1] == v[1] && w[2] == v[2]) {
            atomicMin(&table[slot], (uint32_t)i);
            return;
        }
    }
}

// point i is kept iff it is valid and its voxel's slot holds i (the voxel's lowest index)
__device__ __forceinline__ bool is_rep(const Src& s, const float* stats, const uint32_t* table, uint32_t tmask, int i, float* p) {
    if (i >= s.n || !(stats[7] > 0.0f) || !load_point(s, i, p)) return false;
    float v[3];
    voxel(p, stats, v);
    uint32_t slot = voxel_hash(v, tmask);
    for (uint32_t probe = 0; probe <= tmask; ++probe, slot = (slot + 1) & tmask) {
        const uint32_t cur = table[slot];
        if (cur == EMPTY) return false;
        float q[3], w[3];
        load_point(s, (int)cur, q);
        voxel(q, stats, w);
        if (w[0] == v[0] && w[1] == v[1] && w[2] == v[2]) return cur == (uint32_t)i;
    }
    return false;
}

__global__ __launch_bounds__(SNT) void ppf_rep_count_kernel(Src s, const float* __restrict__ stats,
                                                            const uint32_t* __restrict__ table, uint32_t tmask,
                                                            int* __restrict__ block_counts) {
    __shared__ int wsum[SNT / 64];
    float p[3];
    const int f = is_rep(s, stats, table, tmask, blockIdx.x * SNT + threadIdx.x, p) ? 1 : 0;
    int total;
    block_scan_excl<SNT / 64>(f, OpAdd(), 0, wsum, total, false);
    if (threadIdx.x == 0) block_counts[blockIdx.x] = total;
}

__global__ __launch_bounds__(SNT) void ppf_compact_kernel(Src s, const float* __restrict__ stats, const uint32_t* __restrict__ table,
                                                          uint32_t tmask, const int* __restrict__ block_counts, int max_out,
                                                          int32_t* __restrict__ idx_out, float* __restrict__ pts_out,
                                                          float* __restrict__ nrm_out, int32_t* __restrict__ count) {
    __shared__ int wsum[SNT / 64];
    __shared__ int base_sh;
    if (threadIdx.x == 0) base_sh = 0;
    __syncthreads();
    int part = 0;                                        // counts of the blocks before this one (all blocks: block 0)
    const int upto = blockIdx.x == 0 ? (int)gridDim.x : (int)blockIdx.x;
    for (int b = threadIdx.x; b < upto; b += SNT) part += block_counts[b];
    atomicAdd(&base_sh, part);
    __syncthreads();
    const int base = blockIdx.x == 0 ? 0 : base_sh;
    if (blockIdx.x == 0 && threadIdx.x == 0) count[0] = base_sh;   // the true count, also past max_out
    const int i = blockIdx.x * SNT + threadIdx.x;
    float p[3];
    const bool rep = is_rep(s, stats, table, tmask, i, p);
    int total;
    const int pos = base + block_scan_excl<SNT / 64>(rep ? 1 : 0, OpAdd(), 0, wsum, total, false);
    if (rep && pos < max_out) {
        idx_out[pos] = i;
        pts_out[3 * pos] = p[0], pts_out[3 * pos + 1] = p[1], pts_out[3 * pos + 2] = p[2];
        if (nrm_out) {
            const float* n = s.nrm + 3 * (size_t)i;
            const float ln = sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
            nrm_out[3 * pos] = n[0] / ln, nrm_out[3 * pos + 1] = n[1] / ln, nrm_out[3 * pos + 2] = n[2] / ln;
        }
    }
}

// ---- model table ----------------------------------------------------------------------------------------------------
// one workgroup per model reference point r, threads over partners i; pass 0 counts, pass 1 places
template <int PASS>
__global__ __launch_bounds__(256) void ppf_model_pairs_kernel(const float* __restrict__ P, const float* __restrict__ N, int Ms,
                                                              PpfTables T, int nch, uint32_t* __restrict__ slots,
                                                              uint32_t* __restrict__ entries, int64_t max_entries) {
    const int r = blockIdx.x;
    float pr[3], nr[3], e1[3], e2[3];
    for (int a = 0; a < 3; ++a) pr[a] = P[3 * r + a], nr[a] = N[3 * r + a];
    onb(nr, e1, e2);
    const int chunk = r / CHUNK;
    for (int i = threadIdx.x; i < Ms; i += 256) {
        if (i == r) continue;
        int key, bin;
        if (!pair_feature(T, pr, nr, e1, e2, P + 3 * i, N + 3 * i, key, bin)) continue;
        const uint32_t pos = atomicAdd(&slots[(size_t)key * nch + chunk], 1u);
        if (PASS == 1 && (int64_t)pos < max_entries) entries[pos] = (uint32_t)r * 32u + (uint32_t)bin;
    }
}

// one workgroup: exclusive scan of counts[0 .. L-1] -> offsets[0 .. L] and the placing cursors
__global__ __launch_bounds__(1024) void ppf_scan_kernel(const uint32_t* counts, int64_t L,   // counts may alias cursor
                                                        uint32_t* __restrict__ offsets, uint32_t* cursor) {
    __shared__ uint32_t wsum[16];
    const uint32_t total = wg_scan_range<16>(counts, L, wsum, [&](int64_t j, uint32_t base) { offsets[j] = base, cursor[j] = base; });
    if (threadIdx.x == 0) offsets[L] = total;
}

// ---- scene normals ----------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jacobi3(double (&A)[9], double (&V)[9], int p, int q) {
    const double apq = A[3 * p + q];
    if (apq == 0.0) return;
    const double theta = (A[4 * q] - A[4 * p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double akp = A[3 * k + p], akq = A[3 * k + q];
        A[3 * k + p] = c * akp - s * akq, A[3 * k + q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double apk = A[3 * p + k], aqk = A[3 * q + k];
        A[3 * p + k] = c * apk - s * aqk, A[3 * q + k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double vkp = V[3 * k + p], vkq = V[3 * k + q];
        V[3 * k + p] = c * vkp - s * vkq, V[3 * k + q] = s * vkp + c * vkq;
    }
}

__global__ __launch_bounds__(256) void ppf_normals_kernel(const float* __restrict__ S, const int32_t* __restrict__ count, int cap,
                                                          float r2, float* __restrict__ nrm, uint8_t* __restrict__ ok) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= cap) return;
    const int n = count[0] <= cap ? count[0] : 0;
    bool good = false;
    float out[3] = {0.0f, 0.0f, 0.0f};
    if (i < n) {
        const float px = S[3 * i], py = S[3 * i + 1], pz = S[3 * i + 2];
        double sum[3] = {0.0, 0.0, 0.0};
        int k = 0;
        for (int j = 0; j < n; ++j) {
            const float dx = S[3 * j] - px, dy = S[3 * j + 1] - py, dz = S[3 * j + 2] - pz;
            if ((dx * dx + dy * dy) + dz * dz <= r2) {
                sum[0] += (double)S[3 * j], sum[1] += (double)S[3 * j + 1], sum[2] += (double)S[3 * j + 2];
                ++k;
            }
        }
        if (k >= 3) {
            const double mu[3] = {sum[0] / k, sum[1] / k, sum[2] / k};
            double A[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            for (int j = 0; j < n; ++j) {
                const float dx = S[3 * j] - px, dy = S[3 * j + 1] - py, dz = S[3 * j + 2] - pz;
                if ((dx * dx + dy * dy) + dz * dz <= r2) {
                    const double x[3] = {(double)S[3 * j] - mu[0], (double)S[3 * j + 1] - mu[1], (double)S[3 * j + 2] - mu[2]};
#pragma unroll
                    for (int a = 0; a < 3; ++a)
#pragma unroll
                        for (int b = 0; b < 3; ++b) A[3 * a + b] += x[a] * x[b];
                }
            }
            double V[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
            for (int sweep = 0; sweep < 32; ++sweep) {
                const double off = (A[1] * A[1] + A[2] * A[2]) + A[5] * A[5];
                const double dia = (A[0] * A[0] + A[4] * A[4]) + A[8] * A[8];
                if (!(off > 1e-36 * dia)) break;
                jacobi3(A, V, 0, 1);
                jacobi3(A, V, 0, 2);
                jacobi3(A, V, 1, 2);
            }
            int m = 0;
            if (A[4] < A[4 * m]) m = 1;
            if (A[8] < A[4 * m]) m = 2;
            const double vx = V[m], vy = V[3 + m], vz = V[6 + m];
            const double inv = sqrt((vx * vx + vy * vy) + vz * vz);
            out[0] = (float)(vx / inv), out[1] = (float)(vy / inv), out[2] = (float)(vz / inv);
            if (dot3(out[0], out[1], out[2], px, py, pz) > 0.0f) out[0] = -out[0], out[1] = -out[1], out[2] = -out[2];
            good = true;
        }
    }
    nrm[3 * i] = out[0], nrm[3 * i + 1] = out[1], nrm[3 * i + 2] = out[2];
    ok[i] = good ? 1 : 0;
}

// ---- vote -------------------------------------------------------------------------------------------------------------
struct VoteShared {
    uint32_t acc[CHUNK * NALPHA];              // 120 KiB
    int pre[VNT], start[VNT], bin[VNT];
    int wsum[VNT / 64];
    uint32_t bc[VNT / 64];
    int bi[VNT / 64];
};

__global__ __launch_bounds__(VNT) void ppf_vote_kernel(const float* __restrict__ S, const float* __restrict__ Sn,
                                                       const uint8_t* __restrict__ Sok, const int32_t* __restrict__ count,
                                                       int cap, int ref_step, const uint32_t* __restrict__ offsets,
                                                       const uint32_t* __restrict__ entries, int Ms, int nch, PpfTables T,
                                                       uint2* __restrict__ peaks) {
    __shared__ VoteShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int slot = blockIdx.x, chunk = blockIdx.y, r = slot * ref_step;
    const int n = count_or_0(count, cap);
    uint2* out = peaks + (size_t)slot * nch + chunk;
    if (r >= n || !Sok[r]) {
        if (tid == 0) *out = make_uint2(0u, 0u);
        return;
    }
    const int mc = min(CHUNK, Ms - chunk * CHUNK);
    for (int j = tid; j < mc * NALPHA; j += VNT) sh.acc[j] = 0u;
    float pr[3], nr[3], e1[3], e2[3];
    for (int a = 0; a < 3; ++a) pr[a] = S[3 * r + a], nr[a] = Sn[3 * r + a];
    onb(nr, e1, e2);
    for (int t0 = 0; t0 < n; t0 += VNT) {
        const int i = t0 + tid;
        int len = 0, st = 0, bn = 0;
        if (i < n && i != r && Sok[i]) {
            int key;
            if (pair_feature(T, pr, nr, e1, e2, S + 3 * i, Sn + 3 * i, key, bn)) {
                const size_t o = (size_t)key * nch + chunk;
                st = (int)offsets[o];
                len = (int)(offsets[o + 1] - offsets[o]);
            }
        }
        int total;
        const int pre = block_scan_excl<VNT / 64>(len, OpAdd(), 0, sh.wsum, total, false);
        sh.pre[tid] = pre, sh.start[tid] = st, sh.bin[tid] = bn;
        __syncthreads();
        for (int e = tid; e < total; e += VNT) {
            int lo = 0, hi = VNT - 1;                  // the last partner p with pre[p] <= e owns entry e
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (sh.pre[mid] <= e) lo = mid; else hi = mid - 1;
            }
            const uint32_t ent = entries[(size_t)sh.start[lo] + (e - sh.pre[lo])];
            int alpha = (int)(ent & 31u) - sh.bin[lo];
            if (alpha < 0) alpha += NALPHA;
            atomicAdd(&sh.acc[((int)(ent >> 5) - chunk * CHUNK) * NALPHA + alpha], 1u);
        }
        __syncthreads();
    }
    uint32_t bc = 0u;
    int bi = 0x7fffffff;
    for (int j = tid; j < mc * NALPHA; j += VNT)
        if (sh.acc[j] > bc) bc = sh.acc[j], bi = j;
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t oc = __shfl_xor(bc, m);
        const int oi = __shfl_xor(bi, m);
        if (oc > bc || (oc == bc && oi < bi)) bc = oc, bi = oi;
    }
    if (lane == 0) sh.bc[wv] = bc, sh.bi[wv] = bi;
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < VNT / 64; ++w)
            if (sh.bc[w] > bc || (sh.bc[w] == bc && sh.bi[w] < bi)) bc = sh.bc[w], bi = sh.bi[w];
        *out = bc > 0u ? make_uint2(bc, (uint32_t)(chunk * CHUNK * NALPHA + bi)) : make_uint2(0u, 0u);
    }
}

// per reference slot: merge the chunks' peaks, build the f64 pose p -> s + B_s Rx(-alpha 12 deg) B_m^T (p - m)
__global__ __launch_bounds__(256) void ppf_peak_pose_kernel(const float* __restrict__ S, const float* __restrict__ Sn,
                                                            const int32_t* __restrict__ count, int cap, int ref_step,
                                                            int max_ref, const float* __restrict__ P,
                                                            const float* __restrict__ N, int nch, PpfTables T,
                                                            const uint2* __restrict__ peaks, int32_t* __restrict__ peak_out,
                                                            double* __restrict__ cand_pose) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    if (j >= max_ref) return;
    const int n = count_or_0(count, cap), r = j * ref_step;
    uint32_t bc = 0u, bi = 0u;
    if (r < n)
        for (int c = 0; c < nch; ++c) {
            const uint2 pk = peaks[(size_t)j * nch + c];
            if (pk.x > bc || (pk.x == bc && pk.x > 0u && pk.y < bi)) bc = pk.x, bi = pk.y;
        }
    double Tm[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) Tm[k] = (k % 5) == 0 ? 1.0 : 0.0;
    const int m_r = (int)(bi / NALPHA), alpha = (int)(bi % NALPHA);
    if (bc > 0u) {
        float ns[3], es1[3], es2[3], nm[3], em1[3], em2[3];
        for (int a = 0; a < 3; ++a) ns[a] = Sn[3 * r + a], nm[a] = N[3 * m_r + a];
        onb(ns, es1, es2);
        onb(nm, em1, em2);
        const double Bs[9] = {ns[0], es1[0], es2[0], ns[1], es1[1], es2[1], ns[2], es1[2], es2[2]};   // columns n, e1, e2
        const double Bm[9] = {nm[0], em1[0], em2[0], nm[1], em1[1], em2[1], nm[2], em1[2], em2[2]};
        const double c = T.rot_c[alpha], s = T.rot_s[alpha];
        const double Rx[9] = {1.0, 0.0, 0.0, 0.0, c, s, 0.0, -s, c};
        double M1[9];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) M1[3 * a + b] = (Rx[3 * a] * Bm[3 * b] + Rx[3 * a + 1] * Bm[3 * b + 1]) + Rx[3 * a + 2] * Bm[3 * b + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) Tm[4 * a + b] = (Bs[3 * a] * M1[b] + Bs[3 * a + 1] * M1[3 + b]) + Bs[3 * a + 2] * M1[6 + b];
        const double m[3] = {P[3 * m_r], P[3 * m_r + 1], P[3 * m_r + 2]};
#pragma unroll
        for (int a = 0; a < 3; ++a)
            Tm[4 * a + 3] = (double)S[3 * r + a] - ((Tm[4 * a] * m[0] + Tm[4 * a + 1] * m[1]) + Tm[4 * a + 2] * m[2]);
    }
    peak_out[3 * j] = bc > 0u ? m_r : 0, peak_out[3 * j + 1] = bc > 0u ? alpha : 0, peak_out[3 * j + 2] = (int32_t)bc;
#pragma unroll
    for (int k = 0; k < 16; ++k) cand_pose[16 * (size_t)j + k] = Tm[k];
}

// ---- cluster ----------------------------------------------------------------------------------------------------------
struct ClusterShared {
    unsigned long long key[MAX_SORT];
    uint32_t sum[MAX_SORT];
    int seed[MAX_SORT];
    int ncand, nseed, first;
};

__global__ __launch_bounds__(CNT) void ppf_cluster_kernel(const int32_t* __restrict__ peak, const double* __restrict__ cand_pose,
                                                          const int32_t* __restrict__ count, int cap, int ref_step,
                                                          int max_ref, double thr2, double cos_thr, int Ms, int num_result,
                                                          double* __restrict__ poses_out, double* __restrict__ scores_out,
                                                          int32_t* __restrict__ info) {
    __shared__ ClusterShared sh;
    const int tid = threadIdx.x;
    const int n = count_or_0(count, cap);
    const int nref = min((n + ref_step - 1) / ref_step, max_ref);
    int np2 = 2;
    while (np2 < nref) np2 <<= 1;
    if (tid == 0) sh.ncand = 0, sh.nseed = 0, sh.first = 0x7fffffff;
    __syncthreads();
    for (int j = tid; j < np2; j += CNT) {
        const uint32_t v = j < nref ? (uint32_t)peak[3 * j + 2] : 0u;
        sh.key[j] = v > 0u ? ((unsigned long long)(~v) << 32) | (unsigned)j : ~0ull;
        if (v > 0u) atomicAdd(&sh.ncand, 1);
    }
    __syncthreads();
    wg_bitonic_sort(sh.key, np2);
    const int ncand = sh.ncand;
    for (int c = 0; c < ncand; ++c) {
        const int j = (int)(sh.key[c] & 0xffffffffu);
        const double* Tc = cand_pose + 16 * (size_t)j;
        const int ns = sh.nseed;
        for (int s = tid; s < ns; s += CNT) {
            const double* Ts = cand_pose + 16 * (size_t)sh.seed[s];
            const double dx = Tc[3] - Ts[3], dy = Tc[7] - Ts[7], dz = Tc[11] - Ts[11];
            if (!(((dx * dx + dy * dy) + dz * dz) <= thr2)) continue;
            double tr = 0.0;
#pragma unroll
            for (int a = 0; a < 3; ++a)
#pragma unroll
                for (int b = 0; b < 3; ++b) tr += Tc[4 * a + b] * Ts[4 * a + b];
            if ((tr - 1.0) / 2.0 >= cos_thr) atomicMin(&sh.first, s);
        }
        __syncthreads();
        if (tid == 0) {
            const uint32_t v = ~(uint32_t)(sh.key[c] >> 32);
            if (sh.first < ns) {
                sh.sum[sh.first] += v;
            } else {
                sh.seed[ns] = j, sh.sum[ns] = v;
                sh.nseed = ns + 1;
            }
            sh.first = 0x7fffffff;
        }
        __syncthreads();
    }
    const int nseed = sh.nseed;
    int np3 = 2;
    while (np3 < nseed) np3 <<= 1;
    for (int s = tid; s < np3; s += CNT)
        sh.key[s] = s < nseed ? ((unsigned long long)(~sh.sum[s]) << 32) | (unsigned)s : ~0ull;
    __syncthreads();
    wg_bitonic_sort(sh.key, np3);
    const int nres = min(nseed, num_result);
    for (int k = tid; k < num_result; k += CNT) {
        double sc = 0.0;
        if (k < nres) {
            const int s = (int)(sh.key[k] & 0xffffffffu);
            const double* Ts = cand_pose + 16 * (size_t)sh.seed[s];
            for (int q = 0; q < 16; ++q) poses_out[16 * (size_t)k + q] = Ts[q];
            sc = (double)sh.sum[s] / (double)Ms;
        } else {
            for (int q = 0; q < 16; ++q) poses_out[16 * (size_t)k + q] = 0.0;
        }
        scores_out[k] = sc;
    }
    if (tid == 0) info[0] = nres, info[1] = count[0], info[2] = ncand, info[3] = nseed;
}

uint32_t table_size(int n) {
    uint32_t t = 1024;
    while (t < 2u * (uint32_t)n) t <<= 1;
    return t;
}

int n_blocks(int n) { return (n + SNT - 1) / SNT; }

}  // namespace

extern "C" {

size_t ossid_ppf_sample_workspace_bytes(int n_in) {
    if (n_in <= 0 || n_in > (1 << 28)) return 0;
    return (size_t)table_size(n_in) * 4 + (size_t)n_blocks(n_in) * 4;
}

int ossid_ppf_sample(const float* points, const float* normals, int N, const float* depth, const uint8_t* mask, int H, int W,
                     float fx, float fy, float cx, float cy, float rel, float diam, int max_out, void* workspace,
                     size_t workspace_bytes, int32_t* idx_out, float* pts_out, float* nrm_out, int32_t* count,
                     float* stats, void* stream) {
    Src s{points, normals, depth, mask, 0, W, fx, fy, cx, cy};
    if (points) {
        if (depth || mask || N <= 0) return OSSID_EINVAL;
        s.n = N;
    } else {
        if (!depth || !mask || normals || H <= 0 || W <= 0 || (int64_t)H * W > (1 << 28)) return OSSID_EINVAL;
        if (!(fx != 0.0f) || !(fy != 0.0f) || !isfinite(fx) || !isfinite(fy) || !isfinite(cx) || !isfinite(cy))
            return OSSID_EINVAL;
        s.n = H * W;
    }
    if ((normals != nullptr) != (nrm_out != nullptr)) return OSSID_EINVAL;
    if (!idx_out || !pts_out || !count || !stats || !workspace || max_out <= 0) return OSSID_EINVAL;
    if (!(rel > 0.0f) || !isfinite(rel) || !isfinite(diam)) return OSSID_EINVAL;
    if (workspace_bytes < ossid_ppf_sample_workspace_bytes(s.n)) return OSSID_EINVAL;
    const uint32_t tsize = table_size(s.n);
    uint32_t* table = (uint32_t*)workspace;
    int* bcounts = (int*)(table + tsize);
    const int nb = n_blocks(s.n);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppf_bounds_kernel, dim3(1), dim3(1024), 0, st, s, rel, diam, stats);
    hipLaunchKernelGGL(ppf_fill_u32_kernel, dim3(min((tsize + 255) / 256, 1024u)), dim3(256), 0, st, table, (size_t)tsize, EMPTY);
    hipLaunchKernelGGL(ppf_hash_insert_kernel, dim3((s.n + 255) / 256), dim3(256), 0, st, s, (const float*)stats, table, tsize - 1);
    hipLaunchKernelGGL(ppf_rep_count_kernel, dim3(nb), dim3(SNT), 0, st, s, (const float*)stats, (const uint32_t*)table, tsize - 1,
                       bcounts);
    hipLaunchKernelGGL(ppf_compact_kernel, dim3(nb), dim3(SNT), 0, st, s, (const float*)stats, (const uint32_t*)table, tsize - 1,
                       (const int*)bcounts, max_out, idx_out, pts_out, nrm_out, count);
    return ossid_launch_status();
}

int64_t ossid_ppf_model_table_words(int Ms, float h, float D) {
    if (Ms <= 0 || Ms > OSSID_PPF_MAX_MODEL_POINTS || !tables_ok(h, D)) return 0;
    const int nch = (Ms + CHUNK - 1) / CHUNK;
    return (int64_t)make_tables(h, D).nd * NKEY_ANG * nch + 1;
}

int ossid_ppf_model_table(const float* points, const float* normals, int Ms, float h, float D, uint32_t* offsets,
                          uint32_t* entries, int64_t max_entries, void* workspace, size_t workspace_bytes, void* stream) {
    const int64_t L1 = ossid_ppf_model_table_words(Ms, h, D);
    if (L1 == 0 || !points || !normals || !offsets || !entries || !workspace || max_entries < (int64_t)Ms * (Ms - 1))
        return OSSID_EINVAL;
    if (workspace_bytes < (size_t)L1 * 4) return OSSID_EINVAL;
    const PpfTables T = make_tables(h, D);
    const int nch = (Ms + CHUNK - 1) / CHUNK;
    uint32_t* cnt = (uint32_t*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppf_fill_u32_kernel, dim3(1024), dim3(256), 0, st, cnt, (size_t)(L1 - 1), 0u);
    hipLaunchKernelGGL(ppf_model_pairs_kernel<0>, dim3(Ms), dim3(256), 0, st, points, normals, Ms, T, nch, cnt, entries,
                       max_entries);
    hipLaunchKernelGGL(ppf_scan_kernel, dim3(1), dim3(1024), 0, st, (const uint32_t*)cnt, L1 - 1, offsets, cnt);
    hipLaunchKernelGGL(ppf_model_pairs_kernel<1>, dim3(Ms), dim3(256), 0, st, points, normals, Ms, T, nch, cnt, entries,
                       max_entries);
    return ossid_launch_status();
}

int ossid_ppf_scene_normals(const float* scene, const int32_t* count, int cap, float radius, float* normals, uint8_t* ok,
                            void* stream) {
    if (!scene || !count || !normals || !ok || cap <= 0 || cap > OSSID_PPF_MAX_SCENE_SAMPLES) return OSSID_EINVAL;
    if (!(radius > 0.0f) || !isfinite(radius)) return OSSID_EINVAL;
    const float r2 = (float)((double)radius * (double)radius);
    hipLaunchKernelGGL(ppf_normals_kernel, dim3((cap + 255) / 256), dim3(256), 0, (hipStream_t)stream, scene, count, cap, r2,
                       normals, ok);
    return ossid_launch_status();
}

size_t ossid_ppf_vote_workspace_bytes(int cap, int ref_step, int Ms) {
    if (cap <= 0 || cap > OSSID_PPF_MAX_SCENE_SAMPLES || ref_step <= 0 || Ms <= 0 || Ms > OSSID_PPF_MAX_MODEL_POINTS) return 0;
    const int max_ref = (cap + ref_step - 1) / ref_step, nch = (Ms + CHUNK - 1) / CHUNK;
    return (size_t)max_ref * nch * sizeof(uint2);
}

int ossid_ppf_vote(const float* scene, const float* scene_normals, const uint8_t* scene_ok, const int32_t* count, int cap,
                   int ref_step, const float* model_points, const float* model_normals, int Ms, float h, float D,
                   const uint32_t* offsets, const uint32_t* entries, void* workspace, size_t workspace_bytes,
                   int32_t* peaks, double* cand_poses, void* stream) {
    const size_t need = ossid_ppf_vote_workspace_bytes(cap, ref_step, Ms);
    if (need == 0 || !tables_ok(h, D) || !scene || !scene_normals || !scene_ok || !count || !model_points || !model_normals ||
        !offsets || !entries || !workspace || !peaks || !cand_poses || workspace_bytes < need)
        return OSSID_EINVAL;
    const PpfTables T = make_tables(h, D);
    const int max_ref = (cap + ref_step - 1) / ref_step, nch = (Ms + CHUNK - 1) / CHUNK;
    uint2* pk = (uint2*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ppf_vote_kernel, dim3(max_ref, nch), dim3(VNT), 0, st, scene, scene_normals, scene_ok, count, cap, ref_step,
                       offsets, entries, Ms, nch, T, pk);
    hipLaunchKernelGGL(ppf_peak_pose_kernel, dim3((max_ref + 255) / 256), dim3(256), 0, st, scene, scene_normals, count, cap,
                       ref_step, max_ref, model_points, model_normals, nch, T, (const uint2*)pk, peaks, cand_poses);
    return ossid_launch_status();
}

int ossid_ppf_cluster(const int32_t* peaks, const double* cand_poses, const int32_t* count, int cap, int ref_step, int Ms,
                      float D, float dist_rel, int num_result, double* poses_out, double* scores_out, int32_t* info,
                      void* stream) {
    if (!peaks || !cand_poses || !count || !poses_out || !scores_out || !info) return OSSID_EINVAL;
    if (cap <= 0 || cap > OSSID_PPF_MAX_SCENE_SAMPLES || ref_step <= 0 || Ms <= 0 || num_result <= 0) return OSSID_EINVAL;
    if (!(D > 0.0f) || !isfinite(D) || !(dist_rel > 0.0f) || !isfinite(dist_rel)) return OSSID_EINVAL;
    const double thr = (double)dist_rel * (double)D;
    const double cos_thr = cos(M_PI / 15.0);
    const int max_ref = (cap + ref_step - 1) / ref_step;
    hipLaunchKernelGGL(ppf_cluster_kernel, dim3(1), dim3(CNT), 0, (hipStream_t)stream, peaks, cand_poses, count, cap, ref_step,
                       max_ref, thr * thr, cos_thr, Ms, num_result, poses_out, scores_out, info);
    return ossid_launch_status();
}

}  // extern "C"
