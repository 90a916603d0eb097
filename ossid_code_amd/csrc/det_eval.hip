// Detection mAP (SPEC.md section 10): the second figure the reference's run ends with -- scripts/online_learning.py:615-618
// calls evalFinetuneResults (utils/detection.py:137-187), which hands text files to an external script; the arithmetic of
// the metric that IS in the reference tree is utils/detection_metrics.py:20-156 (DetectionMetric.calculate_mAP) and :158-191
// (find_jaccard_overlap). That class walks the detections of a class one by one in score order and marks ground truths as
// taken. The order-free form used here: a detection is a true positive iff it is the highest-ranked of the detections that
// claim its ground truth -- an integer atomicMin per claim, independent of the order of arrival.
//
// ossid_det_claim (10.2-10.4), one launch:
//   claim     a thread per detection walks its image's ground truths (CSR), keeps the largest IoU of its class (lowest g
//             among equals, NaN never wins) and writes best_gt, best_iou and the sort key (cls << 32) | (~0u - m(score)).
// The caller sorts the keys (stable) and passes the permutation and the classes' offsets in it to
// ossid_det_match (10.5-10.8). Ranks r are positions in that order; a class owns the ranks [class_offset[c],
// class_offset[c+1]), cut into TILES of TILE ranks that never straddle two classes (tile_offset[c] = tiles before class c).
//   init      winner[T][G] = ~0u, n_easy = 0, p11 = 0; then n_easy by integer atomicAdd and tile_offset by one workgroup;
//   winner    every claiming (threshold, detection) does atomicMin(&winner[k][b], r);
//   status    FP / TP / ignored / duplicate per (k, detection), by input index (output) and by rank (workspace);
//   tile_sum  per tile the number of TPs and FPs, packed in one 64-bit word;
//   tile_scan one workgroup per threshold: exclusive sums over the tiles, TILE2 at a time with a running carry;
//   curve     per tile: the inclusive sums inside the tile plus the tile's prefix minus the prefix of the class's first tile
//             = ctp, cfp; prec, rec; p_j by a wave and workgroup maximum and ONE atomicMax per (tile, j) on the bits of the
//             non-negative float; and the tile's key ((~0u - c) << 32) | bits(max prec);
//   tile_sufmax one workgroup per threshold: exclusive suffix maxima of the tile keys. Classes ascend with the rank, so the
//             maximum over all later tiles IS the maximum over the later tiles of the lowest later class: the segmented
//             reverse scan is a plain one on these keys;
//   env       per tile: env_r = max(prec_s, s >= r in the class), and the tile's f64 sum of env over its TPs, added in a
//             fixed order (thread's four, xor butterfly, waves in order);
//   final     per (k, c): APa = (sum of the class's tile partials in tile order) / n_easy, AP11 from the p_j, and the means.
// No kernel waits on another workgroup. Everything lives in caller-owned memory; launches only, nothing read back.
#include <cmath>

#include "workgroup.h"

namespace {

constexpr int TILE = 1024;            // ranks per tile: 256 threads x 4 consecutive ranks
constexpr int TILE2 = 1024;           // tiles per step of the second-level scans: one per thread of a 1024-thread workgroup
constexpr int N_MAX = 1 << 22, G_MAX = 1 << 20, I_MAX = 1 << 20, C_MAX = 4096;
typedef unsigned long long u64;

enum : uint8_t { ST_FP = 0, ST_TP = 1, ST_IGNORED = 2, ST_DUP = 3, ST_NONE = 255 };

struct Thr {
    float t[OSSID_DET_MAX_THRESHOLDS];
};
struct RecThr {
    float t[11];
};

__host__ __device__ inline int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(256) void det_claim_kernel(const float* __restrict__ det_box, const float* __restrict__ det_score,
                                                        const int32_t* __restrict__ det_cls, const int32_t* __restrict__ det_image,
                                                        int N, const float* __restrict__ gt_box, const int32_t* __restrict__ gt_cls,
                                                        const int32_t* __restrict__ gt_offset, int G, int I, int C,
                                                        int32_t* __restrict__ best_gt, float* __restrict__ best_iou,
                                                        long long* __restrict__ sort_key) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    if (n >= N) return;
    const float4 d = *reinterpret_cast<const float4*>(det_box + 4 * (size_t)n);
    const int c = det_cls[n], im = det_image[n];
    int best = -1;
    float biou = 0.0f;
    if (im >= 0 && im < I) {
        const int g0 = clampi(gt_offset[im], 0, G), g1 = clampi(gt_offset[im + 1], g0, G);
        const float a = (d.z - d.x) * (d.w - d.y);
        for (int g = g0; g < g1; ++g) {
            if (gt_cls[g] != c) continue;
            const float4 t = *reinterpret_cast<const float4*>(gt_box + 4 * (size_t)g);
            const float w = fmaxf(fminf(d.z, t.z) - fmaxf(d.x, t.x), 0.0f), h = fmaxf(fminf(d.w, t.w) - fmaxf(d.y, t.y), 0.0f);
            const float inter = w * h;
            const float at = (t.z - t.x) * (t.w - t.y);
            const float iou = inter / ((a + at) - inter);
            if (iou == iou && (best < 0 || iou > biou)) best = g, biou = iou;     // NaN never beats a number; ties keep the lowest g
        }
    }
    best_gt[n] = best;
    best_iou[n] = biou;
    uint32_t b = __float_as_uint(det_score[n]);
    if (b == 0x80000000u) b = 0u;                                            // -0 and +0 tie
    const uint32_t m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);             // ascends with the float
    sort_key[n] = (long long)(((u64)(uint32_t)clampi(c, 0, C - 1) << 32) | (u64)(0xFFFFFFFFu - m));
}

__global__ __launch_bounds__(256) void det_init_kernel(uint32_t* __restrict__ winner, size_t n_winner, int32_t* __restrict__ n_easy,
                                                       int C, uint32_t* __restrict__ p11, size_t n_p11) {
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_winner; i += stride) winner[i] = 0xFFFFFFFFu;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n_p11; i += stride) p11[i] = 0u;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < (size_t)C; i += stride) n_easy[i] = 0;
}

__global__ __launch_bounds__(256) void det_n_easy_kernel(const int32_t* __restrict__ gt_cls, const uint8_t* __restrict__ difficult,
                                                         int G, int C, int32_t* __restrict__ n_easy) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= G) return;
    const int c = gt_cls[g];
    if (c >= 0 && c < C && !(difficult && difficult[g])) atomicAdd(n_easy + c, 1);
}

// tile_offset[c] = tiles before class c, c = 0..C: one workgroup, C <= 4096 = 4 per thread
__global__ __launch_bounds__(1024) void det_tile_offset_kernel(const int32_t* __restrict__ class_offset, int C, int N,
                                                               int32_t* __restrict__ tile_offset) {
    __shared__ int lds[16];
    int cnt[4], own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * (int)threadIdx.x + j;
        cnt[j] = 0;
        if (c < C) {
            const int s = clampi(class_offset[c], 0, N), e = clampi(class_offset[c + 1], s, N);
            cnt[j] = (e - s + TILE - 1) / TILE;
        }
        own += cnt[j];
    }
    int total;
    int run = block_scan_excl<16>(own, OpAdd(), 0, lds, total, false);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = 4 * (int)threadIdx.x + j;
        if (c < C) tile_offset[c] = run;
        run += cnt[j];
    }
    if (threadIdx.x == 0) tile_offset[C] = total;
}

__global__ __launch_bounds__(256) void det_winner_kernel(const int32_t* __restrict__ best_gt, const float* __restrict__ best_iou,
                                                         const int32_t* __restrict__ order, int N,
                                                         const uint8_t* __restrict__ difficult, int G, Thr thr,
                                                         uint32_t* __restrict__ winner) {
    const int r = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (r >= N) return;
    const int n = order[r];
    if ((unsigned)n >= (unsigned)N) return;
    const int b = best_gt[n];
    if ((unsigned)b >= (unsigned)G || !(best_iou[n] > thr.t[k]) || (difficult && difficult[b])) return;
    atomicMin(winner + (size_t)k * G + b, (uint32_t)r);
}

__global__ __launch_bounds__(256) void det_status_kernel(const int32_t* __restrict__ best_gt, const float* __restrict__ best_iou,
                                                         const int32_t* __restrict__ order, int N,
                                                         const uint8_t* __restrict__ difficult, int G, Thr thr,
                                                         const uint32_t* __restrict__ winner, uint8_t* __restrict__ status,
                                                         uint8_t* __restrict__ status_r) {
    const int r = blockIdx.x * 256 + threadIdx.x, k = blockIdx.y;
    if (r >= N) return;
    const int n = order[r];
    uint8_t st = ST_FP;
    if ((unsigned)n < (unsigned)N) {
        const int b = best_gt[n];
        if ((unsigned)b < (unsigned)G && best_iou[n] > thr.t[k])
            st = (difficult && difficult[b]) ? ST_IGNORED : (winner[(size_t)k * G + b] == (uint32_t)r ? ST_TP : ST_DUP);
        status[(size_t)k * N + n] = st;
    }
    status_r[(size_t)k * N + r] = st;
}

// the tile a workgroup works on: its class, first rank and number of ranks (count 0: no such tile)
struct TileAt {
    int c, r0, count;
};
__device__ __forceinline__ TileAt tile_at(int tile, const int32_t* __restrict__ class_offset,
                                          const int32_t* __restrict__ tile_offset, int C, int N) {
    TileAt t = {0, 0, 0};
    if (tile >= tile_offset[C]) return t;
    int lo = 0, hi = C;                                  // the last c with tile_offset[c] <= tile (empty classes share an offset)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (tile_offset[mid] <= tile) lo = mid;
        else hi = mid;
    }
    const int s = clampi(class_offset[lo], 0, N), e = clampi(class_offset[lo + 1], s, N);
    t.c = lo;
    t.r0 = s + (tile - tile_offset[lo]) * TILE;
    t.count = min(TILE, e - t.r0);
    if (t.count < 0) t.count = 0;
    return t;
}

__device__ __forceinline__ int tp_fp(uint8_t st) {        // TPs in the high half, FPs in the low half: a tile has <= 1024 of each
    return st == ST_TP ? (1 << 16) : ((st == ST_FP || st == ST_DUP) ? 1 : 0);
}

__global__ __launch_bounds__(256) void det_tile_sum_kernel(const uint8_t* __restrict__ status_r,
                                                           const int32_t* __restrict__ class_offset,
                                                           const int32_t* __restrict__ tile_offset, int C, int N, int NT,
                                                           u64* __restrict__ tsum) {
    const int tile = blockIdx.x, k = blockIdx.y;
    const TileAt t = tile_at(tile, class_offset, tile_offset, C, N);
    if (t.count == 0) return;
    const uint8_t* s = status_r + (size_t)k * N + t.r0;
    int v = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * (int)threadIdx.x + j;
        if (i < t.count) v += tp_fp(s[i]);
    }
    v = wave_sum_i32(v);
    __shared__ int part[4];
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int a = (part[0] + part[1]) + (part[2] + part[3]);
        tsum[(size_t)k * NT + tile] = ((u64)(uint32_t)(a >> 16) << 32) | (u64)(uint32_t)(a & 0xFFFF);
    }
}

// in place: a[k][0..nt) -> exclusive op-scan (forward), or exclusive suffix scan (reverse), TILE2 entries per step
template <class Op>
__global__ __launch_bounds__(1024) void det_tile_scan_kernel(u64* __restrict__ a, const int32_t* __restrict__ tile_offset, int C,
                                                             int NT, bool reverse) {
    __shared__ u64 lds[16];
    const int nt = clampi(tile_offset[C], 0, NT);
    u64* row = a + (size_t)blockIdx.x * NT;
    u64 carry = 0ull;
    Op op;
    for (int base = 0; base < nt; base += TILE2) {
        const int pos = base + (int)threadIdx.x;             // position in scan order; the reverse form walks the row backwards
        const int i = reverse ? nt - 1 - pos : pos;
        const bool live = pos < nt;
        const u64 v = live ? row[i] : 0ull;
        u64 total;
        const u64 ex = block_scan_excl<16>(v, op, 0ull, lds, total, false);
        if (live) row[i] = op(carry, ex);
        carry = op(carry, total);
    }
}

__global__ __launch_bounds__(256) void det_curve_kernel(const uint8_t* __restrict__ status_r, const int32_t* __restrict__ class_offset,
                                                        const int32_t* __restrict__ tile_offset, int C, int N, int NT,
                                                        const u64* __restrict__ tpre, const int32_t* __restrict__ n_easy, RecThr rt,
                                                        float* __restrict__ prec_ws, u64* __restrict__ tkey,
                                                        uint32_t* __restrict__ p11, int32_t* __restrict__ ctp_out,
                                                        int32_t* __restrict__ cfp_out, float* __restrict__ prec_out,
                                                        float* __restrict__ rec_out) {
    const int tile = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TileAt t = tile_at(tile, class_offset, tile_offset, C, N);
    if (t.count == 0) return;
    __shared__ int lds[4];
    __shared__ uint32_t red[4][12];
    const size_t row = (size_t)k * N + t.r0;
    int v[4], own = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * (int)threadIdx.x + j;
        v[j] = i < t.count ? tp_fp(status_r[row + i]) : 0;
        own += v[j];
    }
    int total;
    int run = block_scan_excl<4>(own, OpAdd(), 0, lds, total, false);
    const u64 pre = tpre[(size_t)k * NT + tile], cls0 = tpre[(size_t)k * NT + tile_offset[t.c]];
    const int tp0 = (int)(uint32_t)(pre >> 32) - (int)(uint32_t)(cls0 >> 32);
    const int fp0 = (int)(uint32_t)pre - (int)(uint32_t)cls0;
    const float ne = (float)n_easy[t.c];
    uint32_t pj[11], pmax = 0u;
#pragma unroll
    for (int j = 0; j < 11; ++j) pj[j] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * (int)threadIdx.x + j;
        run += v[j];
        if (i < t.count) {
            const int ctp = tp0 + (run >> 16), cfp = fp0 + (run & 0xFFFF);
            const float ft = (float)ctp, ff = (float)cfp;
            const float prec = ft / ((ft + ff) + 1e-10f), rec = ft / ne;
            const uint32_t pb = __float_as_uint(prec);
            prec_ws[row + i] = prec;
            if (ctp_out) ctp_out[row + i] = ctp;
            if (cfp_out) cfp_out[row + i] = cfp;
            if (prec_out) prec_out[row + i] = prec;
            if (rec_out) rec_out[row + i] = rec;
            pmax = pb > pmax ? pb : pmax;
#pragma unroll
            for (int q = 0; q < 11; ++q)
                if (rec >= rt.t[q]) pj[q] = pb > pj[q] ? pb : pj[q];
        }
    }
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        uint32_t m = q < 11 ? pj[q] : pmax;
#pragma unroll
        for (int s = 32; s >= 1; s >>= 1) {
            const uint32_t w = (uint32_t)__shfl_xor((int)m, s);
            m = w > m ? w : m;
        }
        if (lane == 0) red[wv][q] = m;
    }
    __syncthreads();
    if (threadIdx.x < 12) {
        const int q = threadIdx.x;
        const uint32_t a = red[0][q] > red[1][q] ? red[0][q] : red[1][q], b = red[2][q] > red[3][q] ? red[2][q] : red[3][q];
        const uint32_t m = a > b ? a : b;
        if (q < 11) {
            if (m) atomicMax(p11 + ((size_t)k * C + t.c) * 11 + q, m);
        } else {
            tkey[(size_t)k * NT + tile] = ((u64)(0xFFFFFFFFu - (uint32_t)t.c) << 32) | (u64)m;
        }
    }
}

__global__ __launch_bounds__(256) void det_env_kernel(const uint8_t* __restrict__ status_r, const float* __restrict__ prec_ws,
                                                      const int32_t* __restrict__ class_offset,
                                                      const int32_t* __restrict__ tile_offset, int C, int N, int NT,
                                                      const u64* __restrict__ tcarry, double* __restrict__ partial,
                                                      float* __restrict__ env_out) {
    const int tile = blockIdx.x, k = blockIdx.y, lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const TileAt t = tile_at(tile, class_offset, tile_offset, C, N);
    if (t.count == 0) return;
    __shared__ uint32_t lds[4];
    __shared__ double part[4];
    const size_t row = (size_t)k * N + t.r0;
    uint32_t p[4];
    bool tp[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * (int)threadIdx.x + j;
        p[j] = i < t.count ? __float_as_uint(prec_ws[row + i]) : 0u;
        tp[j] = i < t.count && status_r[row + i] == ST_TP;
    }
    p[2] = p[3] > p[2] ? p[3] : p[2];
    p[1] = p[2] > p[1] ? p[2] : p[1];
    p[0] = p[1] > p[0] ? p[1] : p[0];
    uint32_t total;
    uint32_t after = block_scan_excl<4>(p[0], OpMax(), 0u, lds, total, true);
    const u64 carry = tcarry[(size_t)k * NT + tile];
    if ((uint32_t)(carry >> 32) == 0xFFFFFFFFu - (uint32_t)t.c) after = (uint32_t)carry > after ? (uint32_t)carry : after;
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int i = 4 * (int)threadIdx.x + j;
        const uint32_t e = p[j] > after ? p[j] : after;
        if (env_out && i < t.count) env_out[row + i] = __uint_as_float(e);
        if (tp[j]) sum += (double)__uint_as_float(e);
    }
    sum = wave_sum_f64(sum);
    if (lane == 0) part[wv] = sum;
    __syncthreads();
    if (threadIdx.x == 0) partial[(size_t)k * NT + tile] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(256) void det_final_kernel(const int32_t* __restrict__ class_offset,
                                                        const int32_t* __restrict__ tile_offset, int C, int N, int NT,
                                                        const int32_t* __restrict__ n_easy, const double* __restrict__ partial,
                                                        const float* __restrict__ p11, float* __restrict__ ap11,
                                                        double* __restrict__ apa, float* __restrict__ map11,
                                                        double* __restrict__ mapa) {
    const int k = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        const float* p = p11 + ((size_t)k * C + c) * 11;
        float s = p[0];
        for (int j = 1; j < 11; ++j) s = s + p[j];
        ap11[(size_t)k * C + c] = s / 11.0f;
        double a = 0.0;
        const int ne = n_easy[c];
        if (N > 0 && ne > 0) {
            const int t0 = clampi(tile_offset[c], 0, NT), t1 = clampi(tile_offset[c + 1], t0, NT);
            for (int t = t0; t < t1; ++t) a += partial[(size_t)k * NT + t];
            a = a / (double)ne;
        }
        apa[(size_t)k * C + c] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        float s = 0.0f;
        double a = 0.0;
        for (int c = 0; c < C; ++c) s = s + ap11[(size_t)k * C + c], a += apa[(size_t)k * C + c];
        map11[k] = s / (float)C;
        mapa[k] = a / (double)C;
    }
}

inline size_t up8(size_t v) { return (v + 7) & ~(size_t)7; }

struct Layout {
    size_t winner, status_r, prec, tile_offset, tsum, tkey, partial, bytes;
    int NT;
};
inline Layout layout(int N, int G, int C, int T) {
    Layout L;
    L.NT = (N + TILE - 1) / TILE + C;
    size_t o = 0;
    L.winner = o, o += up8((size_t)T * G * 4);
    L.status_r = o, o += up8((size_t)T * N);
    L.prec = o, o += up8((size_t)T * N * 4);
    L.tile_offset = o, o += up8((size_t)(C + 1) * 4);
    L.tsum = o, o += (size_t)T * L.NT * 8;
    L.tkey = o, o += (size_t)T * L.NT * 8;
    L.partial = o, o += (size_t)T * L.NT * 8;
    L.bytes = o;
    return L;
}
inline bool sizes_ok(int N, int G, int C, int T) {
    return N >= 0 && N <= N_MAX && G >= 0 && G <= G_MAX && C >= 1 && C <= C_MAX && T >= 1 && T <= OSSID_DET_MAX_THRESHOLDS;
}

}  // namespace

extern "C" {

size_t ossid_det_eval_workspace_bytes(int N, int G, int C, int T) {
    return sizes_ok(N, G, C, T) ? layout(N, G, C, T).bytes : 0;
}

int ossid_det_claim(const float* det_box, const float* det_score, const int32_t* det_cls, const int32_t* det_image, int N,
                    const float* gt_box, const int32_t* gt_cls, const int32_t* gt_offset, int G, int I, int C, int32_t* best_gt,
                    float* best_iou, int64_t* sort_key, void* stream) {
    if (!sizes_ok(N, G, C, 1) || I < 1 || I > I_MAX || !gt_offset) return OSSID_EINVAL;
    if (N > 0 && (!det_box || !det_score || !det_cls || !det_image || !best_gt || !best_iou || !sort_key)) return OSSID_EINVAL;
    if (G > 0 && (!gt_box || !gt_cls)) return OSSID_EINVAL;
    if (((uintptr_t)det_box | (uintptr_t)gt_box) & 15) return OSSID_EINVAL;
    if (N == 0) return OSSID_OK;
    hipLaunchKernelGGL(det_claim_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, (hipStream_t)stream, det_box, det_score,
                       det_cls, det_image, N, gt_box, gt_cls, gt_offset, G, I, C, best_gt, best_iou, (long long*)sort_key);
    return ossid_launch_status();
}

int ossid_det_match(const int32_t* best_gt, const float* best_iou, const int32_t* order, const int32_t* class_offset, int N,
                    const int32_t* gt_cls, const uint8_t* gt_difficult, int G, int C, const float* iou_thr_host, int T,
                    void* workspace, size_t workspace_bytes, uint8_t* status, int32_t* n_easy, float* p11, float* ap11, double* apa,
                    float* map11, double* mapa, int32_t* ctp, int32_t* cfp, float* prec, float* rec, float* env, void* stream) {
    if (!sizes_ok(N, G, C, T) || !iou_thr_host || !class_offset || !n_easy || !p11 || !ap11 || !apa || !map11 || !mapa || !workspace ||
        ((uintptr_t)workspace & 7))
        return OSSID_EINVAL;
    if (N > 0 && (!best_gt || !best_iou || !order || !status)) return OSSID_EINVAL;
    if (G > 0 && !gt_cls) return OSSID_EINVAL;
    const Layout L = layout(N, G, C, T);
    if (workspace_bytes < L.bytes) return OSSID_EINVAL;
    Thr thr = {};
    for (int k = 0; k < T; ++k) {
        if (!std::isfinite(iou_thr_host[k])) return OSSID_EINVAL;
        thr.t[k] = iou_thr_host[k];
    }
    RecThr rt;
    for (int j = 0; j < 11; ++j) rt.t[j] = (float)((double)j * 0.1);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    uint32_t* winner = (uint32_t*)(ws + L.winner);
    uint8_t* status_r = (uint8_t*)(ws + L.status_r);
    float* prec_ws = (float*)(ws + L.prec);
    int32_t* tile_offset = (int32_t*)(ws + L.tile_offset);
    u64 *tsum = (u64*)(ws + L.tsum), *tkey = (u64*)(ws + L.tkey);
    double* partial = (double*)(ws + L.partial);
    const size_t n_winner = (size_t)T * G, n_p11 = (size_t)T * C * 11;
    const size_t most = n_winner > n_p11 ? n_winner : n_p11;
    hipLaunchKernelGGL(det_init_kernel, dim3((unsigned)((most + 255) / 256 < 2048 ? (most + 255) / 256 : 2048)), dim3(256), 0, s, winner,
                       n_winner, n_easy, C, (uint32_t*)p11, n_p11);
    if (G > 0)
        hipLaunchKernelGGL(det_n_easy_kernel, dim3((unsigned)((G + 255) / 256)), dim3(256), 0, s, gt_cls, gt_difficult, G, C, n_easy);
    hipLaunchKernelGGL(det_tile_offset_kernel, dim3(1), dim3(1024), 0, s, class_offset, C, N, tile_offset);
    if (N > 0) {
        const dim3 flat((unsigned)((N + 255) / 256), (unsigned)T), tiles((unsigned)L.NT, (unsigned)T);
        if (G > 0)
            hipLaunchKernelGGL(det_winner_kernel, flat, dim3(256), 0, s, best_gt, best_iou, order, N, gt_difficult, G, thr, winner);
        hipLaunchKernelGGL(det_status_kernel, flat, dim3(256), 0, s, best_gt, best_iou, order, N, gt_difficult, G, thr, winner, status,
                           status_r);
        hipLaunchKernelGGL(det_tile_sum_kernel, tiles, dim3(256), 0, s, status_r, class_offset, tile_offset, C, N, L.NT, tsum);
        hipLaunchKernelGGL(det_tile_scan_kernel<OpAdd>, dim3((unsigned)T), dim3(1024), 0, s, tsum, tile_offset, C, L.NT, false);
        hipLaunchKernelGGL(det_curve_kernel, tiles, dim3(256), 0, s, status_r, class_offset, tile_offset, C, N, L.NT, tsum, n_easy, rt,
                           prec_ws, tkey, (uint32_t*)p11, ctp, cfp, prec, rec);
        hipLaunchKernelGGL(det_tile_scan_kernel<OpMax>, dim3((unsigned)T), dim3(1024), 0, s, tkey, tile_offset, C, L.NT, true);
        hipLaunchKernelGGL(det_env_kernel, tiles, dim3(256), 0, s, status_r, prec_ws, class_offset, tile_offset, C, N, L.NT, tkey, partial,
                           env);
    }
    hipLaunchKernelGGL(det_final_kernel, dim3((unsigned)T), dim3(256), 0, s, class_offset, tile_offset, C, N, L.NT, n_easy, partial, p11,
                       ap11, apa, map11, mapa);
    return ossid_launch_status();
}

}  // extern "C"
