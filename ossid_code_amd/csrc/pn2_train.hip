// PointNet2SSG in TRAINING mode: forward with batch-statistics BatchNorm and dropout, and the backward pass to every
// parameter (SPEC.md 12). Stands behind zephyr.models.pointnet2.PointNet2SSG (scripts/online_learning.py:212-227 builds and
// loads it) and restates pointnet2_ops' PointnetSAModule / SharedMLP / the classification head in torch's channel order
// (xyz first). The inference kernels (csrc/pn2.hip) are separate and untouched; sampling and grouping indices come from
// the same ossid_pn2_fps / ossid_pn2_ball_query.
//
// Everything is a chain of a few generic kernels over row-major f32 matrices [rows][channels]:
//   group      gather [xyz_i - centre, features, 0-pad] rows
//   gemm       D = A . B on v_mfma_f32_32x32x2_f32 (exact f32 products, eight interleaved fmaf chains per output), any strides;
//              the forward (X W^T), the data gradient (dZ W) and the weight gradient (dZ^T X, split over rows) are three
//              stride settings of it
//   colstats   per-channel sums in f64 over row chunks, combined in chunk order
//   bn_relu / bn_relu_pool, bn_bwd_reduce / bn_bwd_apply, ungroup, dropout, bias
// No float atomics: every reduction has a fixed order, so two runs give the same bits.
// What is kept: every pre-activation Z and every inner activation A. The backward pass works IN PLACE: dZ overwrites Z and
// dA overwrites A, so one forward supports one backward.
#include "common.h"
#include "mfma.h"

namespace {

constexpr int NBN = 11;
constexpr int BN_C[NBN] = {64, 64, 128, 128, 128, 256, 256, 512, 1024, 512, 256};
constexpr int STAT_TOTAL = 3328;
constexpr float BN_EPS = 1e-5f, BN_MOMENTUM = 0.1f;
constexpr int STAT_MAX_CHUNKS = 256;

// ---- gemm -----------------------------------------------------------------------------------------------------------------
// D[z][m][n] = sum over k in split z of A(m,k) * B(k,n), A(m,k) = A[m*sam + k*sak], B(k,n) = B[k*sbk + n*sbn]; out-of-range
// operands read as zero. A workgroup (4 waves) makes a 64 x 64 tile, each wave a 32 x 32 quarter, from 16-deep slices in LDS.
struct Gemm {
    const float* A;
    long sam, sak;
    const float* B;
    long sbk, sbn;
    float* D;
    long ldd, dsplit;
    int M, N, K, kchunk;
};

__global__ __launch_bounds__(256) void gemm_kernel(Gemm g) {
    __shared__ float As[16][65], Bs[16][65];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 31, h = lane >> 5;
    const int wm = wave >> 1, wn = wave & 1;
    const long m0 = (long)blockIdx.x * 64, n0 = (long)blockIdx.y * 64;
    const int k0 = blockIdx.z * g.kchunk, k1 = min(g.K, k0 + g.kchunk);
    const bool a_kfast = g.sak == 1, b_kfast = g.sbk == 1;
    // NACC interleaved chains: 16-deep slice s of the split goes to accumulator s % NACC, and the accumulators are added in
    // order at the end. One chain over a long reduction (1024 and more) rounds worse than a blocked f32 GEMM does.
    constexpr int NACC = 8;
    v16f accs[NACC];
#pragma unroll
    for (int j = 0; j < NACC; ++j)
#pragma unroll
        for (int i = 0; i < 16; ++i) accs[j][i] = 0.0f;
    for (int kb0 = k0; kb0 < k1; kb0 += 16 * NACC) {
#pragma unroll
        for (int j = 0; j < NACC; ++j) {
            const int kb = kb0 + 16 * j;
            if (kb >= k1) break;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int e = tid + 256 * i;
                {
                    const int kk = a_kfast ? (e & 15) : (e >> 6), mm = a_kfast ? (e >> 4) : (e & 63);
                    const long gm = m0 + mm, gk = kb + kk;
                    As[kk][mm] = (gm < g.M && gk < k1) ? g.A[gm * g.sam + gk * g.sak] : 0.0f;
                }
                {
                    const int kk = b_kfast ? (e & 15) : (e >> 6), nn = b_kfast ? (e >> 4) : (e & 63);
                    const long gn = n0 + nn, gk = kb + kk;
                    Bs[kk][nn] = (gn < g.N && gk < k1) ? g.B[gk * g.sbk + gn * g.sbn] : 0.0f;
                }
            }
            __syncthreads();
#pragma unroll
            for (int kk = 0; kk < 8; ++kk) accs[j] = mfma(As[2 * kk + h][wm * 32 + c], Bs[2 * kk + h][wn * 32 + c], accs[j]);
            __syncthreads();
        }
    }
    v16f acc = accs[0];
#pragma unroll
    for (int j = 1; j < NACC; ++j) acc += accs[j];
    float* D = g.D + (long)blockIdx.z * g.dsplit;
    const long col = n0 + wn * 32 + c;
    if (col < g.N) {
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const long row = m0 + wm * 32 + 8 * q + 4 * h + e;
                if (row < g.M) D[row * g.ldd + col] = acc[4 * q + e];
            }
    }
}

// out[i] = part[0][i] + part[1][i] + ... in split order
__global__ __launch_bounds__(256) void combine_kernel(const float* __restrict__ part, long n, int splits, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float s = part[i];
    for (int z = 1; z < splits; ++z) s += part[(long)z * n + i];
    out[i] = s;
}

int launch_gemm(Gemm g, int splits, hipStream_t s) {
    if (g.M <= 0 || g.N <= 0) return OSSID_OK;
    const long gx = ((long)g.M + 63) / 64, gy = ((long)g.N + 63) / 64;
    if (gx > 0x7fffffffL || gy > 65535 || splits > 65535) return OSSID_EINVAL;
    hipLaunchKernelGGL(gemm_kernel, dim3((unsigned)gx, (unsigned)gy, splits), dim3(256), 0, s, g);
    return ossid_launch_status();
}

int linear_fwd(const float* X, long R, int Kp, const float* W, int Kr, int C, float* Z, hipStream_t s) {
    Gemm g{X, Kp, 1, W, 1, Kr, Z, C, 0, (int)R, C, Kr, Kr};
    return launch_gemm(g, 1, s);
}

// dX[R][N] = dZ[R][C] . W[C][ldw] columns 0..N (the caller offsets W to choose them)
int linear_dgrad(const float* dZ, long R, int C, const float* W, int ldw, int N, float* dX, hipStream_t s) {
    Gemm g{dZ, C, 1, W, ldw, 1, dX, N, 0, (int)R, N, C, C};
    return launch_gemm(g, 1, s);
}

// rows per split of the weight gradient: at least 512, at most 256 splits
void wgrad_split(long R, int* chunk, int* splits) {
    long ch = (R + 255) / 256;
    if (ch < 512) ch = 512;
    ch = (ch + 15) / 16 * 16;
    *chunk = (int)ch;
    *splits = (int)((R + ch - 1) / ch);
    if (*splits < 1) *splits = 1;
}

size_t wgrad_ws_bytes(long R, int C, int Kr) {
    int chunk, splits;
    wgrad_split(R, &chunk, &splits);
    return splits > 1 ? (size_t)splits * C * Kr * sizeof(float) : 0;
}

// dW[C][Kr] = dZ[R][C]^T . X[R][Kp] columns 0..Kr
int linear_wgrad(const float* dZ, long R, int C, const float* X, int Kp, int Kr, float* dW, float* ws, hipStream_t s) {
    int chunk, splits;
    wgrad_split(R, &chunk, &splits);
    Gemm g{dZ, 1, C, X, Kp, 1, splits > 1 ? ws : dW, Kr, (long)C * Kr, C, Kr, (int)R, chunk};
    int rc = launch_gemm(g, splits, s);
    if (rc != OSSID_OK || splits == 1) return rc;
    const long n = (long)C * Kr;
    hipLaunchKernelGGL(combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, ws, n, splits, dW);
    return ossid_launch_status();
}

// ---- group ----------------------------------------------------------------------------------------------------------------
// X[r][0..3) = xyz[idx] - centre, X[r][3..3+Cf) = feat[idx], X[r][3+Cf..Kp) = 0; r = (b, j, s), rows_per_batch = npoint * S.
// idx NULL: the row's own point (S = 1); centre NULL: nothing subtracted (SA3 concatenates only).
__global__ __launch_bounds__(256) void group_kernel(const float* __restrict__ xyz, int xs, const float* __restrict__ feat, int fs,
                                                    int Cf, const float* __restrict__ centre, const int* __restrict__ idx, int n,
                                                    int S, long rows_per_batch, long R, int Kp, float* __restrict__ X) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * Kp) return;
    const long r = i / Kp;
    const int k = (int)(i - r * Kp);
    const long b = r / rows_per_batch;
    const long src = b * n + (idx ? idx[r] : (r - b * rows_per_batch));
    float v = 0.0f;
    if (k < 3) {
        v = xyz[src * xs + k];
        if (centre) v = v - centre[(r / S) * 3 + k];
    } else if (k < 3 + Cf) {
        v = feat[src * fs + (k - 3)];
    }
    X[i] = v;
}

// ---- BatchNorm statistics -------------------------------------------------------------------------------------------------
// part[chunk][c] = (sum z, sum z^2) in f64 over the chunk's rows; a block covers 64 channels with 4 row lanes.
__global__ __launch_bounds__(256) void colstats_kernel(const float* __restrict__ Z, long R, int C, long rpc, double* __restrict__ part) {
    __shared__ double sh[4][64][2];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx;
    const long r0 = (long)blockIdx.y * rpc, r1 = min(R, r0 + rpc);
    double s1 = 0.0, s2 = 0.0;
    if (c < C)
        for (long r = r0 + ty; r < r1; r += 4) {
            const double z = (double)Z[r * C + c];
            s1 += z;
            s2 += z * z;
        }
    sh[ty][tx][0] = s1;
    sh[ty][tx][1] = s2;
    __syncthreads();
    if (ty == 0 && c < C) {
        for (int j = 1; j < 4; ++j) {
            s1 += sh[j][tx][0];
            s2 += sh[j][tx][1];
        }
        part[((long)blockIdx.y * C + c) * 2 + 0] = s1;
        part[((long)blockIdx.y * C + c) * 2 + 1] = s2;
    }
}

// mean, 1/sqrt(biased var + eps); running statistics as torch updates them (momentum 0.1, unbiased variance)
__global__ __launch_bounds__(256) void stats_finalize_kernel(const double* __restrict__ part, int nchunk, long R, int C,
                                                             float* __restrict__ mu, float* __restrict__ rs,
                                                             float* __restrict__ var_out, float* __restrict__ run_mean,
                                                             float* __restrict__ run_var) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < nchunk; ++j) {
        s1 += part[((long)j * C + c) * 2 + 0];
        s2 += part[((long)j * C + c) * 2 + 1];
    }
    const double mean = s1 / (double)R;
    double var = s2 / (double)R - mean * mean;
    if (var < 0.0) var = 0.0;
    mu[c] = (float)mean;
    rs[c] = (float)(1.0 / sqrt(var + (double)BN_EPS));
    if (var_out) var_out[c] = (float)var;
    if (run_mean) run_mean[c] = (1.0f - BN_MOMENTUM) * run_mean[c] + BN_MOMENTUM * (float)mean;
    if (run_var) {
        const float unbiased = (float)(var * ((double)R / (double)(R - 1)));
        run_var[c] = (1.0f - BN_MOMENTUM) * run_var[c] + BN_MOMENTUM * unbiased;
    }
}

void stat_chunks(long R, int* nchunk, long* rpc) {
    long n = (R + 255) / 256;
    if (n < 1) n = 1;
    if (n > STAT_MAX_CHUNKS) n = STAT_MAX_CHUNKS;
    *rpc = (R + n - 1) / n;
    *nchunk = (int)((R + *rpc - 1) / *rpc);
}

int bn_stats(const float* Z, long R, int C, double* part, float* mu, float* rs, float* var_out, float* run_mean,
             float* run_var, hipStream_t s) {
    int nchunk;
    long rpc;
    stat_chunks(R, &nchunk, &rpc);
    hipLaunchKernelGGL(colstats_kernel, dim3((C + 63) / 64, nchunk), dim3(256), 0, s, Z, R, C, rpc, part);
    hipLaunchKernelGGL(stats_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, nchunk, R, C, mu, rs, var_out,
                       run_mean, run_var);
    return ossid_launch_status();
}

// the one statement of the normalisation: forward and backward both call it, so the ReLU decision recomputed in the
// backward pass is the forward's
__device__ __forceinline__ float bn_hat(float z, float mu, float rs) { return (z - mu) * rs; }
__device__ __forceinline__ float bn_out(float zh, float g, float b) { return zh * g + b; }

__global__ __launch_bounds__(256) void bn_relu_kernel(const float* __restrict__ Z, long n, int C, const float* __restrict__ mu,
                                                      const float* __restrict__ rs, const float* __restrict__ gamma,
                                                      const float* __restrict__ beta, float* __restrict__ A,
                                                      uint8_t* __restrict__ mask) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int c = (int)(i % C);
    const float y = bn_out(bn_hat(Z[i], mu[c], rs[c]), gamma[c], beta[c]);
    const bool on = y > 0.0f;
    A[i] = on ? y : 0.0f;
    if (mask) mask[i] = on;
}

// out[g][c] = max over the group's S rows of relu(bn(z)), the FIRST maximum in row order; arg = its row within the group
__global__ __launch_bounds__(256) void bn_relu_pool_kernel(const float* __restrict__ Z, long G, int S, int C,
                                                           const float* __restrict__ mu, const float* __restrict__ rs,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           float* __restrict__ out, int* __restrict__ arg,
                                                           uint8_t* __restrict__ mask, int* __restrict__ dbg_arg) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= G * C) return;
    const long g = i / C;
    const int c = (int)(i - g * C);
    const float m = mu[c], r = rs[c], ga = gamma[c], be = beta[c];
    float best = 0.0f;
    int bi = 0;
    for (int s = 0; s < S; ++s) {
        const long at = (g * S + s) * C + c;
        const float y = bn_out(bn_hat(Z[at], m, r), ga, be);
        const bool on = y > 0.0f;
        const float a = on ? y : 0.0f;
        if (mask) mask[at] = on;
        if (s == 0 || a > best) {
            best = a;
            bi = s;
        }
    }
    out[i] = best;
    arg[i] = bi;
    if (dbg_arg) dbg_arg[i] = bi;
}

// ---- BatchNorm backward ---------------------------------------------------------------------------------------------------
// the gradient arriving at relu(bn(z)) of element (r, c): a dense matrix dA, or a pooled gradient routed to the argmax row
struct DySrc {
    const float* dA;
    const float* dpool;
    const int* arg;
    int S;
};
__device__ __forceinline__ float dy_at(const DySrc& d, long r, int c, int C, float y) {
    if (!(y > 0.0f)) return 0.0f;
    if (d.dA) return d.dA[r * C + c];
    const long g = r / d.S;
    const int s = (int)(r - g * d.S);
    return d.arg[g * C + c] == s ? d.dpool[g * C + c] : 0.0f;
}

__global__ __launch_bounds__(256) void bn_bwd_reduce_kernel(const float* __restrict__ Z, long R, int C, long rpc, DySrc d,
                                                            const float* __restrict__ mu, const float* __restrict__ rs,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            double* __restrict__ part) {
    __shared__ double sh[4][64][2];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6, c = blockIdx.x * 64 + tx;
    const long r0 = (long)blockIdx.y * rpc, r1 = min(R, r0 + rpc);
    double s1 = 0.0, s2 = 0.0;
    if (c < C) {
        const float m = mu[c], r_ = rs[c], ga = gamma[c], be = beta[c];
        for (long r = r0 + ty; r < r1; r += 4) {
            const float zh = bn_hat(Z[r * C + c], m, r_);
            const float dy = dy_at(d, r, c, C, bn_out(zh, ga, be));
            s1 += (double)dy;
            s2 += (double)dy * (double)zh;
        }
    }
    sh[ty][tx][0] = s1;
    sh[ty][tx][1] = s2;
    __syncthreads();
    if (ty == 0 && c < C) {
        for (int j = 1; j < 4; ++j) {
            s1 += sh[j][tx][0];
            s2 += sh[j][tx][1];
        }
        part[((long)blockIdx.y * C + c) * 2 + 0] = s1;
        part[((long)blockIdx.y * C + c) * 2 + 1] = s2;
    }
}

// dbeta = sum dy, dgamma = sum dy * zhat; coef = (mean dy, mean dy * zhat)
__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const double* __restrict__ part, int nchunk, long R, int C,
                                                              float* __restrict__ dgamma, float* __restrict__ dbeta,
                                                              float* __restrict__ coef) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= C) return;
    double s1 = 0.0, s2 = 0.0;
    for (int j = 0; j < nchunk; ++j) {
        s1 += part[((long)j * C + c) * 2 + 0];
        s2 += part[((long)j * C + c) * 2 + 1];
    }
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
    coef[2 * c + 0] = (float)(s1 / (double)R);
    coef[2 * c + 1] = (float)(s2 / (double)R);
}

// dZ = gamma * rs * (dy - mean dy - zhat * mean(dy zhat)), written over Z
__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(float* __restrict__ Z, long R, int C, DySrc d,
                                                           const float* __restrict__ mu, const float* __restrict__ rs,
                                                           const float* __restrict__ gamma, const float* __restrict__ beta,
                                                           const float* __restrict__ coef) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= R * C) return;
    const long r = i / C;
    const int c = (int)(i - r * C);
    const float zh = bn_hat(Z[i], mu[c], rs[c]);
    const float dy = dy_at(d, r, c, C, bn_out(zh, gamma[c], beta[c]));
    Z[i] = (gamma[c] * rs[c]) * ((dy - coef[2 * c]) - zh * coef[2 * c + 1]);
}

int bn_bwd(float* Z, long R, int C, DySrc d, const float* mu, const float* rs, const float* gamma, const float* beta,
           double* part, float* coef, float* dgamma, float* dbeta, hipStream_t s) {
    int nchunk;
    long rpc;
    stat_chunks(R, &nchunk, &rpc);
    hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3((C + 63) / 64, nchunk), dim3(256), 0, s, Z, R, C, rpc, d, mu, rs, gamma, beta,
                       part);
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((C + 255) / 256), dim3(256), 0, s, part, nchunk, R, C, dgamma, dbeta, coef);
    const long n = R * C;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, Z, R, C, d, mu, rs, gamma, beta,
                       coef);
    return ossid_launch_status();
}

// ---- ungroup --------------------------------------------------------------------------------------------------------------
// out[b][i][c] = sum of dG[b][e][c] over the entries e (ascending) with idx[b][e] == i: the scatter-add of the grouping
// written as a gather, one wave per target point; the wave scans the index list 64 entries at a time and adds the matching
// rows in entry order.
__global__ __launch_bounds__(256) void ungroup_kernel(const float* __restrict__ dG, const int* __restrict__ idx, int E, int n,
                                                      int Cf, float* __restrict__ out) {
    const int lane = threadIdx.x & 63, b = blockIdx.y;
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= n) return;
    const int* ib = idx + (long)b * E;
    const float* gb = dG + (long)b * E * Cf;
    for (int c0 = 0; c0 < Cf; c0 += 256) {
        float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        for (int e0 = 0; e0 < E; e0 += 64) {
            const int e = e0 + lane;
            unsigned long long hit = __ballot(e < E && ib[e] == i);
            while (hit) {
                const int bit = __ffsll((long long)hit) - 1;
                hit &= hit - 1;
                const float* row = gb + (long)(e0 + bit) * Cf;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int c = c0 + lane + 64 * j;
                    if (c < Cf) acc[j] += row[c];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + lane + 64 * j;
            if (c < Cf) out[((long)b * n + i) * Cf + c] = acc[j];
        }
    }
}

int ungroup(const float* dG, const int* idx, int B, int E, int n, int Cf, float* out, hipStream_t s) {
    hipLaunchKernelGGL(ungroup_kernel, dim3((n + 3) / 4, B), dim3(256), 0, s, dG, idx, E, n, Cf, out);
    return ossid_launch_status();
}

// ---- head pieces ----------------------------------------------------------------------------------------------------------
// out = in * keep * scale (the forward's dropout and, on the gradient, its backward)
__global__ __launch_bounds__(256) void dropout_kernel(const float* __restrict__ in, const uint8_t* __restrict__ keep, float scale,
                                                      long n, float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = keep[i] ? in[i] * scale : 0.0f;
}

__global__ __launch_bounds__(256) void add_bias_kernel(float* __restrict__ y, int n, const float* __restrict__ bias) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = y[i] + bias[0];
}

// one thread: the sum in row order, accumulated in f64 and rounded once, as the column sums are (an f32 accumulator is
// 1.4 x 2^-24 off at 17 rows where the rounded f64 sum is 0.07 x 2^-24 off)
__global__ void sum_kernel(const float* __restrict__ x, int n, float* __restrict__ out) {
    if (blockIdx.x || threadIdx.x) return;
    double s = 0.0;
    for (int i = 0; i < n; ++i) s += (double)x[i];
    out[0] = (float)s;
}

__global__ __launch_bounds__(256) void copy_u8_kernel(const uint8_t* __restrict__ in, long n, uint8_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = in[i];
}

// ---- workspace ------------------------------------------------------------------------------------------------------------
struct Layer {
    long R;
    int Kp, Kr, C;
    float *X, *Z, *A;   // input rows, pre-activation (later dZ), activation (later dA); A NULL for a pooled layer
    int stat;           // offset into mu / rs
};

struct Plan {
    int B, M, np1, np2;
    int *fps1, *ball1, *fps2, *ball2, *arg[3];
    float *xyz1, *xyz2, *feat[3], *dfeat[3];
    float *A10d, *mu, *rs, *coef, *wpart;
    double* spart;
    uint8_t* keep;
    Layer L[NBN];
    size_t bytes;
};

Plan carve(char* base, int B, int M, int np1, int np2) {
    Plan p{};
    p.B = B, p.M = M, p.np1 = np1, p.np2 = np2;
    size_t off = 0;
    auto take = [&](size_t nbytes) {
        char* q = base ? base + off : nullptr;
        off += (nbytes + 255) / 256 * 256;
        return q;
    };
    auto f32 = [&](long n) { return (float*)take((size_t)n * 4); };
    auto i32 = [&](long n) { return (int*)take((size_t)n * 4); };
    const long G1 = (long)B * np1, R1 = G1 * 64, R3 = (long)B * np2, R2 = R3 * 64;
    p.fps1 = i32(G1), p.xyz1 = f32(G1 * 3), p.ball1 = i32(R1);
    p.fps2 = i32(R3), p.xyz2 = f32(R3 * 3), p.ball2 = i32(R2);
    const long rows[NBN] = {R1, R1, R1, R2, R2, R2, R3, R3, R3, B, B};
    const int kr[NBN] = {8, 64, 64, 131, 128, 128, 259, 256, 512, 1024, 512};
    int stat = 0;
    for (int l = 0; l < NBN; ++l) {
        Layer& L = p.L[l];
        L.R = rows[l], L.Kr = kr[l], L.Kp = (kr[l] + 7) / 8 * 8, L.C = BN_C[l], L.stat = stat;
        stat += L.C;
        const bool first = l % 3 == 0 && l < 9, pooled = l % 3 == 2 && l < 9;
        L.X = first ? f32(L.R * L.Kp) : (l == 9 ? nullptr : p.L[l - 1].A);
        L.Z = f32(L.R * L.C);
        L.A = pooled ? nullptr : f32(L.R * L.C);
        if (pooled) {
            const int m = l / 3;
            const long g = m == 0 ? G1 : (m == 1 ? R3 : B);
            p.feat[m] = f32(g * L.C), p.dfeat[m] = f32(g * L.C), p.arg[m] = i32(g * L.C);
        }
    }
    p.L[9].X = p.feat[2];
    p.A10d = f32((long)B * 256);
    p.keep = (uint8_t*)take((size_t)B * 256);
    p.mu = f32(STAT_TOTAL), p.rs = f32(STAT_TOTAL), p.coef = f32(2 * 1024);
    p.spart = (double*)take((size_t)STAT_MAX_CHUNKS * 1024 * 2 * sizeof(double));
    size_t wp = wgrad_ws_bytes(B, 1, 256);
    for (int l = 0; l < NBN; ++l) {
        const size_t w = wgrad_ws_bytes(p.L[l].R, p.L[l].C, p.L[l].Kr);
        if (w > wp) wp = w;
    }
    p.wpart = (float*)take(wp);
    p.bytes = off;
    return p;
}

bool bad_shape(int B, int M, int np1, int np2) {
    return B < 2 || np1 <= 0 || np2 <= 0 || np1 % 32 || np2 % 32 || M < np1 || np1 < np2 ||
           (long)B * np1 * 64 > 0x7fffffffL;        // row counts are ints in the kernels' arguments
}

#define PN2T_TRY(expr)                 \
    do {                               \
        const int rc_ = (expr);        \
        if (rc_ != OSSID_OK) return rc_; \
    } while (0)

inline unsigned blocks(long n) { return (unsigned)((n + 255) / 256); }

}  // namespace

extern "C" {

size_t ossid_pn2_train_workspace_bytes(int B, int M, int npoint1, int npoint2) {
    if (bad_shape(B, M, npoint1, npoint2)) return 0;
    return carve(nullptr, B, M, npoint1, npoint2).bytes;
}

int ossid_pn2_train_forward(const float* point_x, int B, int M, const ossid_pn2_train_params* w, const uint8_t* keep_mask,
                            float p_drop, void* workspace, size_t workspace_bytes, float* scores,
                            const ossid_pn2_train_dbg* dbg, void* stream) {
    if (!w || bad_shape(B, M, w->npoint1, w->npoint2)) return OSSID_EINVAL;
    if (!point_x || !keep_mask || !workspace || !scores || !(p_drop >= 0.0f && p_drop < 1.0f)) return OSSID_EINVAL;
    if (((uintptr_t)workspace & 255) != 0) return OSSID_EINVAL;
    const Plan p = carve((char*)workspace, B, M, w->npoint1, w->npoint2);
    if (workspace_bytes < p.bytes) return OSSID_EINVAL;
    for (int l = 0; l < 12; ++l)
        if (!w->w[l] || (l < NBN && (!w->gamma[l] || !w->beta[l]))) return OSSID_EINVAL;
    if (!w->bias) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int np1 = p.np1, np2 = p.np2;

    PN2T_TRY(ossid_pn2_fps(point_x, 8, B, M, np1, p.fps1, p.xyz1, stream));
    PN2T_TRY(ossid_pn2_ball_query(point_x, 8, B, M, p.xyz1, np1, w->radius1, 64, p.ball1, stream));
    PN2T_TRY(ossid_pn2_fps(p.xyz1, 3, B, np1, np2, p.fps2, p.xyz2, stream));
    PN2T_TRY(ossid_pn2_ball_query(p.xyz1, 3, B, np1, p.xyz2, np2, w->radius2, 64, p.ball2, stream));

    for (int l = 0; l < NBN; ++l) {
        const Layer& L = p.L[l];
        if (l == 0)
            hipLaunchKernelGGL(group_kernel, dim3(blocks(L.R * L.Kp)), dim3(256), 0, s, point_x, 8, point_x + 3, 8, 5, p.xyz1,
                               p.ball1, M, 64, (long)np1 * 64, L.R, L.Kp, L.X);
        else if (l == 3)
            hipLaunchKernelGGL(group_kernel, dim3(blocks(L.R * L.Kp)), dim3(256), 0, s, p.xyz1, 3, p.feat[0], 128, 128, p.xyz2,
                               p.ball2, np1, 64, (long)np2 * 64, L.R, L.Kp, L.X);
        else if (l == 6)
            hipLaunchKernelGGL(group_kernel, dim3(blocks(L.R * L.Kp)), dim3(256), 0, s, p.xyz2, 3, p.feat[1], 256, 256,
                               (const float*)nullptr, (const int*)nullptr, np2, 1, (long)np2, L.R, L.Kp, L.X);
        PN2T_TRY(linear_fwd(L.X, L.R, L.Kp, w->w[l], L.Kr, L.C, L.Z, s));
        PN2T_TRY(bn_stats(L.Z, L.R, L.C, p.spart, p.mu + L.stat, p.rs + L.stat, nullptr, w->run_mean[l], w->run_var[l], s));
        uint8_t* mask = dbg ? dbg->relu[l] : nullptr;
        if (L.A) {
            hipLaunchKernelGGL(bn_relu_kernel, dim3(blocks(L.R * L.C)), dim3(256), 0, s, L.Z, L.R * L.C, L.C, p.mu + L.stat,
                               p.rs + L.stat, w->gamma[l], w->beta[l], L.A, mask);
        } else {
            const int m = l / 3, S = m == 2 ? np2 : 64;
            const long G = L.R / S;
            hipLaunchKernelGGL(bn_relu_pool_kernel, dim3(blocks(G * L.C)), dim3(256), 0, s, L.Z, G, S, L.C, p.mu + L.stat,
                               p.rs + L.stat, w->gamma[l], w->beta[l], p.feat[m], p.arg[m], mask,
                               dbg ? dbg->argmax[m] : (int*)nullptr);
        }
    }
    const long nd = (long)B * 256;
    hipLaunchKernelGGL(copy_u8_kernel, dim3(blocks(nd)), dim3(256), 0, s, keep_mask, nd, p.keep);
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks(nd)), dim3(256), 0, s, p.L[10].A, keep_mask, 1.0f / (1.0f - p_drop), nd,
                       p.A10d);
    PN2T_TRY(linear_fwd(p.A10d, B, 256, w->w[11], 256, 1, scores, s));
    hipLaunchKernelGGL(add_bias_kernel, dim3(blocks(B)), dim3(256), 0, s, scores, B, w->bias);
    if (dbg) {
        const struct {
            int* dst;
            const int* src;
            long n;
        } cp[4] = {{dbg->fps1, p.fps1, (long)B * np1}, {dbg->ball1, p.ball1, (long)B * np1 * 64},
                   {dbg->fps2, p.fps2, (long)B * np2}, {dbg->ball2, p.ball2, (long)B * np2 * 64}};
        for (int i = 0; i < 4; ++i)
            if (cp[i].dst && hipMemcpyAsync(cp[i].dst, cp[i].src, cp[i].n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess)
                return OSSID_ELAUNCH;
    }
    return ossid_launch_status();
}

int ossid_pn2_train_backward(const float* dscores, int B, int M, const ossid_pn2_train_params* w, float p_drop,
                             void* workspace, size_t workspace_bytes, const ossid_pn2_train_grads* g, void* stream) {
    if (!w || !g || bad_shape(B, M, w->npoint1, w->npoint2)) return OSSID_EINVAL;
    if (!dscores || !workspace || !(p_drop >= 0.0f && p_drop < 1.0f)) return OSSID_EINVAL;
    if (((uintptr_t)workspace & 255) != 0) return OSSID_EINVAL;
    const Plan p = carve((char*)workspace, B, M, w->npoint1, w->npoint2);
    if (workspace_bytes < p.bytes) return OSSID_EINVAL;
    for (int l = 0; l < 12; ++l)
        if (!w->w[l] || !g->w[l] || (l < NBN && (!w->gamma[l] || !w->beta[l] || !g->gamma[l] || !g->beta[l]))) return OSSID_EINVAL;
    if (!g->bias) return OSSID_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const int np1 = p.np1, np2 = p.np2;

    // last linear layer and dropout
    hipLaunchKernelGGL(sum_kernel, dim3(1), dim3(64), 0, s, dscores, B, g->bias);
    PN2T_TRY(linear_wgrad(dscores, B, 1, p.A10d, 256, 256, g->w[11], p.wpart, s));
    PN2T_TRY(linear_dgrad(dscores, B, 1, w->w[11], 256, 256, p.A10d, s));
    const long nd = (long)B * 256;
    hipLaunchKernelGGL(dropout_kernel, dim3(blocks(nd)), dim3(256), 0, s, p.A10d, p.keep, 1.0f / (1.0f - p_drop), nd, p.L[10].A);

    for (int l = NBN - 1; l >= 0; --l) {
        const Layer& L = p.L[l];
        DySrc d{};
        if (L.A) {
            d.dA = L.A;
        } else {
            const int m = l / 3;
            d.dpool = p.dfeat[m], d.arg = p.arg[m], d.S = m == 2 ? np2 : 64;
        }
        PN2T_TRY(bn_bwd(L.Z, L.R, L.C, d, p.mu + L.stat, p.rs + L.stat, w->gamma[l], w->beta[l], p.spart, p.coef, g->gamma[l],
                        g->beta[l], s));
        PN2T_TRY(linear_wgrad(L.Z, L.R, L.C, L.X, L.Kp, L.Kr, g->w[l], p.wpart, s));
        if (l == 0) break;
        if (l == 9) {
            PN2T_TRY(linear_dgrad(L.Z, L.R, L.C, w->w[l], L.Kr, L.Kr, p.dfeat[2], s));
        } else if (l == 6) {       // feature columns only: the gradient of feat2, row for row
            PN2T_TRY(linear_dgrad(L.Z, L.R, L.C, w->w[l] + 3, L.Kr, 256, p.dfeat[1], s));
        } else if (l == 3) {       // feature columns into the grouped input's buffer, then the scatter-add through ball2
            PN2T_TRY(linear_dgrad(L.Z, L.R, L.C, w->w[l] + 3, L.Kr, 128, L.X, s));
            PN2T_TRY(ungroup(L.X, p.ball2, B, np2 * 64, np1, 128, p.dfeat[0], s));
        } else {
            PN2T_TRY(linear_dgrad(L.Z, L.R, L.C, w->w[l], L.Kr, L.Kr, p.L[l - 1].A, s));
        }
    }
    return ossid_launch_status();
}

/* ---- stage entry points (tests/test_pn2_train_gpu.py holds each against float64) ---- */
int ossid_pn2_train_linear_fwd(const float* X, int R, int Kp, const float* W, int Kr, int C, float* Z, void* stream) {
    if (!X || !W || !Z || R <= 0 || C <= 0 || Kr <= 0 || Kp < Kr) return OSSID_EINVAL;
    return linear_fwd(X, R, Kp, W, Kr, C, Z, (hipStream_t)stream);
}

int ossid_pn2_train_linear_dgrad(const float* dZ, int R, int C, const float* W, int ldw, int N, float* dX, void* stream) {
    if (!dZ || !W || !dX || R <= 0 || C <= 0 || N <= 0 || ldw < N) return OSSID_EINVAL;
    return linear_dgrad(dZ, R, C, W, ldw, N, dX, (hipStream_t)stream);
}

size_t ossid_pn2_train_wgrad_workspace_bytes(int R, int C, int Kr) {
    if (R <= 0 || C <= 0 || Kr <= 0) return 0;
    return wgrad_ws_bytes(R, C, Kr) + 256;
}

int ossid_pn2_train_linear_wgrad(const float* dZ, int R, int C, const float* X, int Kp, int Kr, float* dW, void* workspace,
                                 size_t workspace_bytes, void* stream) {
    if (!dZ || !X || !dW || R <= 0 || C <= 0 || Kr <= 0 || Kp < Kr) return OSSID_EINVAL;
    if (!workspace || workspace_bytes < wgrad_ws_bytes(R, C, Kr) + 256 || ((uintptr_t)workspace & 255)) return OSSID_EINVAL;
    return linear_wgrad(dZ, R, C, X, Kp, Kr, dW, (float*)workspace, (hipStream_t)stream);
}

int ossid_pn2_train_ungroup(const float* dG, const int32_t* idx, int B, int E, int n, int Cf, float* out, void* stream) {
    if (!dG || !idx || !out || B <= 0 || E <= 0 || n <= 0 || Cf <= 0) return OSSID_EINVAL;
    return ungroup(dG, idx, B, E, n, Cf, out, (hipStream_t)stream);
}

size_t ossid_pn2_train_bn_stats_workspace_bytes(void) { return (size_t)STAT_MAX_CHUNKS * 1024 * 2 * sizeof(double); }

int ossid_pn2_train_bn_stats(const float* Z, int R, int C, void* workspace, size_t workspace_bytes, float* mean,
                             float* rstd, float* var, void* stream) {
    if (!Z || !mean || !rstd || R <= 0 || C <= 0 || C > 1024) return OSSID_EINVAL;
    if (!workspace || workspace_bytes < ossid_pn2_train_bn_stats_workspace_bytes() || ((uintptr_t)workspace & 255)) return OSSID_EINVAL;
    return bn_stats(Z, R, C, (double*)workspace, mean, rstd, var, nullptr, nullptr, (hipStream_t)stream);
}

int ossid_pn2_train_bn_relu_pool(const float* Z, int G, int S, int C, const float* mean, const float* rstd,
                                 const float* gamma, const float* beta, float* out, int32_t* argmax, void* stream) {
    if (!Z || !mean || !rstd || !gamma || !beta || !out || !argmax || G <= 0 || S <= 0 || C <= 0) return OSSID_EINVAL;
    hipLaunchKernelGGL(bn_relu_pool_kernel, dim3(blocks((long)G * C)), dim3(256), 0, (hipStream_t)stream, Z, (long)G, S, C, mean,
                       rstd, gamma, beta, out, argmax, (uint8_t*)nullptr, (int*)nullptr);
    return ossid_launch_status();
}

}  // extern "C"
