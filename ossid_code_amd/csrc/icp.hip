// Point-to-point ICP refinement of a pose against the depth pixels its model points project to (SPEC.md section 5), the
// step between the scorer and the renderer: scripts/online_learning.py:471-480 (zephyr.utils.icp.icpRefinement).
//
// One workgroup per pose, every iteration inside the one launch:
//   stage   target cloud Q from the uv row (depth2xyz of pipeline.hip), a uniform grid over Q's bounding box in LDS
//           (counting sort: LDS atomics count, a workgroup scan, LDS atomics place), the model points in registers;
//   iterate correspondences by probing the 27 cells around each source -- nearest by (d2, Q index), so the order inside
//           a cell does not matter and the result equals SPEC 5's brute force --, f64 moments per thread in a fixed order,
//           a fixed-shape reduction (no global atomics: bit-reproducible), one lane solves Horn's quaternion
//           eigenproblem (the Kabsch optimum over SO(3), det R = +1) and publishes the new pose through LDS.
// Every output is written by the kernel (no memset).
#include <float.h>
#include <limits.h>

#include <cmath>

#include "cell_grid.h"
#include "workgroup.h"

namespace {

constexpr int NT = 512;                     // threads per workgroup (8 waves; 1024 spills at the 128-VGPR cap)
constexpr int PPT = OSSID_ICP_MAX_POINTS / NT;  // model points / target candidates per thread
constexpr int NW = NT / 64;
constexpr int MAX_CELLS = 4096;
constexpr int NMOM = 17;                    // count, sum d2, sum s (3), sum q (3), sum s q^T (9)
static_assert(OSSID_ICP_MAX_POINTS % NT == 0, "points per thread");

struct IcpShared {
    float4 q[OSSID_ICP_MAX_POINTS];         // Q sorted by cell: x, y, z, Q order key (j) as bits
    int cell[MAX_CELLS];                    // counts -> starts -> ends of each cell
    double red[NW][NMOM];
    double pose[16], mom[NMOM];
    float bb[NW][6];
    int wsum[NW];
    CellGrid grid;
    int go;
};

// the grid's storage for cell_probe: cell[c] = END of cell c, sorted points in LDS
struct IcpCells {
    const IcpShared& sh;
    __device__ __forceinline__ void run(int first, int last, int& b, int& e) const {
        b = first == 0 ? 0 : sh.cell[first - 1], e = sh.cell[last];
    }
    __device__ __forceinline__ float4 point(int p) const { return sh.q[p]; }
};

// One Jacobi rotation of the symmetric 4x4 A (row-major) in the (p, q) plane, accumulated into V. Called with constant
// p, q from fully unrolled loops, so A and V stay in registers.
__device__ __forceinline__ void jacobi_rotate(double (&A)[16], double (&V)[16], int p, int q) {
    const double apq = A[4 * p + q];
    if (apq == 0.0) return;
    const double theta = (A[5 * q] - A[5 * p]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
#pragma unroll
    for (int k = 0; k < 4; ++k) {              // A <- A J
        const double akp = A[4 * k + p], akq = A[4 * k + q];
        A[4 * k + p] = c * akp - s * akq;
        A[4 * k + q] = s * akp + c * akq;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {              // A <- J^T A
        const double apk = A[4 * p + k], aqk = A[4 * q + k];
        A[4 * p + k] = c * apk - s * aqk;
        A[4 * q + k] = s * apk + c * aqk;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {              // V <- V J
        const double vkp = V[4 * k + p], vkq = V[4 * k + q];
        V[4 * k + p] = c * vkp - s * vkq;
        V[4 * k + q] = s * vkp + c * vkq;
    }
}

// Cyclic Jacobi sweeps on the symmetric 4x4 A (in place) until the off-diagonal part is negligible -> the unit
// eigenvector (w, x, y, z) of the largest eigenvalue.
__device__ void max_eigvec4(double (&A)[16], double (&v)[4]) {
    double V[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) V[i] = (i % 5) == 0 ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 24; ++sweep) {
        double off = 0.0, dia = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            dia += A[5 * i] * A[5 * i];
#pragma unroll
            for (int j = i + 1; j < 4; ++j) off += A[4 * i + j] * A[4 * i + j];
        }
        if (!(off > 1e-36 * dia)) break;
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int q = p + 1; q < 4; ++q) jacobi_rotate(A, V, p, q);
    }
    double best = A[0];
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = V[4 * i];
#pragma unroll
    for (int b = 1; b < 4; ++b)
        if (A[5 * b] > best) {
            best = A[5 * b];
#pragma unroll
            for (int i = 0; i < 4; ++i) v[i] = V[4 * i + b];
        }
}

// pose <- dT * pose, dT the best rigid fit q ~ R s + t of the moments mom (taken about the origin c0); run by one lane,
// pose and mom in LDS, the solve in registers.
__device__ void icp_update(double* pose, const double* mom, const float* lo) {
    const double n = mom[0];
    const double c0[3] = {(double)lo[0], (double)lo[1], (double)lo[2]};
    const double ms[3] = {mom[2] / n, mom[3] / n, mom[4] / n}, mq[3] = {mom[5] / n, mom[6] / n, mom[7] / n};
    // S[a][b] = sum (s-ms)_a (q-mq)_b = sum s_a q_b - (sum s_a) mq_b
#define S_(a, b) (mom[8 + 3 * (a) + (b)] - mom[2 + (a)] * mq[(b)])
    const double Sxx = S_(0, 0), Sxy = S_(0, 1), Sxz = S_(0, 2), Syx = S_(1, 0), Syy = S_(1, 1), Syz = S_(1, 2),
                 Szx = S_(2, 0), Szy = S_(2, 1), Szz = S_(2, 2);
#undef S_
    // Horn's N: its top eigenvector is the unit quaternion (w, x, y, z) of the rotation maximising sum q . R s
    double A[16] = {Sxx + Syy + Szz, Syz - Szy,        Szx - Sxz,         Sxy - Syx,
                    Syz - Szy,       Sxx - Syy - Szz,  Sxy + Syx,         Szx + Sxz,
                    Szx - Sxz,       Sxy + Syx,        -Sxx + Syy - Szz,  Syz + Szy,
                    Sxy - Syx,       Szx + Sxz,        Syz + Szy,         -Sxx - Syy + Szz};
    double qv[4];
    max_eigvec4(A, qv);
    const double inv = 1.0 / sqrt(((qv[0] * qv[0] + qv[1] * qv[1]) + qv[2] * qv[2]) + qv[3] * qv[3]);
    const double w = qv[0] * inv, x = qv[1] * inv, y = qv[2] * inv, z = qv[3] * inv;
    const double R[9] = {w * w + x * x - y * y - z * z, 2.0 * (x * y - w * z), 2.0 * (x * z + w * y),
                         2.0 * (y * x + w * z), w * w - x * x + y * y - z * z, 2.0 * (y * z - w * x),
                         2.0 * (z * x - w * y), 2.0 * (z * y + w * x), w * w - x * x - y * y + z * z};
    double t[3];
#pragma unroll
    for (int a = 0; a < 3; ++a)                         // t = (mq + c0) - R (ms + c0)
        t[a] = (mq[a] + c0[a]) - ((R[3 * a] * (ms[0] + c0[0]) + R[3 * a + 1] * (ms[1] + c0[1])) +
                                  R[3 * a + 2] * (ms[2] + c0[2]));
    double P[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = pose[i];
#pragma unroll
    for (int c = 0; c < 4; ++c)                         // pose <- [R t] pose
#pragma unroll
        for (int a = 0; a < 3; ++a)
            pose[4 * a + c] = ((R[3 * a] * P[c] + R[3 * a + 1] * P[4 + c]) + R[3 * a + 2] * P[8 + c]) + (c == 3 ? t[a] : 0.0);
}

__global__ __launch_bounds__(NT) void icp_refine_kernel(const float* __restrict__ depth, int H, int W,
                                                        const int32_t* __restrict__ uv, const double* __restrict__ poses_in,
                                                        const float* __restrict__ points, int M, float fx, float fy,
                                                        float cx, float cy, float max_dist, int max_iter,
                                                        double* __restrict__ poses_out, double* __restrict__ fitness,
                                                        double* __restrict__ rmse, int32_t* __restrict__ iterations) {
    __shared__ IcpShared sh;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const size_t k = blockIdx.x;
    if (tid < 16) sh.pose[tid] = poses_in[k * 16 + tid];

    // ---- stage: target candidates j = tid + NT*i (validity, back-projection), model points -------------------------
    float qx[PPT], qy[PPT], qz[PPT], px[PPT], py[PPT], pz[PPT];
    bool qok[PPT];
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        const int j = tid + NT * i;
        qok[i] = false;
        qx[i] = qy[i] = qz[i] = 0.0f;
        px[i] = py[i] = pz[i] = 0.0f;
        if (j < M) {
            px[i] = points[3 * j], py[i] = points[3 * j + 1], pz[i] = points[3 * j + 2];
            const int x = uv[(k * M + j) * 2], y = uv[(k * M + j) * 2 + 1];
            if (x >= 0 && x < W && y >= 0 && y < H) {
                const float z = depth[(size_t)y * W + x];
                if (z > 0.0f) {
                    qx[i] = ((float)x - cx) * z / fx;
                    qy[i] = ((float)y - cy) * z / fy;
                    qz[i] = z;
                    // a non-finite target is at infinite / NaN distance from every source: SPEC 5 never pairs it
                    qok[i] = isfinite(qx[i]) && isfinite(qy[i]) && isfinite(qz[i]);
                }
            }
        }
        if (qok[i]) {
            mn[0] = fminf(mn[0], qx[i]), mn[1] = fminf(mn[1], qy[i]), mn[2] = fminf(mn[2], qz[i]);
            mx[0] = fmaxf(mx[0], qx[i]), mx[1] = fmaxf(mx[1], qy[i]), mx[2] = fmaxf(mx[2], qz[i]);
        }
    }
    wg_bbox3<NW>(mn, mx, sh.bb);
    if (tid == 0) {
        if (!(mn[0] <= mx[0]))                         // empty Q: a one-cell grid that nothing lands in
            for (int a = 0; a < 3; ++a) mn[a] = mx[a] = 0.0f;
        sh.grid = cell_grid_size(mn, mx, max_dist, MAX_CELLS);
    }
    __syncthreads();
    const CellGrid G = sh.grid;
    const int ncell = G.n[0] * G.n[1] * G.n[2];

    // ---- grid: count, scan, place --------------------------------------------------------------------------------
    for (int c = tid; c < ncell; c += NT) sh.cell[c] = 0;
    __syncthreads();
    int qc[PPT];
#pragma unroll
    for (int i = 0; i < PPT; ++i) {
        qc[i] = cell_of(G, qx[i], qy[i], qz[i]);
        if (qok[i]) atomicAdd(&sh.cell[qc[i]], 1);
    }
    __syncthreads();
    {   // exclusive scan of the counts: MAX_CELLS / NT consecutive cells per thread
        constexpr int CPT = MAX_CELLS / NT;
        int v[CPT], s = 0;
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int c = tid * CPT + i;
            v[i] = c < ncell ? sh.cell[c] : 0;
            s += v[i];
        }
        int total;
        int base = block_scan_excl<NW>(s, OpAdd(), 0, sh.wsum, total, false);
#pragma unroll
        for (int i = 0; i < CPT; ++i) {
            const int c = tid * CPT + i;
            if (c < ncell) sh.cell[c] = base;
            base += v[i];
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PPT; ++i)
        if (qok[i]) {
            const int pos = atomicAdd(&sh.cell[qc[i]], 1);          // afterwards cell[c] = end of cell c
            sh.q[pos] = make_float4(qx[i], qy[i], qz[i], __int_as_float(tid + NT * i));
        }
    __syncthreads();

    // ---- iterate ---------------------------------------------------------------------------------------------------
    const float md2 = max_dist * max_dist;
    const double c0[3] = {(double)G.lo[0], (double)G.lo[1], (double)G.lo[2]};   // moments are taken about Q's box corner
    double prev_fit = 0.0, prev_rmse = 0.0;
    int it = 0;
    for (;;) {
        float T[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) T[i] = (float)sh.pose[i];
        double mom[NMOM];
#pragma unroll
        for (int i = 0; i < NMOM; ++i) mom[i] = 0.0;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            if (tid + NT * i >= M) continue;
            const float sx = ((T[0] * px[i] + T[1] * py[i]) + T[2] * pz[i]) + T[3];
            const float sy = ((T[4] * px[i] + T[5] * py[i]) + T[6] * pz[i]) + T[7];
            const float sz = ((T[8] * px[i] + T[9] * py[i]) + T[10] * pz[i]) + T[11];
            const CellHit hit = cell_probe(G, IcpCells{sh}, sx, sy, sz, INFINITY);
            if (hit.j != INT_MAX && hit.d2 <= md2) {
                const float4 bq = sh.q[hit.pos];
                const double s[3] = {(double)sx - c0[0], (double)sy - c0[1], (double)sz - c0[2]};
                const double q[3] = {(double)bq.x - c0[0], (double)bq.y - c0[1], (double)bq.z - c0[2]};
                mom[0] += 1.0;
                mom[1] += (double)hit.d2;
#pragma unroll
                for (int a = 0; a < 3; ++a) mom[2 + a] += s[a], mom[5 + a] += q[a];
#pragma unroll
                for (int a = 0; a < 3; ++a)
#pragma unroll
                    for (int b2 = 0; b2 < 3; ++b2) mom[8 + 3 * a + b2] += s[a] * q[b2];
            }
        }
#pragma unroll
        for (int i = 0; i < NMOM; ++i) mom[i] = wave_sum_f64(mom[i]);
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < NMOM; ++i) sh.red[wv][i] = mom[i];
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < NMOM; ++i) {
                double v = sh.red[0][i];
                for (int w = 1; w < NW; ++w) v += sh.red[w][i];
                sh.mom[i] = v;
            }
            const double n = sh.mom[0];
            const double fit = n / (double)M, rm = n > 0.0 ? sqrt(sh.mom[1] / n) : 0.0;
            const bool conv = it > 0 && fabs(fit - prev_fit) < 1e-6 && fabs(rm - prev_rmse) < 1e-6;
            prev_fit = fit, prev_rmse = rm;
            if (conv || it >= max_iter || n < 3.0) {
                for (int i = 0; i < 16; ++i) poses_out[k * 16 + i] = sh.pose[i];
                fitness[k] = fit;
                rmse[k] = rm;
                iterations[k] = it;
                sh.go = 0;
            } else {
                icp_update(sh.pose, sh.mom, sh.grid.lo);
                ++it;
                sh.go = 1;
            }
        }
        __syncthreads();
        if (!sh.go) break;
    }
}

}  // namespace

extern "C" {

int ossid_icp_refine(const float* depth, int H, int W, const int32_t* uv, const double* poses_in, const float* points, int K,
                     int M, float fx, float fy, float cx, float cy, float max_dist, int max_iter, double* poses_out,
                     double* fitness, double* rmse, int32_t* iterations, void* stream) {
    if (!depth || !uv || !poses_in || !points || !poses_out || !fitness || !rmse || !iterations) return OSSID_EINVAL;
    if (H <= 0 || W <= 0 || K <= 0 || M <= 0 || M > OSSID_ICP_MAX_POINTS || max_iter < 0) return OSSID_EINVAL;
    if (!(max_dist > 0.0f) || !std::isfinite(max_dist) || !(fx != 0.0f) || !(fy != 0.0f) || !std::isfinite(fx) ||
        !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy))
        return OSSID_EINVAL;
    hipLaunchKernelGGL(icp_refine_kernel, dim3(K), dim3(NT), 0, (hipStream_t)stream, depth, H, W, uv, poses_in, points, M, fx,
                       fy, cx, cy, max_dist, max_iter, poses_out, fitness, rmse, iterations);
    return ossid_launch_status();
}

}  // extern "C"
