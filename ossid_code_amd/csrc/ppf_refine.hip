// Dense pose refinement of PPF hypotheses against the scene (SPEC.md 6.9): point-to-plane Gauss-Newton, scene -> model
// correspondences, what Halcon's find_surface_model does by default (DensePoseRefinement 'true') after its clustering.
//
//   model grid   once per model: for each distinct distance threshold of the step schedule a uniform grid over the
//                refinement model points in the model frame (counting sort in global memory by one workgroup per level);
//                the cell edge follows cell_grid.h's exactness argument, so the 27-cell probe keeping the lexicographic
//                minimum of (d2, model index) equals SPEC 6.9's brute force for every pair it accepts.
//   per frame    one launch chain, the hypothesis count stays on the device (info[0] of ossid_ppf_cluster):
//                init (pose copies, f32 inverses), then per step one workgroup per (hypothesis, chunk of 1024 scene
//                points) writing 27 f64 moments and a pair count, and one thread per hypothesis summing the chunks in
//                order, solving by Cholesky and updating the pose; a last pass counts pairs at the final pose and one
//                workgroup sorts by score. No atomics on values that are summed: results are bit-reproducible, and a
//                hypothesis refined alone equals its row in a batch.
// No output is cleared with a memset: every output and every workspace word a kernel reads is written by a kernel.
#include <float.h>
#include <math.h>

#include "cell_grid.h"
#include "workgroup.h"

namespace {

constexpr int RNT = 256;                     // correspondence workgroup
constexpr int RPT = 4;                       // scene points per thread
constexpr int RCH = RNT * RPT;               // scene points per chunk
constexpr int NMOM = 27;                     // A upper triangle (21), g (6)
constexpr int NPART = NMOM + 1;              // + pair count
constexpr int MAX_CELLS = 32768;             // per level
constexpr int MAX_LEVELS = 16;
constexpr int MAX_STEPS = 16;
constexpr int MAX_RESULTS = 4096;            // sort in LDS
constexpr int GNT = 1024;                    // grid build workgroup

struct Level {
    CellGrid g;
    int ncell;
};

struct GridHeader {                          // at the start of the grid buffer, written by the setup kernel
    Level lev[MAX_LEVELS];
};

// grid buffer: header | model points float4 [Mr] | normals float4 [Mr] | per level: start int [MAX_CELLS + 1],
// cursor int [MAX_CELLS], sorted float4 [Mr] (x, y, z, model index as bits)
__host__ __device__ constexpr size_t align16(size_t b) { return (b + 15) & ~(size_t)15; }
size_t level_bytes(int Mr) { return align16((size_t)(2 * MAX_CELLS + 1) * 4) + (size_t)Mr * 16; }
__host__ __device__ constexpr size_t header_bytes() { return align16(sizeof(GridHeader)); }
size_t grid_bytes(int Mr, int nlev) { return header_bytes() + (size_t)Mr * 32 + (size_t)nlev * level_bytes(Mr); }

struct GridView {
    const GridHeader* hdr;
    const float4* pts;
    const float4* nrm;
    const char* levels;
    size_t lbytes;
    int Mr;
    __device__ __forceinline__ const int* start(int l) const { return (const int*)(levels + l * lbytes); }
    __device__ __forceinline__ const float4* sorted(int l) const {
        return (const float4*)(levels + l * lbytes + align16((size_t)(2 * MAX_CELLS + 1) * 4));
    }
};

GridView grid_view(const void* g, int Mr, int nlev) {
    const char* b = (const char*)g;
    GridView v;
    v.hdr = (const GridHeader*)b;
    v.pts = (const float4*)(b + header_bytes());
    v.nrm = v.pts + Mr;
    v.levels = b + header_bytes() + (size_t)Mr * 32;
    v.lbytes = level_bytes(Mr);
    v.Mr = Mr;
    (void)nlev;
    return v;
}

// SPEC 6.9: thr_k = f32(max(0.1 * 2^-k * D, 2 * h_r)) in f64; the first k at which the floor applies ends the distinct
// thresholds, every later step uses that level's grid.
double thr_f64(int k, float D, float h) { return fmax(0.1 * ldexp(1.0, -k) * (double)D, 2.0 * (double)h); }
int floor_step(float D, float h) {
    int k = 0;
    while (k + 1 < MAX_LEVELS && 0.1 * ldexp(1.0, -k) * (double)D > 2.0 * (double)h) ++k;
    return k;
}
int n_levels(int steps, float D, float h) { return min(steps, floor_step(D, h) + 1); }
int level_of(int k, float D, float h) { return min(k, floor_step(D, h)); }

bool args_ok(int Mr, int steps, float D, float h) {
    return Mr > 0 && Mr <= OSSID_PPF_MAX_REFINE_MODEL_POINTS && steps >= 1 && steps <= MAX_STEPS && D > 0.0f && isfinite(D) &&
           h > 0.0f && isfinite(h);
}

// ---- model grid ---------------------------------------------------------------------------------------------------------
struct Thr {
    float t[MAX_LEVELS];
};

// one workgroup: bounds of the model points, every level's grid (cell_grid_size), float4 copies of the points and normals
__global__ __launch_bounds__(GNT) void refine_grid_setup_kernel(const float* __restrict__ P, const float* __restrict__ N, int Mr,
                                                                int nlev, Thr thr, void* __restrict__ grid) {
    __shared__ float red[GNT / 64][6];
    GridHeader* hdr = (GridHeader*)grid;
    float4* pts = (float4*)((char*)grid + header_bytes());
    float4* nrm = pts + Mr;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int i = threadIdx.x; i < Mr; i += GNT) {
        const float x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        pts[i] = make_float4(x, y, z, 0.0f);
        nrm[i] = make_float4(N[3 * i], N[3 * i + 1], N[3 * i + 2], 0.0f);
        mn[0] = fminf(mn[0], x), mn[1] = fminf(mn[1], y), mn[2] = fminf(mn[2], z);
        mx[0] = fmaxf(mx[0], x), mx[1] = fmaxf(mx[1], y), mx[2] = fmaxf(mx[2], z);
    }
    wg_bbox3<GNT / 64>(mn, mx, red);
    if (threadIdx.x >= nlev) return;                    // nlev <= MAX_LEVELS: wave 0
    Level& L = hdr->lev[threadIdx.x];
    L.g = cell_grid_size(mn, mx, thr.t[threadIdx.x], MAX_CELLS);
    L.ncell = L.g.n[0] * L.g.n[1] * L.g.n[2];
}

// one workgroup per level: counting sort of the model points into the level's cells (order inside a cell is free: the
// probe takes the lexicographic minimum of (d2, index))
__global__ __launch_bounds__(GNT) void refine_grid_sort_kernel(int Mr, void* __restrict__ grid, size_t lbytes) {
    __shared__ int wsum[GNT / 64];
    const GridHeader* hdr = (const GridHeader*)grid;
    const float4* pts = (const float4*)((const char*)grid + header_bytes());
    char* lv = (char*)grid + header_bytes() + (size_t)Mr * 32 + blockIdx.x * lbytes;
    int* start = (int*)lv;
    int* cursor = start + MAX_CELLS + 1;
    float4* sorted = (float4*)(lv + align16((size_t)(2 * MAX_CELLS + 1) * 4));
    const Level L = hdr->lev[blockIdx.x];
    for (int c = threadIdx.x; c < L.ncell; c += GNT) cursor[c] = 0;
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < Mr; i += GNT) {
        const float4 p = pts[i];
        atomicAdd(&cursor[cell_of(L.g, p.x, p.y, p.z)], 1);
    }
    __threadfence();
    __syncthreads();
    wg_scan_range<GNT / 64>(cursor, L.ncell, wsum, [&](int c, int base) { start[c] = base, cursor[c] = base; });
    if (threadIdx.x == 0) start[L.ncell] = Mr;
    __threadfence();
    __syncthreads();
    for (int i = threadIdx.x; i < Mr; i += GNT) {
        const float4 p = pts[i];
        const int pos = atomicAdd(&cursor[cell_of(L.g, p.x, p.y, p.z)], 1);
        sorted[pos] = make_float4(p.x, p.y, p.z, __int_as_float(i));
    }
}

// ---- per frame ----------------------------------------------------------------------------------------------------------
struct Work {                                // carved out of the caller's workspace
    double* pose;                            // [NR][16] current pose
    float* inv;                              // [NR][12] f32 (R^T | -R^T t), row-major 3 x 4
    int* active;                             // [NR] 1 while steps remain
    int* done;                               // [NR] updates applied
    double* part;                            // [NR][nch][NPART]
};

Work carve(void* ws, int NR, int nch) {
    char* b = (char*)ws;
    Work w;
    w.pose = (double*)b;
    b += align16((size_t)NR * 16 * 8);
    w.inv = (float*)b;
    b += align16((size_t)NR * 12 * 4);
    w.active = (int*)b;
    b += align16((size_t)NR * 4);
    w.done = (int*)b;
    b += align16((size_t)NR * 4);
    w.part = (double*)b;
    return w;
}

size_t work_bytes(int NR, int nch) {
    return align16((size_t)NR * 16 * 8) + align16((size_t)NR * 12 * 4) + 2 * align16((size_t)NR * 4) +
           (size_t)NR * nch * NPART * 8;
}

// nh null: every row is a pose (ossid_ppf_refine_match)
__device__ __forceinline__ int n_hyp(const int32_t* nh, int NR) { return nh ? min(max(nh[0], 0), NR) : NR; }
__device__ __forceinline__ bool scene_ok(const int32_t* count, int cap) { return count[0] >= 0 && count[0] <= cap; }

// R^T and -R^T t in f64, cast to f32
__device__ __forceinline__ void write_inverse(const double* T, float* inv) {
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const double r0 = T[j], r1 = T[4 + j], r2 = T[8 + j];          // row j of R^T = column j of R
        inv[4 * j] = (float)r0, inv[4 * j + 1] = (float)r1, inv[4 * j + 2] = (float)r2;
        inv[4 * j + 3] = (float)(-((r0 * T[3] + r1 * T[7]) + r2 * T[11]));
    }
}

__global__ __launch_bounds__(256) void refine_init_kernel(const double* __restrict__ poses_in, const int32_t* __restrict__ nh,
                                                          const int32_t* __restrict__ count, int cap, int NR, Work w,
                                                          int32_t* __restrict__ status) {
    const int h = blockIdx.x * 256 + threadIdx.x;
    const int n = n_hyp(nh, NR);
    const bool sok = scene_ok(count, cap);
    if (h == 0 && status) status[0] = sok ? 0 : 1, status[1] = count[0], status[2] = n, status[3] = 0;
    if (h >= NR) return;
    double T[16];
    for (int q = 0; q < 16; ++q) T[q] = h < n ? poses_in[16 * (size_t)h + q] : 0.0;
    for (int q = 0; q < 16; ++q) w.pose[16 * (size_t)h + q] = T[q];
    write_inverse(T, w.inv + 12 * (size_t)h);
    w.active[h] = (h < n && sok) ? 1 : 0;
    w.done[h] = 0;
}

// a level's storage for cell_probe: start[c] = first position of cell c (start[ncell] = Mr), sorted points in global memory
struct LevelCells {
    const int* start;
    const float4* srt;
    __device__ __forceinline__ void run(int first, int last, int& b, int& e) const { b = start[first], e = start[last + 1]; }
    __device__ __forceinline__ float4 point(int p) const { return srt[p]; }
};

// nearest refinement model point of x within the level's grid, ties to the lowest index -> index (or -1 when none
// within thr2)
__device__ __forceinline__ int probe(const GridView& g, int lev, const float* x, float thr2) {
    const CellHit h = cell_probe(g.hdr->lev[lev].g, LevelCells{g.start(lev), g.sorted(lev)}, x[0], x[1], x[2], FLT_MAX);
    return (h.j != INT_MAX && h.d2 <= thr2) ? h.j : -1;
}

// MODE 0: moments of one step for active hypotheses; 1: pair count at the final pose for every hypothesis; 2: the
// matched model index of every scene point (the correspondence set, for tests)
template <int MODE>
__global__ __launch_bounds__(RNT) void refine_corr_kernel(const float* __restrict__ S, const int32_t* __restrict__ count, int cap,
                                                          GridView g, int lev, float thr2, const int32_t* __restrict__ nh,
                                                          int NR, int nch_max, Work w, int32_t* __restrict__ match) {
    __shared__ double red[RNT / 64][NPART];
    const int c = blockIdx.x, h = blockIdx.y;
    if (!scene_ok(count, cap) || h >= n_hyp(nh, NR)) return;
    if (MODE == 0 && !w.active[h]) return;
    const int ns = count[0];
    if (c * RCH >= ns) return;
    const float* iv = w.inv + 12 * (size_t)h;
    float Ri[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) Ri[q] = iv[q];
    double acc[NMOM];
#pragma unroll
    for (int q = 0; q < NMOM; ++q) acc[q] = 0.0;
    int pairs = 0;
    for (int p = 0; p < RPT; ++p) {
        const int i = c * RCH + p * RNT + threadIdx.x;
        if (i >= ns) break;
        const float s0 = S[3 * i], s1 = S[3 * i + 1], s2 = S[3 * i + 2];
        float x[3];
#pragma unroll
        for (int j = 0; j < 3; ++j) x[j] = ((Ri[4 * j] * s0 + Ri[4 * j + 1] * s1) + Ri[4 * j + 2] * s2) + Ri[4 * j + 3];
        const int j = probe(g, lev, x, thr2);
        if (MODE == 2) {
            match[(size_t)h * cap + i] = j;
            continue;
        }
        if (j < 0) continue;
        ++pairs;
        if (MODE == 1) continue;
        const float4 m4 = g.pts[j], n4 = g.nrm[j];
        const double X0 = x[0], X1 = x[1], X2 = x[2], n0 = n4.x, n1 = n4.y, n2 = n4.z;
        const double J[6] = {X1 * n2 - X2 * n1, X2 * n0 - X0 * n2, X0 * n1 - X1 * n0, n0, n1, n2};
        const double r = (n0 * (X0 - (double)m4.x) + n1 * (X1 - (double)m4.y)) + n2 * (X2 - (double)m4.z);
        int q = 0;
#pragma unroll
        for (int a = 0; a < 6; ++a)
#pragma unroll
            for (int b = a; b < 6; ++b) acc[q++] += J[a] * J[b];
#pragma unroll
        for (int a = 0; a < 6; ++a) acc[21 + a] += J[a] * r;
    }
    if (MODE == 2) return;
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    double* out = w.part + ((size_t)h * nch_max + c) * NPART;
    if (MODE == 0) {
#pragma unroll
        for (int q = 0; q < NMOM; ++q) {
            const double v = wave_sum_f64(acc[q]);
            if (lane == 0) red[wv][q] = v;
        }
    }
    const double pv = wave_sum_f64((double)pairs);
    if (lane == 0) red[wv][NMOM] = pv;
    __syncthreads();
    if (threadIdx.x < NPART && (MODE == 0 || threadIdx.x == NMOM)) {
        double v = 0.0;
        for (int k = 0; k < RNT / 64; ++k) v += red[k][threadIdx.x];
        out[threadIdx.x] = v;
    }
}

// one thread per hypothesis: sum the chunks in order, Cholesky, T <- T . [dR^T | -dR^T tau]
__global__ __launch_bounds__(64) void refine_solve_kernel(const int32_t* __restrict__ count, int cap, const int32_t* __restrict__ nh,
                                                          int NR, int nch_max, Work w) {
    const int h = blockIdx.x * 64 + threadIdx.x;
    if (h >= NR || !w.active[h]) return;
    const int nch = (min(count[0], cap) + RCH - 1) / RCH;
    double m[NPART];
    for (int q = 0; q < NPART; ++q) m[q] = 0.0;
    for (int c = 0; c < nch; ++c) {
        const double* p = w.part + ((size_t)h * nch_max + c) * NPART;
        for (int q = 0; q < NPART; ++q) m[q] += p[q];
    }
    if (m[NMOM] < 6.0) {
        w.active[h] = 0;
        return;
    }
    double A[6][6], g[6];
    int q = 0;
    for (int a = 0; a < 6; ++a)
        for (int b = a; b < 6; ++b) A[a][b] = A[b][a] = m[q++];
    for (int a = 0; a < 6; ++a) g[a] = m[21 + a];
    const double tol = 1e-12 * (((((A[0][0] + A[1][1]) + A[2][2]) + A[3][3]) + A[4][4]) + A[5][5]) / 6.0;
    double L[6][6];
    for (int j = 0; j < 6; ++j) {
        double s = A[j][j];
        for (int k = 0; k < j; ++k) s -= L[j][k] * L[j][k];
        if (!(s > tol)) {
            w.active[h] = 0;
            return;
        }
        L[j][j] = sqrt(s);
        for (int i = j + 1; i < 6; ++i) {
            double t = A[i][j];
            for (int k = 0; k < j; ++k) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    double y[6], d[6];
    for (int i = 0; i < 6; ++i) {
        double t = -g[i];
        for (int k = 0; k < i; ++k) t -= L[i][k] * y[k];
        y[i] = t / L[i][i];
    }
    for (int i = 5; i >= 0; --i) {
        double t = y[i];
        for (int k = i + 1; k < 6; ++k) t -= L[k][i] * d[k];
        d[i] = t / L[i][i];
    }
    // dR = Rodrigues(omega)
    const double wx = d[0], wy = d[1], wz = d[2];
    const double th = sqrt((wx * wx + wy * wy) + wz * wz);
    double dR[9];
    if (th < 1e-12) {
        const double v[9] = {1.0, -wz, wy, wz, 1.0, -wx, -wy, wx, 1.0};
        for (int k = 0; k < 9; ++k) dR[k] = v[k];
    } else {
        const double kx = wx / th, ky = wy / th, kz = wz / th, sn = sin(th), cs1 = 1.0 - cos(th);
        const double K[9] = {0.0, -kz, ky, kz, 0.0, -kx, -ky, kx, 0.0};
        for (int a = 0; a < 3; ++a)
            for (int b = 0; b < 3; ++b) {
                const double k2 = (K[3 * a] * K[b] + K[3 * a + 1] * K[3 + b]) + K[3 * a + 2] * K[6 + b];
                dR[3 * a + b] = ((a == b ? 1.0 : 0.0) + sn * K[3 * a + b]) + cs1 * k2;
            }
    }
    double* T = w.pose + 16 * (size_t)h;
    double R[9], Rn[9];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) R[3 * a + b] = T[4 * a + b];
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Rn[3 * a + b] = (R[3 * a] * dR[3 * b] + R[3 * a + 1] * dR[3 * b + 1]) + R[3 * a + 2] * dR[3 * b + 2];
    for (int a = 0; a < 3; ++a) {
        T[4 * a + 3] = T[4 * a + 3] - ((Rn[3 * a] * d[3] + Rn[3 * a + 1] * d[4]) + Rn[3 * a + 2] * d[5]);
        for (int b = 0; b < 3; ++b) T[4 * a + b] = Rn[3 * a + b];
    }
    double Tl[16];
    for (int k = 0; k < 16; ++k) Tl[k] = T[k];
    write_inverse(Tl, w.inv + 12 * (size_t)h);
    w.done[h] += 1;
    (void)nh;
}

// one workgroup: pair counts per hypothesis (chunks in order), bitonic sort by (pairs descending, input rank), outputs
__global__ __launch_bounds__(1024) void refine_final_kernel(const int32_t* __restrict__ count, int cap,
                                                            const int32_t* __restrict__ nh, int NR, int nch_max, int Mr, Work w,
                                                            double* __restrict__ poses_out, double* __restrict__ scores,
                                                            int32_t* __restrict__ pairs_out, int32_t* __restrict__ steps_out) {
    __shared__ unsigned long long key[MAX_RESULTS];
    const int n = n_hyp(nh, NR);
    const bool sok = scene_ok(count, cap);
    const int nch = sok ? (count[0] + RCH - 1) / RCH : 0;
    int np2 = 2;
    while (np2 < n) np2 <<= 1;
    for (int h = threadIdx.x; h < np2; h += 1024) {
        unsigned long long k = ~0ull;
        if (h < n) {
            double s = 0.0;
            for (int c = 0; c < nch; ++c) s += w.part[((size_t)h * nch_max + c) * NPART + NMOM];
            k = ((unsigned long long)(~(uint32_t)s) << 32) | (unsigned)h;
        }
        key[h] = k;
    }
    __syncthreads();
    wg_bitonic_sort(key, np2);
    for (int r = threadIdx.x; r < NR; r += 1024) {
        if (r < n) {
            const int h = (int)(key[r] & 0xffffffffu);
            const uint32_t p = ~(uint32_t)(key[r] >> 32);
            for (int q = 0; q < 16; ++q) poses_out[16 * (size_t)r + q] = w.pose[16 * (size_t)h + q];
            scores[r] = (double)p / (double)Mr;
            pairs_out[r] = (int32_t)p;
            steps_out[r] = w.done[h];
        } else {
            for (int q = 0; q < 16; ++q) poses_out[16 * (size_t)r + q] = 0.0;
            scores[r] = 0.0;
            pairs_out[r] = 0;
            steps_out[r] = 0;
        }
    }
}

int nch_of(int cap) { return (cap + RCH - 1) / RCH; }

}  // namespace

extern "C" {

size_t ossid_ppf_refine_grid_bytes(int Mr, int steps, float D, float h) {
    if (!args_ok(Mr, steps, D, h)) return 0;
    return grid_bytes(Mr, n_levels(steps, D, h));
}

int ossid_ppf_refine_model_grid(const float* points, const float* normals, int Mr, int steps, float D, float h, void* grid,
                                size_t grid_bytes_, void* stream) {
    const size_t need = ossid_ppf_refine_grid_bytes(Mr, steps, D, h);
    if (need == 0 || !points || !normals || !grid || grid_bytes_ < need) return OSSID_EINVAL;
    const int nlev = n_levels(steps, D, h);
    Thr thr;
    for (int l = 0; l < MAX_LEVELS; ++l) thr.t[l] = l < nlev ? (float)thr_f64(l, D, h) : 0.0f;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(refine_grid_setup_kernel, dim3(1), dim3(GNT), 0, st, points, normals, Mr, nlev, thr, grid);
    hipLaunchKernelGGL(refine_grid_sort_kernel, dim3(nlev), dim3(GNT), 0, st, Mr, grid, level_bytes(Mr));
    return ossid_launch_status();
}

size_t ossid_ppf_refine_workspace_bytes(int cap, int num_poses) {
    if (cap <= 0 || cap > OSSID_PPF_MAX_REFINE_SCENE_POINTS || num_poses <= 0 || num_poses > MAX_RESULTS) return 0;
    return work_bytes(num_poses, nch_of(cap));
}

int ossid_ppf_refine(const float* scene, const int32_t* count, int cap, const void* grid, size_t grid_bytes_, int Mr,
                     const double* poses_in, const int32_t* num_hyp, int num_poses, int steps, float D, float h,
                     void* workspace, size_t workspace_bytes, double* poses_out, double* scores, int32_t* pairs,
                     int32_t* steps_done, int32_t* status, void* stream) {
    const size_t need = ossid_ppf_refine_workspace_bytes(cap, num_poses);
    const size_t gneed = ossid_ppf_refine_grid_bytes(Mr, steps, D, h);
    if (need == 0 || gneed == 0 || !scene || !count || !grid || grid_bytes_ < gneed || !poses_in || !num_hyp ||
        !workspace || workspace_bytes < need || !poses_out || !scores || !pairs || !steps_done || !status)
        return OSSID_EINVAL;
    const int NR = num_poses, nch = nch_of(cap), nlev = n_levels(steps, D, h);
    const Work w = carve(workspace, NR, nch);
    const GridView g = grid_view(grid, Mr, nlev);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(refine_init_kernel, dim3((NR + 255) / 256), dim3(256), 0, st, poses_in, num_hyp, count, cap, NR, w, status);
    for (int k = 0; k < steps; ++k) {
        const float thr = (float)thr_f64(k, D, h);
        const float thr2 = (float)((double)thr * (double)thr);
        hipLaunchKernelGGL(refine_corr_kernel<0>, dim3(nch, NR), dim3(RNT), 0, st, scene, count, cap, g, level_of(k, D, h), thr2,
                           num_hyp, NR, nch, w, (int32_t*)nullptr);
        hipLaunchKernelGGL(refine_solve_kernel, dim3((NR + 63) / 64), dim3(64), 0, st, count, cap, num_hyp, NR, nch, w);
    }
    const float thr = (float)thr_f64(steps - 1, D, h);
    hipLaunchKernelGGL(refine_corr_kernel<1>, dim3(nch, NR), dim3(RNT), 0, st, scene, count, cap, g, level_of(steps - 1, D, h),
                       (float)((double)thr * (double)thr), num_hyp, NR, nch, w, (int32_t*)nullptr);
    hipLaunchKernelGGL(refine_final_kernel, dim3(1), dim3(1024), 0, st, count, cap, num_hyp, NR, nch, Mr, w, poses_out, scores,
                       pairs, steps_done);
    return ossid_launch_status();
}

int ossid_ppf_refine_match(const float* scene, const int32_t* count, int cap, const void* grid, size_t grid_bytes_, int Mr,
                           const double* poses, int num_poses, int steps, int step, float D, float h, void* workspace,
                           size_t workspace_bytes, int32_t* match, void* stream) {
    const size_t need = ossid_ppf_refine_workspace_bytes(cap, num_poses);
    const size_t gneed = ossid_ppf_refine_grid_bytes(Mr, steps, D, h);
    if (need == 0 || gneed == 0 || step < 0 || step >= steps || !scene || !count || !grid || grid_bytes_ < gneed || !poses ||
        !workspace || workspace_bytes < need || !match)
        return OSSID_EINVAL;
    const int NR = num_poses, nch = nch_of(cap), nlev = n_levels(steps, D, h);
    const Work w = carve(workspace, NR, nch);
    const GridView g = grid_view(grid, Mr, nlev);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(refine_init_kernel, dim3((NR + 255) / 256), dim3(256), 0, st, poses, (const int32_t*)nullptr, count, cap, NR,
                       w, (int32_t*)nullptr);
    const float thr = (float)thr_f64(step, D, h);
    hipLaunchKernelGGL(refine_corr_kernel<2>, dim3(nch, NR), dim3(RNT), 0, st, scene, count, cap, g, level_of(step, D, h),
                       (float)((double)thr * (double)thr), (const int32_t*)nullptr, NR, nch, w, match);
    return ossid_launch_status();
}

}  // extern "C"
